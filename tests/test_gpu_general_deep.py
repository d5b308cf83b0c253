"""GPU parity of the run-time-shaped value-net kernels (csrc/genl_kernels.h, plan_general_deep.py): GeneralSolver /
EllipticSolver with V = DenseNet of one to four hidden layers -- the nets the reference's diffusion-loss notebooks swap into
model.V (function_space.py:116-140; Allen-Cahn.ipynb:72 arch = [110, 110, 50]) -- against the oracle's autograd and the
reference's golden runs.  Tolerances as for the two-hidden-layer kernels (test_gpu_general.py): gradient <= 5e-4 * max|g|,
loss per iteration <= 1e-4 relative, active-step counts exact."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_general_composite_golden import DEEP, DEEP_BOUNDED, DEEP_ELLIPTIC, R4_GENERAL, build as build_pkg
from test_gpu_bounded_elliptic import oracle_run
from util_cases import psp

pytestmark = pytest.mark.gpu
ALL = DEEP + DEEP_BOUNDED + DEEP_ELLIPTIC + ["allencahn_d10_densenet_tanh_diffusion"]     # (DenseNet_tanh: nn.Linear weights)


def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", ALL)
def test_first_iteration_gradient_matches_oracle(name):
    case = load_golden(name)["case"]
    prob, model = build_pkg(case, device=dev(), backend="native", L=1)
    model.train()
    assert model.plan_name == "native" and type(model._gen_plan).__name__ == "GeneralDeepPlan"
    ref = oracle_run(case, 1)
    assert model.K_log == ref["K_log"]
    assert math.isclose(model.loss_log[0], ref["loss_log"][0], rel_tol=5e-5), (model.loss_log, ref["loss_log"])
    g_ref = torch.cat([g.reshape(-1) for g in ref["traces"][0]["grads"]])
    g = model._gen_plan.grad.cpu()
    assert g.shape == g_ref.shape
    err = float((g - g_ref).abs().max()) / float(g_ref.abs().max())
    print("%s: gradient rel err %.2e" % (name, err))
    assert err <= 5e-4, err


@pytest.mark.parametrize("name", ALL)
def test_loss_log_matches_reference_golden(name):
    rec = load_golden(name)
    prob, model = build_pkg(rec["case"], device=dev(), backend="native")
    model.train()
    assert type(model._gen_plan).__name__ == "GeneralDeepPlan"
    exp = rec["expected"]
    assert model.K_log == exp["K_log"]
    errs = [abs(a - b) / abs(b) for a, b in zip(model.loss_log, exp["loss_log"])]
    print("%s: loss rel err per iteration %s" % (name, ["%.1e" % e for e in errs]))
    assert max(errs) <= 1e-4, (model.loss_log, exp["loss_log"])
    xp = torch.tensor(exp["probe_x"]).reshape(-1, prob.d)
    if rec["case"]["family"] != "elliptic":
        xp = torch.cat([xp, torch.full((xp.shape[0], 1), exp["probe_t"])], 1)
    with torch.no_grad():
        v = model.V(xp.to(dev())).squeeze().cpu()
    want = torch.tensor(exp["probe_V"])
    assert float((v - want).abs().max()) <= 1e-4 * max(1e-2, float(want.abs().max()))


def test_wave_split_and_launch_groups_agree():
    """The same net through the one-wave and the eight-wave kernels (PSP_GENL_NW), and a net whose weight-gradient tiles need
    several launch groups against the oracle: the work split never changes the result beyond summation order."""
    import os
    case = load_golden("dwgen_d10_arch4_bsde")["case"]            # [30, 30, 30, 30]: small enough for one wave per tile
    grads = {}
    keep = os.environ.get("PSP_GENL_NW")
    try:
        for nw in ("1", "8"):
            os.environ["PSP_GENL_NW"] = nw
            prob, model = build_pkg(case, device=dev(), backend="native", L=1)
            model.train()
            assert int(model._gen_plan.sizes.waves_per_tile) == int(nw)
            grads[nw] = (model._gen_plan.grad.clone(), model.loss_log[0], model.K_log[0])
    finally:
        if keep is None:
            os.environ.pop("PSP_GENL_NW", None)
        else:
            os.environ["PSP_GENL_NW"] = keep
    (g1, l1, k1), (g8, l8, k8) = grads["1"], grads["8"]
    assert k1 == k8 and math.isclose(l1, l8, rel_tol=2e-6)
    assert float((g1 - g8).abs().max()) <= 2e-5 * float(g1.abs().max())
    # 4 x 128 hidden units at d = 20: 2 + 8 .. blocks per layer -> (2 + 10 + 18 + 26) * 8 + 34 = 482 tiles = two launch groups
    wide = dict(case, net=dict(arch=[128, 128, 128, 128], seed=42),
                problem=dict(kind="DoubleWell_multidim_for_general_solver",
                             kwargs=dict(d=20, d_1=10, d_2=10, T=0.1, eta=0.1, kappa=1, modus="HJB")))
    prob, model = build_pkg(wide, device=dev(), backend="native", L=1)
    model.train()
    assert int(model._gen_plan.sizes.bwd_workgroups) > int(model._gen_plan.grad_partial.numel() // model._gen_plan.P)   # > 1 group
    ref = oracle_run(wide, 1)
    assert model.K_log == ref["K_log"] and math.isclose(model.loss_log[0], ref["loss_log"][0], rel_tol=5e-5)
    g_ref = torch.cat([g.reshape(-1) for g in ref["traces"][0]["grads"]])
    err = float((model._gen_plan.grad.cpu() - g_ref).abs().max()) / float(g_ref.abs().max())
    print("4 x 128 net: gradient rel err %.2e" % err)
    assert err <= 5e-4


class NotebookTanh2(torch.nn.Module):
    """A value net as a notebook would define it for itself (`Committor function.ipynb` cell 1 does): not a class of the
    package -- dense-concat layout, (in, out) weights in a list W, tanh(.)**2.  The plan recognises it by structure and by a
    probe of its forward (plan_general_deep.value_net_spec)."""

    def __init__(self, d_in, arch, lr, seed, power=2):
        super().__init__()
        torch.manual_seed(seed)
        self.nn_dims = [d_in] + list(arch) + [1]
        self.power = power
        self.W = []
        for i in range(len(self.nn_dims) - 1):
            self.W.append(torch.nn.Parameter(torch.randn(sum(self.nn_dims[:i + 1]), self.nn_dims[i + 1]) * 0.1))
            self.W.append(torch.nn.Parameter(torch.zeros(self.nn_dims[i + 1])))
        for i, w in enumerate(self.W):
            self.register_parameter("p%d" % i, w)
        self.optim = torch.optim.Adam(self.parameters(), lr=lr)

    def forward(self, x):
        n = len(self.nn_dims) - 1
        for i in range(n - 1):
            x = torch.cat([x, torch.tanh(x @ self.W[2 * i] + self.W[2 * i + 1]) ** self.power], 1)
        return x @ self.W[2 * n - 2] + self.W[2 * n - 1]


def test_user_defined_dense_concat_net_runs_on_the_kernels():
    rec = load_golden("committor_d10_tanh2_notebook_diffusion")
    case = rec["case"]
    prob, model = build_pkg(case, device=dev(), backend="native")
    model.V = NotebookTanh2(prob.d, case["net"]["arch"], case["solver"]["lr"], case["net"]["seed"]).to(dev())
    model.train()
    assert type(model._gen_plan).__name__ == "GeneralDeepPlan" and model._gen_plan.net_spec["act"] == "tanh2"
    exp = rec["expected"]
    assert model.K_log == exp["K_log"]
    # (two_spheres boundary data hangs on the last bit of a host reduction: the log is compared with the oracle run on THIS machine,
    #  tests/test_gpu_bounded_elliptic.py::test_loss_log_matches_reference_golden)
    want = oracle_run(case, len(exp["loss_log"]))["loss_log"]
    errs = [abs(a - b) / abs(b) for a, b in zip(model.loss_log, want)]
    assert max(errs) <= 1e-4, (model.loss_log, want, exp["loss_log"])
    # a forward the kernels do not implement (tanh cubed) is NOT taken for one they do: composite plan, with a warning
    prob, other = build_pkg(case, device=dev(), backend="auto", L=1)
    other.V = NotebookTanh2(prob.d, case["net"]["arch"], case["solver"]["lr"], case["net"]["seed"], power=3).to(dev())
    with pytest.warns(UserWarning, match="composite torch plan"):
        other.train()
    assert other.plan_name == "torch" and "none of the dense-concat formulas" in other.plan_reason


def test_philox_rollout_is_deterministic_and_shard_independent():
    """On-device noise at the notebook's net: bitwise determinism; the second half of the batch run alone (k_offset) reproduces
    the full run's per-trajectory outputs."""
    import ctypes as C
    nat = psp.native
    case = load_golden("allencahn_d100_notebook_a110")["case"]
    prob, model = build_pkg(case, device=dev(), backend="native", L=1, noise="philox", K=512)
    model.train()
    plan = model._gen_plan
    Y1, V1 = plan.YN.clone(), plan.VN.clone()
    prob2, model2 = build_pkg(case, device=dev(), backend="native", L=1, noise="philox", K=512)
    model2.train()
    assert torch.equal(model2._gen_plan.YN, Y1) and torch.equal(model2._gen_plan.VN, V1)
    assert model2.loss_log == model.loss_log and torch.equal(model2._gen_plan.grad, plan.grad)
    assert torch.isfinite(plan.grad).all() and float(plan.grad.abs().max()) > 0
    # the upper half alone: a fresh solver (the initial weights: the full run's outputs precede its Adam step) with K / 2
    # trajectories, the forward launched through the C ABI at k_offset = K / 2 on the full run's x0 and t0 of those rows
    K = 512
    Xfull = plan._sample_domain_device(0)
    t0full = torch.rand(K, generator=plan._gen, device=dev()) * prob.T
    prob3, half = build_pkg(case, device=dev(), backend="native", L=1, noise="philox", K=K // 2)
    hp = half._choose_plan()
    assert type(hp).__name__ == "GeneralDeepPlan" and hp.K_local == K // 2
    hp.cfg.k_offset = K // 2
    hp.kcount.zero_()
    x0, t0 = Xfull[K // 2:].contiguous(), t0full[K // 2:].contiguous()
    nat.check(nat.load().psp_genl_rollout_fwd(C.byref(hp.gcfg), nat.ptr(hp.flat), nat.ptr(x0), nat.ptr(t0), None,
                                              int(half.seed), 0, nat.ptr(hp.tables), nat.ptr(hp.path), nat.ptr(hp.ahat),
                                              nat.ptr(hp.VN), nat.ptr(hp.YN), nat.ptr(hp.XN_k), nat.ptr(hp.tN), nat.ptr(hp.kcount),
                                              nat.stream_ptr(dev())), "psp_genl_rollout_fwd")
    torch.cuda.synchronize()
    assert torch.equal(hp.YN, Y1[K // 2:]) and torch.equal(hp.VN, V1[K // 2:])


def test_two_hidden_layer_nets_keep_the_templated_kernels():
    case = load_golden("dwgen_d10_diffusion")["case"]
    prob, model = build_pkg(case, device=dev(), backend="native", L=1)
    model.train()
    assert type(model._gen_plan).__name__ == "GeneralNativePlan"
    # ... except where they do not reach: hidden width above 64
    prob, model = build_pkg(case, device=dev(), backend="native", L=1)
    model.V = psp.DenseNet(d_in=prob.d + 1, d_out=1, lr=1e-3, arch=[96, 96], seed=42).to(dev())
    model.train()
    assert type(model._gen_plan).__name__ == "GeneralDeepPlan"


def test_deep_net_agrees_with_the_templated_kernels_on_a_two_layer_net():
    """The same [H, H] net through both kernel families (the deep plan forced): loss and gradient agree to rounding."""
    from path_space_pde_solver_amd import plan_general_deep as pgd
    case = load_golden("dwgen_d10_diffusion")["case"]
    prob, a = build_pkg(case, device=dev(), backend="native", L=1, mlp_dtype="fp32")
    a.train()
    prob, b = build_pkg(case, device=dev(), backend="native", L=1, mlp_dtype="fp32")
    assert pgd.deep_eligibility(b) is None
    b._gen_plan = pgd.GeneralDeepPlan(b)
    b._gen_plan.key = b._plan_key()
    b.train()                                            # (_choose_plan keeps a plan whose key and net still match)
    assert type(b._gen_plan).__name__ == "GeneralDeepPlan"
    assert b.K_log == a.K_log
    assert math.isclose(a.loss_log[0], b.loss_log[0], rel_tol=2e-6)
    ga, gb = a._gen_plan.grad, b._gen_plan.grad
    assert float((ga - gb).abs().max()) <= 2e-5 * float(ga.abs().max())
