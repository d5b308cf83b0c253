"""CPU tests of the linear / affine / constant control plan (plan_affine_native.py): eligibility reasons, plan choice, the
size query of the C ABI, the chain rule of a Linear control with G != I and the importance-sampling step map."""
import ctypes as C

import pytest
import torch

from affine_cases import build_modules, gain_matrices
from util_cases import psp

aff = psp.plan_affine_native
nat = psp.native
CPU = torch.device("cpu")


def make(kind="Linear", d=4, problem=None, control=None, **kw):
    prob = problem if problem is not None else psp.LQGC(d=d, off_diag=0.1, T=0.1, seed=42, delta_t=0.005, device=CPU)
    args = dict(lr=0.1, L=1, K=16, delta_t=0.01, time_approx="outer", verbose=False, device=CPU)
    args.update(kw)
    model = psp.Solver(name="aff", problem=prob, **args)
    if kind is not None:
        model.z_n = build_modules(control or dict(kind=kind), prob.d, model.N, model.lr, 42)
        model.update_Phis()
    return model


def test_the_three_lists_are_eligible_up_to_the_device():
    for kind in ("Linear", "Affine", "Constant"):
        model = make(kind)
        assert aff.affine_configuration_reason(model) is None
        assert "needs a GPU" in aff.affine_eligibility(model)
    for loss in ("moment", "variance", "cross_entropy", "relative_entropy"):
        assert aff.affine_configuration_reason(make("Linear", loss_method=loss)) is None
    assert aff.affine_configuration_reason(make("Linear", adaptive_forward_process=True, detach_forward=False)) is None
    assert aff.affine_configuration_reason(make("Constant", problem=psp.LLGC(d=3, off_diag=0.05, T=0.1, seed=42, device=CPU))) is None


def _declined():
    """(tag, model, a word of the reason) for every configuration the plan declines."""
    out = []
    m = make("Linear")
    m.approx_method = "value_function"
    out.append(("value_function", m, "approx_method"))
    m = make("Linear")
    m.time_approx = "inner"
    out.append(("inner", m, "time_approx='outer'"))
    out.append(("densenet_list", make(None), "not a list of modules of exactly one"))
    m = make("Linear")
    m.z_n[1] = psp.Affine(d=4, lr=0.1)
    out.append(("mixed_classes", m, "exactly one"))
    m = make("Affine")
    m.z_n[0].forward = lambda x: x
    out.append(("forward_overridden", m, "class forward"))

    class MyLinear(psp.Linear):
        def forward(self, x):
            return x
    m = make("Linear")
    m.z_n = [MyLinear(d=4, B=torch.eye(4), Q=torch.eye(4), lr=0.1) for _ in range(m.N)]
    out.append(("subclass", m, "exactly one"))
    m = make("Linear")
    m.z_n = m.z_n[:-1]
    out.append(("one_module_short", m, "one module per time step"))
    out.append(("d_65", make("Constant", problem=psp.LLGC(d=65, off_diag=0.01, T=0.1, seed=42, device=CPU)), "d <= 64"))
    out.append(("reparametrization", make("Linear", loss_method="reparametrization"), "loss_method"))
    m = make("Linear", loss_method="relative_entropy")
    m.adaptive_forward_process = False
    out.append(("relent_nonadaptive", m, "non-adaptive"))
    out.append(("burgers", make("Linear", burgers_drift=True), "diagnostics"))
    out.append(("log_gradient", make("Linear", log_gradient=True), "diagnostics"))
    out.append(("gradient_variance", make("Linear", compute_gradient_variance=3), "diagnostics"))
    out.append(("metastability", make("Linear", metastability_logs=(torch.zeros(4), 0.1)), "diagnostics"))
    out.append(("bf16", make("Linear", mlp_dtype="bf16"), "fp32 only"))
    out.append(("f16x3", make("Linear", mlp_dtype="f16x3"), "fp32 only"))
    prob = psp.LQGC(d=4, off_diag=0.1, T=0.1, seed=42, delta_t=0.005, device=CPU)
    prob.native_spec = lambda: None
    out.append(("no_native_spec", make("Linear", problem=prob), "native_spec"))
    prob = psp.LLGC(d=4, off_diag=0.1, T=0.1, seed=42, device=CPU)
    prob.u_true_tables = lambda: dict(tables=[[[0.0]]], group_of_dim=[0] * 4, xb=1.0, dx=0.1, delta_t=0.01)
    out.append(("ul2_grid", make("Constant", problem=prob), "PSP_UL2_GRID"))
    prob = psp.LLGC(d=4, off_diag=0.1, T=0.1, seed=42, device=CPU)
    prob.u_true_x_independent = False
    out.append(("ul2_host", make("Constant", problem=prob), "u_l2_error_flag"))
    # the notebooks' commented-out SGD variant
    m = make("Linear")
    for z in m.z_n:
        z.optim = torch.optim.SGD(z.parameters(), lr=0.1)
    out.append(("sgd", m, "plain torch.optim.Adam"))
    m = make("Linear")
    m.z_n[2].optim.param_groups[0]["lr"] = 0.05
    out.append(("unequal_lr", m, "different Adam settings"))
    m = make("Linear")
    m.z_n[0].optim = torch.optim.Adam(m.z_n[0].parameters(), lr=0.1, weight_decay=0.01)
    out.append(("weight_decay", m, "weight_decay"))
    out.append(("path_budget", make("Linear", path_budget_bytes=1000), "does not chunk"))
    return out


def test_every_declined_configuration_has_its_reason():
    seen = set()
    for tag, model, word in _declined():
        reason = aff.affine_configuration_reason(model)
        assert reason is not None and word in reason, (tag, reason)
        seen.add(tag)
    assert len(seen) == 23


def test_overridden_problem_coefficient_is_declined():
    prob = psp.LQGC(d=4, off_diag=0.1, T=0.1, seed=42, delta_t=0.005, device=CPU)
    prob.b = lambda x: 0.0 * x
    reason = aff.affine_configuration_reason(make("Linear", problem=prob))
    assert reason is not None and "catalogue implementation" in reason


def test_plan_choice_of_other_controls_is_unchanged():
    """The default Solver(name, LQGC(...)) (a DenseNet list) and a swapped DenseNet list keep the DenseNet plan's verdict; a
    Linear list gets this plan's; under backend='auto' all of them run the composite plan on a CPU."""
    default = make(None)
    default._choose_plan()
    assert default.plan_name == "torch" and default.plan_reason == psp.plan_dense_native.dense_eligibility(default)
    swapped = make(None)
    swapped.z_n = [psp.DenseNet(d_in=4, d_out=4, lr=0.1, arch=[8, 8], seed=n) for n in range(swapped.N)]
    swapped.update_Phis()
    swapped._choose_plan()
    assert swapped.plan_name == "torch" and swapped.plan_reason == psp.plan_dense_native.dense_eligibility(swapped)
    lin = make("Linear")
    lin._choose_plan()
    assert lin.plan_name == "torch" and lin.plan_reason == aff.affine_eligibility(lin)
    with pytest.raises(psp.plan_native.PlanUnsupported, match="needs a GPU"):
        make("Linear", backend="native")._choose_plan()
    lin.train()                                           # composite, exactly as before
    assert len(lin.loss_log) == 1


def _config(d=16, d_real=5, K=37, N=5, **kw):
    cfg = nat.AffConfig()
    cfg.struct_bytes = C.sizeof(nat.AffConfig)
    b = cfg.base
    b.d, b.H, b.K_local, b.N, b.K_global = d, 0, K, N, K
    b.dt, b.sqrt_dt, b.store_path = 0.01, 0.1, 1
    cfg.d_real, cfg.has_matrix, cfg.has_bias = d_real, 1, 0
    for k, v in kw.items():
        setattr(cfg if hasattr(nat.AffConfig, k) and k != "base" else b, k, v)
    return cfg


def test_query_accepts_and_rejects_without_a_gpu():
    lib = nat.load()
    assert nat.aff_instances() == [16, 32, 64]
    sizes = nat.AffSizes()
    cfg = _config()
    assert lib.psp_aff_query(C.byref(cfg), C.byref(sizes)) == 0
    assert sizes.path_bytes == 5 * 37 * 2 * 16 * 4 and sizes.padded_params == 16 * 16 + 16
    assert sizes.fwd_partial_bytes == 16 * sizes.fwd_workgroups and sizes.partial_bytes == 5 * sizes.slices * sizes.padded_params * 4
    assert sizes.slices * 32 >= 37 > (sizes.slices - 1) * 32 and sizes.bwd_workgroups == 5 * sizes.slices
    big = _config(d=64, d_real=64, K=65536, N=50, drift_kind=nat.DRIFT_DENSE, sigma_kind=nat.SIGMA_DENSE)
    big.base.u_l2_out, big.ul2_kind, big.ul2_ref = 8, nat.UL2_LINEAR, 8          # (never dereferenced by the query)
    assert lib.psp_aff_query(C.byref(big), C.byref(sizes)) == 0
    assert sizes.fwd_threads == 256 and sizes.lds_bytes <= 160 * 1024
    rejects = [(_config(H=30), -3, "base.H"), (_config(mlp_dtype=nat.MLP_F16X3), -3, "fp32"), (_config(d=48), -2, "bucket"),
               (_config(d_real=17), -1, "d_real"), (_config(struct_bytes=8), -1, "struct_bytes"),
               (_config(has_matrix=0), -1, "has_matrix or has_bias"), (_config(drift_kind=7), -1, "enum"),
               (_config(store_path=4), -1, "enum"), (_config(K_local=0), -1, "non-positive")]
    grid = _config(u_l2_out=8, ul2_kind=nat.UL2_GRID, ul2_ref=8)
    rejects.append((grid, -3, "PSP_UL2_GRID"))
    rejects.append((_config(u_l2_out=8, ul2_kind=nat.UL2_TABLE), -1, "ul2_ref"))
    for cfg, code, word in rejects:
        assert lib.psp_aff_query(C.byref(cfg), C.byref(sizes)) == code
        assert word in nat.last_error(), nat.last_error()
    assert lib.psp_aff_query(None, C.byref(sizes)) == -1


def test_chain_rule_of_a_linear_control_against_autograd():
    """dF = G^T dM with G = Q^-1 B^T for random well-conditioned B, Q: the gradient of a scalar function of Linear.forward."""
    d, N, K = 7, 3, 11
    mods = build_modules(dict(kind="Linear", gains=3), d, N, 0.1, 42)
    B, Q = gain_matrices(d, 3)
    assert float(torch.linalg.cond(B)) < 4 and float(torch.linalg.cond(Q)) < 4
    G = aff.linear_gains(mods, CPU)
    assert G is not None and G.shape == (N, d, d)
    g = torch.Generator().manual_seed(0)
    X, W = torch.randn(N, K, d, generator=g), torch.randn(N, K, d, generator=g)
    loss = sum((mods[n](X[n]) * W[n]).sum() for n in range(N))
    loss.backward()
    F = torch.stack([m.F.detach() for m in mods])
    M = aff.effective_map(G, F)
    for n in range(N):
        assert torch.allclose(mods[n](X[n]).detach(), X[n] @ M[n].t(), atol=1e-5)
    dM = torch.einsum("nki,nkj->nij", W, X)               # d loss / d M_n for Z = M X
    dF = aff.chain_rule(G, dM)
    want = torch.stack([m.F.grad for m in mods])
    assert float((dF - want).abs().max()) <= 1e-5 * float(want.abs().max())
    # G = I: the product is skipped, M is F itself
    eye_mods = build_modules(dict(kind="Linear"), d, N, 0.1, 42)
    assert aff.linear_gains(eye_mods, CPU) is None
    assert aff.effective_map(None, F) is F and aff.chain_rule(None, dM) is dM


@pytest.mark.parametrize("kind", ["Linear", "Constant"])
def test_importance_sampling_tables_follow_the_step_map(kind):
    """The gains / rows handed to psp_is_rollout reproduce -Z_n(X, n delta) on probe points, on evaluation grids finer and
    coarser than the training grid."""
    d = 4
    model = make(kind, d=d, control=dict(kind=kind, gains=5) if kind == "Linear" else None)
    for n, z in enumerate(model.z_n):                     # distinct modules, so that a wrong index shows
        with torch.no_grad():
            for p in z.parameters():
                p.add_(0.1 * n)
    xp = torch.randn(5, d, generator=torch.Generator().manual_seed(7))
    for delta in (0.004, 0.01, 0.025):
        N_eval = int(-(-model.T // delta))
        code, table = aff.is_control_tables(model, N_eval, delta)
        assert code == (nat.ISC_LINEAR if kind == "Linear" else nat.ISC_TABLE) and table.shape[0] == N_eval
        idx = aff.step_index(model, N_eval, delta)
        assert idx[0] == 0 and max(idx) <= model.N - 1 and idx == sorted(idx)
        for n in range(N_eval):
            with torch.no_grad():
                want = -model.Z_n(xp, n * delta)
            got = xp @ table[n].t() if kind == "Linear" else table[n].expand_as(want)
            assert torch.allclose(got, want, atol=1e-5), (delta, n)
    assert aff.is_control_tables(make("Affine"), 10, 0.01) is None
    assert aff.is_control_tables(make(None), 10, 0.01) is None
