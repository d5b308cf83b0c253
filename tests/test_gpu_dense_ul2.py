"""GPU: the u_L2 log of the DenseNet-control forward (hjbd_fwd_kernel<.., LOGU>, include/psp.h PSP_UL2_*) -- the default
Solver constructor (u_l2_error_flag on whenever the problem has u_true) plans 'native' for the three kinds of reference control:
a table of u*(t_n) (LLGC), the gains of a u* linear in x (LQGC), the double wells' grid tables.  Fixtures: the reference's own
runs (tests/golden/make_golden_ul2.py)."""
import math

import pytest
import torch

from conftest import load_golden
from test_dense_ul2_reference import emulate_u
from util_cases import make_pkg_solver, psp

pytestmark = pytest.mark.gpu
CASES = ["llgc_d12_outer_ul2", "lqgc_d10_outer_ul2", "dw_d6_mixed_outer_ul2", "dw1d_densenet_inner_ul2", "llgc_d100_outer_ul2"]
BIG = 7.0e4


def dev():
    return torch.device("cuda:0")


def _native(model):
    assert model.plan_name == "native", model.plan_reason
    assert isinstance(model._native_plan, psp.plan_dense_native.DenseNativePlan)
    return model._native_plan


@pytest.mark.parametrize("mlp", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", CASES)
def test_fixture_u_l2_and_loss_match_reference(name, mlp):
    rec = load_golden(name)
    model = make_pkg_solver(rec["case"], dev(), backend="native", mlp_dtype=mlp)
    model.train()
    plan = _native(model)
    assert plan.matrix_mode == mlp and plan.ul2 is not None
    exp = rec["expected"]
    assert len(model.u_L2_loss) == len(exp["u_L2_loss"])
    for l, (got, want) in enumerate(zip(model.u_L2_loss, exp["u_L2_loss"])):
        assert math.isclose(got, want, rel_tol=1e-4), (l, model.u_L2_loss, exp["u_L2_loss"])
    for l, (got, want) in enumerate(zip(model.loss_log, exp["loss_log"])):
        assert math.isclose(got, want, rel_tol=1e-4), (l, model.loss_log, exp["loss_log"])
    for got, want in zip(model.Y_0_log, exp["Y_0_log"]):
        assert math.isclose(got, want, rel_tol=1e-4, abs_tol=1e-6)
    if exp["probes"]:
        xp = torch.tensor(exp["probe_x"]).reshape(-1, model.d).to(dev())
        for pr in exp["probes"]:
            with torch.no_grad():
                u = (-model.Z_n(xp, pr["t"])).cpu()
            want = torch.tensor(pr["minus_Z"]).reshape(u.shape)
            assert float((u - want).abs().max()) <= 1e-4 * max(1e-2, float(want.abs().max()))


def _images_X(plan, N, K, d):
    """X_n (N, K, d) from the register images of the rollout: block (n, tile), X image at float 0, image float ks * 64 + 16 q + j
    = feature 4 ks + q of sample j (csrc/hjbd_kernels.h DGeo::pX)."""
    nt = (K + 15) // 16
    KP = plan.d_pad // 4
    blocks = plan.images.view(N, nt, -1)[:, :, :KP * 64].reshape(N, nt, KP, 4, 16)
    return blocks.permute(0, 1, 4, 2, 3).reshape(N, nt * 16, KP * 4)[:, :K, :d]


@pytest.mark.parametrize("mlp", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", CASES[:4])
def test_per_trajectory_log_against_torch(name, mlp):
    """L = 1, attached forward process (X_N is kept): the kernel's per-trajectory sums against a torch evaluation from the
    stored X_n, the nets as they were during the rollout and the builder's u*."""
    rec = load_golden(name)
    model = make_pkg_solver(rec["case"], dev(), backend="native", mlp_dtype=mlp, L=1, detach_forward=False)
    params = list(model.z_n.parameters()) if not isinstance(model.z_n, list) else [p for z in model.z_n for p in z.parameters()]
    p0 = [p.detach().clone() for p in params]
    model.train()
    plan = _native(model)
    assert plan.kernel_bwd and plan.attached
    with torch.no_grad():
        for p, v in zip(params, p0):                     # the parameters of the rollout (before the Adam step)
            p.copy_(v)
        N, K, d = model.N, model.K, model.d
        X = _images_X(plan, N, K, d)
        Xn1 = torch.cat([X[1:], plan.XN_k[:, :d].unsqueeze(0)], 0)
        ref = psp.plan_dense_native.ul2_reference(model.problem, N, model.delta_t_np, plan.d_pad, K, 0)
        want = torch.zeros(K, dtype=torch.float64)
        for n in range(N):
            Z = model.Z_n_(X[n], n)
            xp = torch.zeros(K, plan.d_pad)
            xp[:, :d] = Xn1[n].cpu()
            u = emulate_u(ref, xp, n)[:, :d].to(dev())
            want += (((-Z - u) ** 2).sum(1) * model.delta_t).double().cpu()
    got = plan.ul2.double().cpu()
    # element by element: 1e-5 relative, with an absolute floor far below any trajectory's own value
    bad = (got - want).abs() > 1e-5 * want.abs() + 1e-9 * float(want.abs().max())
    assert not bool(bad.any()), (got[bad][:4], want[bad][:4])
    assert math.isclose(model.u_L2_loss[0], float(want.mean()), rel_tol=1e-5)


@pytest.mark.parametrize("name", CASES[:4])
def test_native_log_matches_composite(name):
    rec = load_golden(name)
    nat_m = make_pkg_solver(rec["case"], dev(), backend="native", mlp_dtype="fp32", noise="reference")
    nat_m.train()
    _native(nat_m)
    cmp_m = make_pkg_solver(rec["case"], dev(), backend="torch", noise="reference")
    cmp_m.train()
    assert cmp_m.plan_name == "torch"
    for l, (a, b) in enumerate(zip(nat_m.u_L2_loss, cmp_m.u_L2_loss)):
        assert math.isclose(a, b, rel_tol=1e-5), (l, nat_m.u_L2_loss, cmp_m.u_L2_loss)


@pytest.mark.parametrize("name", ["llgc_d12_outer_ul2", "lqgc_d10_outer_ul2", "dw_d6_mixed_outer_ul2"])
def test_log_is_a_diagnostic(name):
    """Same seed with the log on and off: the same losses and final parameters (the log only reads the rollout)."""
    rec = load_golden(name)
    on = make_pkg_solver(rec["case"], dev(), backend="native")
    off = make_pkg_solver(rec["case"], dev(), backend="native", u_l2_error_flag=False)
    on.train()
    off.train()
    assert _native(on).ul2 is not None and _native(off).ul2 is None
    assert on.loss_log == off.loss_log
    assert torch.equal(on._native_plan.flat, off._native_plan.flat)
    assert all(v == 0.0 for v in off.u_L2_loss) and all(v > 0.0 for v in on.u_L2_loss)


def test_guarded_rollout_logs_the_fp32_value():
    """Range guard tripped (the scaled-down-net recipe of test_gpu_range_guard.py): the predicated fp32-MFMA rerun overwrites the
    per-trajectory log, so u_L2 is the fp32 value and not NaN."""
    rec = load_golden("llgc_d12_outer_ul2")

    def run(mlp, **kw):
        model = make_pkg_solver(rec["case"], dev(), backend="native", mlp_dtype=mlp, L=2, **kw)
        with torch.no_grad():
            for net in model.z_n:
                for p in net.parameters():
                    p.mul_(1e-2)
        x0 = model.X_0.clone()
        x0[3] = BIG
        model.X_0 = x0
        model.train()
        _native(model)
        return model

    ref, got = run("fp32"), run("f16x3")
    assert got._native_plan.matrix_mode == "f16x3" and got.range_fallback_iterations == 2
    assert all(math.isfinite(v) for v in ref.u_L2_loss), ref.u_L2_loss
    assert got.u_L2_loss == ref.u_L2_loss and got.loss_log == ref.loss_log


def test_default_constructor_plans_native():
    """The issue's two examples: LLGC d = 100 with nothing but K and delta_t, and the LQGC notebook cell with L reduced."""
    prob = psp.LLGC(d=100, off_diag=0.01, T=0.5, device=dev())
    m = psp.Solver("x", prob, K=64, L=1, delta_t=0.01, device=dev(), verbose=False)
    m.train()
    assert m.plan_name == "native" and m.u_l2_error_flag and math.isfinite(m.u_L2_loss[0]) and m.u_L2_loss[0] > 0
    lq = psp.LQGC(d=10, off_diag=0.1, T=0.5, delta_t=0.005, device=dev())
    m = psp.Solver("x", lq, K=500, L=2, lr=0.003, delta_t=0.01, loss_method="moment", learn_Y_0=True, detach_forward=True,
                   device=dev(), verbose=False)
    m.train()
    assert m.plan_name == "native" and m.u_l2_error_flag and all(math.isfinite(v) and v > 0 for v in m.u_L2_loss)


def _wide_problem(kind):
    if kind == "llgc":
        return dict(kind="LLGC", kwargs=dict(d=140, off_diag=0.01, T=0.1, seed=42))
    if kind == "lqgc":
        return dict(kind="LQGC", kwargs=dict(d=140, off_diag=0.05, T=0.1, seed=42, delta_t=0.005))
    return dict(kind="DoubleWell_multidim", kwargs=dict(d=140, d_1=70, d_2=70, T=0.1, eta=0.5, kappa=2.0),
                calls=[["compute_reference_solution", dict(nx=300)], ["compute_reference_solution_2", dict(nx=300)]])


@pytest.mark.parametrize("mlp", ["fp32", "f16x3"])
@pytest.mark.parametrize("kind", ["llgc", "lqgc", "dw"])
def test_wide_instance_log_matches_composite(kind, mlp):
    """d = 140 runs on the (256, 32) instance: the d > 128 side of the kernel (kind 0 summed per state block, -Z_n of kinds 1 / 2
    in registers) against the composite plan on the same reference noise."""
    case = dict(name="wide_ul2_" + kind, problem=_wide_problem(kind),
                solver=dict(loss_method="log-variance", time_approx="outer", detach_forward=True, L=2, lr=0.002, K=48,
                            delta_t=0.01, seed=42))
    nat_m = make_pkg_solver(case, dev(), backend="native", mlp_dtype=mlp, noise="reference")
    nat_m.train()
    plan = _native(nat_m)
    assert plan.d_pad == 256 and plan.matrix_mode == mlp and plan.ul2 is not None
    cmp_m = make_pkg_solver(case, dev(), backend="torch", noise="reference")
    cmp_m.train()
    assert cmp_m.plan_name == "torch"
    tol = 1e-5 if mlp == "fp32" else 1e-4
    assert all(v > 0 for v in cmp_m.u_L2_loss)
    for l, (a, b) in enumerate(zip(nat_m.u_L2_loss, cmp_m.u_L2_loss)):
        assert math.isclose(a, b, rel_tol=tol), (l, nat_m.u_L2_loss, cmp_m.u_L2_loss)
    # (the loss itself only as a sanity check: at d = 140 the composite plan forms the log-variance of D ~ 1e2..1e3 in fp32 and
    #  loses ~1e-4 to cancellation, where the kernel's sums are fp64; loss parity is the business of the reference fixtures)
    for a, b in zip(nat_m.loss_log, cmp_m.loss_log):
        assert math.isclose(a, b, rel_tol=1e-3)
