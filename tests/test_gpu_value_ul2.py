"""GPU: the u_L2 log of Solver(approx_method='value_function') inside the run-time-shaped forward kernel
(csrc/genl_kernels.h genl_fwd_kernel<NW, false, false, true> / <NW, true, true, true>; include/psp.h psp_genl_ul2; plan_value_native.py)
for the three descriptions of the reference control: a table of u*(t_n) (LLGC), the gains of a u* linear in x (LQGC), the double
wells' grid tables.  Fixtures: the reference's own runs with the u_L2 flag left at its default
(tests/golden/make_golden_value_ul2.py)."""
import copy
import ctypes as C
import math

import pytest
import torch

from conftest import load_golden
from test_dense_ul2_reference import emulate_u
from util_cases import make_pkg_solver, psp

pytestmark = pytest.mark.gpu
nat = psp.native
pvn = psp.plan_value_native

CASES = ["llgc_d8_off_value_ul2", "lqgc_d5_value_ul2", "lqgc_d17_arch3_value_ul2", "dw_d6_mixed_value_ul2", "dw1d_value_ul2",
         "llgc_d8_diag_value_ul2"]
KIND = {"llgc_d8_off_value_ul2": nat.UL2_TABLE, "lqgc_d5_value_ul2": nat.UL2_LINEAR, "lqgc_d17_arch3_value_ul2": nat.UL2_LINEAR,
        "dw_d6_mixed_value_ul2": nat.UL2_GRID, "dw1d_value_ul2": nat.UL2_GRID, "llgc_d8_diag_value_ul2": nat.UL2_TABLE}
LQ = {"llgc_d8_off_value_ul2", "lqgc_d5_value_ul2", "lqgc_d17_arch3_value_ul2"}      # the linear-quadratic instance


def dev():
    return torch.device("cuda:0")


def _native(model, log=True):
    assert model.plan_name == "native", model.plan_reason
    plan = model._native_plan
    assert isinstance(plan, pvn.ValueNativePlan) and plan.deep is not None
    assert (plan.ul2 is not None) == log == (plan.ul2_cfg is not None)
    return plan


def _trained(name, **over):
    model = make_pkg_solver(copy.deepcopy(load_golden(name)["case"]), dev(), backend="native", **over)
    model.train()
    return model


# ---- 1. the reference's fixtures -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_fixture_u_l2_and_loss_match_reference(name):
    rec = load_golden(name)
    assert "u_l2_error_flag" not in rec["case"]["solver"]            # the flag at its default: on
    model = _trained(name)
    plan = _native(model)
    assert model.u_l2_error_flag and plan.ul2_cfg.kind == KIND[name] and (plan.coeffs is not None) == (name in LQ)
    exp = rec["expected"]
    print("%s: u_L2 %s vs %s; loss %s vs %s" % (name, model.u_L2_loss, exp["u_L2_loss"], model.loss_log, exp["loss_log"]))
    assert len(model.u_L2_loss) == len(exp["u_L2_loss"]) == len(model.loss_log) == len(exp["loss_log"]) == model.L
    for l, (got, want) in enumerate(zip(model.u_L2_loss, exp["u_L2_loss"])):
        assert math.isclose(got, want, rel_tol=1e-4), (l, model.u_L2_loss, exp["u_L2_loss"])
    for l, (got, want) in enumerate(zip(model.loss_log, exp["loss_log"])):
        assert math.isclose(got, want, rel_tol=1e-4), (l, model.loss_log, exp["loss_log"])


# ---- 2. per trajectory, against a float64 rollout of the same step ----------------------------------------------------------

def _plan_for(name, net=None, **over):
    case = copy.deepcopy(load_golden(name)["case"])
    if net is not None:
        case["net"] = net
    model = make_pkg_solver(case, dev(), backend="native", L=1, **over)
    plan = pvn.ValueNativePlan(model, noise="reference")
    return model, plan


def _inputs(model, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = model.X_0.detach().cpu().float().reshape(1, -1).repeat(model.K, 1).contiguous()
    xi = torch.randn(model.N, model.K, model.d, generator=g).contiguous()
    return x0, xi


def _direct_log(plan, x0, xi):
    """One psp_genl_rollout_fwd_ul2 call on the plan's buffers (its staged gains included) with supplied x0 and noise."""
    x0, xi = x0.to(dev()), xi.to(dev())
    assert plan.gcfg.base.noise_mode == nat.NOISE_SUPPLIED
    plan.ul2.fill_(float("nan"))
    plan.kcount.zero_()
    nat.check(plan.lib.psp_genl_rollout_fwd_ul2(
        C.byref(plan.gcfg), plan._coeffs_ref(), C.byref(plan.ul2_cfg), nat.ptr(plan.flat), nat.ptr(x0), nat.ptr(plan.t0),
        nat.ptr(xi), 42, 0, nat.ptr(plan.tables), nat.ptr(plan.path), nat.ptr(plan.ahat_buf), nat.ptr(plan.VN), nat.ptr(plan.YN),
        nat.ptr(plan.XN_k), nat.ptr(plan.tN), nat.ptr(plan.kcount), nat.stream_ptr(dev())), "psp_genl_rollout_fwd_ul2")
    torch.cuda.synchronize()
    return plan.ul2.double().cpu()


def _torch_log(model, plan, x0, xi, dtype):
    """The step of solver.py:466-478 on the CPU in ``dtype``: Z = sigma grad_x V(X_n, n), the Euler step, then
    |-Z - u*(X_{n+1}, n dt)|^2 dt with u* from the kernel's description (emulate_u)."""
    spec = model.problem.native_spec()
    d, N, K = model.d, model.N, model.K
    dt, sq = float(model.delta_t.item()), float(model.sq_delta_t.item())            # the fp32 values the kernel is given
    net = copy.deepcopy(model.y_n[0]).cpu().to(dtype)
    cvt = lambda t: None if t is None else torch.as_tensor(t).detach().cpu().to(dtype)
    B = cvt(spec["sigma"][1]) if spec["sigma"][0] == nat.SIGMA_DENSE else float(spec["sigma"][2]) * torch.eye(d, dtype=dtype)
    dkind, dval = spec["drift"][0], cvt(spec["drift"][1])
    X = x0.to(dtype)
    out = torch.zeros(K, dtype=dtype)
    for n in range(N):
        Xg = X.clone().requires_grad_(True)
        V = net(torch.cat([torch.full((K, 1), float(n), dtype=dtype), Xg], 1))
        g, = torch.autograd.grad(V.sum(), Xg)
        Z = g @ B.t()                                               # Z = B grad_x V, row form
        c = -Z if model.adaptive_forward_process else torch.zeros_like(Z)
        if dkind == nat.DRIFT_DENSE:
            b = X @ dval.t()
        elif dkind == nat.DRIFT_DIAG:
            b = dval * X
        elif dkind == nat.DRIFT_DOUBLE_WELL:
            b = -4.0 * dval * X * (X * X - 1.0)
        else:
            b = torch.zeros_like(X)
        X = X + b * dt + (xi[n].to(dtype) * sq + c * dt) @ B.t()
        u = emulate_u(plan.ul2_ref, X, n).to(dtype)
        out = out + ((-Z - u) ** 2).sum(1) * dt
    return out.double()


@pytest.mark.parametrize("name", CASES)
def test_per_trajectory_log_against_float64_rollout(name):
    model, plan = _plan_for(name)
    assert plan.ul2_cfg.kind == KIND[name] and plan.ul2_ref["K_global"] == model.K and plan.ul2_ref["k_offset"] == 0
    x0, xi = _inputs(model, 11)
    got = _direct_log(plan, x0, xi)
    want = _torch_log(model, plan, x0, xi, torch.float64)
    comp = _torch_log(model, plan, x0, xi, torch.float32)
    assert bool(torch.isfinite(got).all()) and float(want.min()) > 0
    floor = 1e-9 * float(want.abs().max())
    dev32 = float(((comp - want).abs() / want.abs()).max())            # the fp32 composite evaluation's own deviation
    devk = float(((got - want).abs() / want.abs()).max())
    print("%s: kernel vs float64 %.2e, fp32 torch vs float64 %.2e (max relative over %d trajectories)" % (name, devk, dev32, model.K))
    tol = max(1e-5, 4.0 * dev32)
    bad = (got - want).abs() > tol * want.abs() + floor
    assert not bool(bad.any()), (tol, got[bad][:4], want[bad][:4])


# ---- 3. the multi-wave instances ---------------------------------------------------------------------------------------------

def _first_iteration_log(name, monkeypatch, nw, **over):
    if nw is None:
        monkeypatch.delenv("PSP_GENL_NW", raising=False)
    else:
        monkeypatch.setenv("PSP_GENL_NW", nw)
    model = _trained(name, L=1, **over)
    plan = _native(model)
    return plan.ul2.double().cpu(), int(plan.sizes.waves_per_tile), model.u_L2_loss[0]


@pytest.mark.parametrize("name", ["lqgc_d17_arch3_value_ul2", "dw_d6_mixed_value_ul2"])
def test_eight_wave_instance_matches_one_wave(name, monkeypatch):
    one, nw1, m1 = _first_iteration_log(name, monkeypatch, None)
    eight, nw8, m8 = _first_iteration_log(name, monkeypatch, "8")
    assert (nw1, nw8) == (1, 8)
    assert float(one.min()) > 0
    assert float(((eight - one).abs() / one.abs()).max()) <= 1e-6, (one[:4], eight[:4])
    assert math.isclose(m1, m8, rel_tol=1e-6)


@pytest.mark.parametrize("name", ["lqgc_d17_arch3_value_ul2", "dw_d6_mixed_value_ul2"])
def test_four_wave_instance_matches_eight_wave(name, monkeypatch):
    """A net of nine hidden blocks never runs on one wave; PSP_GENL_NW=4 gives it the four-wave forward a large batch gets."""
    case = load_golden(name)["case"]

    def run(nw):
        monkeypatch.setenv("PSP_GENL_NW", nw)
        c = dict(copy.deepcopy(case), net=dict(kind="value_densenet", arch=[48, 48, 48], seed=7))
        model = make_pkg_solver(c, dev(), backend="native", L=1)
        model.train()
        plan = _native(model)
        return plan.ul2.double().cpu(), int(plan.sizes.waves_per_tile)

    (eight, nw8), (four, nw4) = run("8"), run("4")
    assert (nw8, nw4) == (8, 4) and float(eight.min()) > 0
    assert float(((four - eight).abs() / eight.abs()).max()) <= 1e-6


# ---- 4. the log is a diagnostic ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["llgc_d8_off_value_ul2", "lqgc_d5_value_ul2"])
def test_log_is_a_diagnostic(name):
    on, off = _trained(name), _trained(name, u_l2_error_flag=False)
    pon, poff = _native(on), _native(off, log=False)
    # the same instance family: the run-time-shaped linear-quadratic kernels, the same waves per tile
    assert pon.coeffs is not None and poff.coeffs is not None
    assert pon.sizes.waves_per_tile == poff.sizes.waves_per_tile and pon.sizes.path_bytes == poff.sizes.path_bytes
    assert on.loss_log == off.loss_log and len(on.loss_log) == on.L
    assert torch.equal(pon.flat, poff.flat)
    assert all(v == 0.0 for v in off.u_L2_loss) and all(v > 0.0 for v in on.u_L2_loss)


# ---- 5. native against composite ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in CASES if KIND[n] != nat.UL2_GRID])
def test_native_log_matches_composite(name):
    nat_m = _trained(name, noise="reference")
    _native(nat_m)
    cmp_m = make_pkg_solver(copy.deepcopy(load_golden(name)["case"]), dev(), backend="torch", noise="reference")
    cmp_m.train()
    assert cmp_m.plan_name == "torch" and all(v > 0 for v in cmp_m.u_L2_loss)
    print("%s: native %s composite %s" % (name, nat_m.u_L2_loss, cmp_m.u_L2_loss))
    for l, (a, b) in enumerate(zip(nat_m.u_L2_loss, cmp_m.u_L2_loss)):
        assert math.isclose(a, b, rel_tol=1e-5), (l, nat_m.u_L2_loss, cmp_m.u_L2_loss)


# ---- 6. a NULL struct is the existing entry point ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lqgc_d5_value_ul2", "dw_d6_mixed_value_ul2"])
def test_null_struct_is_the_existing_entry_point(name):
    # (a three-layer value net: with the flag off the default [30, 30] net of the double well runs on the templated kernels)
    model, plan = _plan_for(name, net=dict(kind="value_densenet", arch=[20, 16, 12], seed=7), u_l2_error_flag=False)
    assert plan.ul2_cfg is None and plan.deep is not None and (plan.coeffs is not None) == (name in LQ)
    x0, xi = (t.to(dev()) for t in _inputs(model, 12))

    def run(ul2_entry):
        for t in (plan.path, plan.ahat_buf, plan.YN, plan.XN_k, plan.VN):
            t.fill_(float("nan"))
        plan.kcount.zero_()
        tail = (nat.ptr(plan.flat), nat.ptr(x0), nat.ptr(plan.t0), nat.ptr(xi), 42, 0, nat.ptr(plan.tables), nat.ptr(plan.path),
                nat.ptr(plan.ahat_buf), nat.ptr(plan.VN), nat.ptr(plan.YN), nat.ptr(plan.XN_k), nat.ptr(plan.tN),
                nat.ptr(plan.kcount), nat.stream_ptr(dev()))
        if ul2_entry:
            nat.check(plan.lib.psp_genl_rollout_fwd_ul2(C.byref(plan.gcfg), plan._coeffs_ref(), None, *tail), "fwd_ul2")
        else:
            nat.check(plan.lib.psp_genl_rollout_fwd_lq(C.byref(plan.gcfg), plan._coeffs_ref(), *tail), "fwd_lq")
        torch.cuda.synchronize()
        return [t.clone() for t in (plan.YN, plan.XN_k, plan.path, plan.VN, plan.ahat_buf)]

    want, got = run(False), run(True)
    assert bool(torch.isfinite(want[0]).all()) and float(want[1].abs().max()) > 0
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ---- the constructor call of the issue ---------------------------------------------------------------------------------------

def test_default_flag_plans_native():
    lq = psp.LQGC(d=20, off_diag=0.1, T=0.2, delta_t=0.005, device=dev())
    m = psp.Solver("x", lq, approx_method="value_function", time_approx="inner", detach_forward=True, K=256, L=2, delta_t=0.01,
                   device=dev(), verbose=False)
    m.train()
    assert m.plan_name == "native" and m.u_l2_error_flag, m.plan_reason
    _native(m)
    assert len(m.u_L2_loss) == 2 and all(math.isfinite(v) and v > 0 for v in m.u_L2_loss)
