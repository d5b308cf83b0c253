"""The device-side K_test_log diagnostic (csrc/genl_eval_kernels.h, device_test_log.py), host side: argument handling of
psp_genl_eval_query, the struct layouts, the numpy mirror of the point sampler (tests/sampler_mirror.py) against the domains'
distributions, the problems' native_vtrue_spec() against their v_true, and the ``test_log`` keyword.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import sampler_mirror as sm
from util_cases import psp

nat = psp.native


def _cfg(d=5, widths=(30, 30), has_time=0, K=100, kind=nat.TSAMPLE_BALL, a=0.0, b=1.0, vt=nat.VTRUE_EXP, slots=3):
    c = nat.GenlEvalConfig()
    c.d, c.has_time, c.n_hidden = d, has_time, len(widths)
    for i, w in enumerate(widths[:4]):
        c.widths[i] = w
    c.activation = nat.ACT_RELU2
    c.K_points, c.sample_kind, c.bound_a, c.bound_b, c.T = K, kind, a, b, 1.0
    c.vtrue_kind = vt
    c.vtrue_par[0] = 1.0
    c.log_slots = slots
    return c


def _query(c):
    sizes = nat.GenlEvalSizes()
    lib = nat.load()
    rc = lib.psp_genl_eval_query(C.byref(c), C.byref(sizes))
    return rc, sizes, (lib.psp_last_error().decode() if rc else "")


def test_struct_sizes_match_the_library():
    out = (C.c_int32 * 2)()
    assert nat.load().psp_abi_struct_sizes4(C.byref(out)) == 0
    assert list(out) == [C.sizeof(nat.GenlEvalConfig), C.sizeof(nat.GenlEvalSizes)]


def _blocks(n):
    return (n + 15) // 16


@pytest.mark.parametrize("d,has_time,widths,K", [(5, 0, (30, 30), 100), (100, 1, (110, 110, 50), 10000), (112, 0, (128, 1), 1),
                                                 (1, 0, (13,), 37), (20, 0, (30, 30, 30, 30), 10000)])
def test_query_sizes_are_consistent(d, has_time, widths, K):
    rc, sz, msg = _query(_cfg(d=d, has_time=has_time, widths=widths, K=K))
    assert rc == 0, msg
    d_in = d + has_time
    hb = sum(_blocks(w) for w in widths)
    tb = _blocks(d_in) + hb
    fan, n_params = d_in, 0
    for w in widths:
        n_params += fan * w + w
        fan += w
    n_params += fan + 1
    assert sz.n_params == n_params
    assert sz.workgroups == _blocks(K) and sz.partial_bytes == 4 * 8 * sz.workgroups
    assert sz.lds_bytes == 1024 * tb                         # the activation image alone: half the rollout's request
    assert sz.waves_per_tile in (1, 8)
    if hb > 8 or tb > 16:
        assert sz.waves_per_tile == 8                        # one wave per tile only for the nets its register slots hold
    if hb <= 5 and tb <= 16:
        assert sz.waves_per_tile == 1
    # the tables: forward and reverse operand of every layer, its staged bias, the output vector
    floats, blocks = 0, _blocks(d_in)
    for w in widths:
        floats += 2 * _blocks(w) * 4 * blocks * 64 + 16 * _blocks(w)
        blocks += _blocks(w)
    floats += 16 * blocks
    assert sz.table_bytes == 4 * floats


@pytest.mark.parametrize("kw,code", [
    (dict(widths=(129, 30)), -2), (dict(widths=(30, 30, 30, 30, 30)), -2), (dict(d=113), -2), (dict(d=112, has_time=1), -2),
    (dict(kind=nat.TSAMPLE_BOX, a=1.0, b=1.0), -1), (dict(kind=nat.TSAMPLE_BOX, a=2.0, b=1.0), -1),
    (dict(kind=nat.TSAMPLE_ANNULUS, a=2.0, b=2.0), -1), (dict(kind=nat.TSAMPLE_ANNULUS, a=3.0, b=2.0), -1),
    (dict(kind=nat.TSAMPLE_BALL, b=0.0), -1), (dict(kind=4), -1), (dict(kind=-1), -1), (dict(vt=3), -1), (dict(vt=-1), -1),
    (dict(K=0), -1), (dict(K=-5), -1), (dict(slots=0), -1), (dict(widths=(0,)), -2)])
def test_query_rejects(kw, code):
    rc, _, msg = _query(_cfg(**kw))
    assert rc == code and msg, (kw, rc, msg)


def test_query_accepts_every_kind():
    for kind, a, b in ((nat.TSAMPLE_SUPPLIED, 0.0, 0.0), (nat.TSAMPLE_BALL, 0.0, 2.0), (nat.TSAMPLE_ANNULUS, 1.0, 2.0),
                       (nat.TSAMPLE_BOX, -1.0, 1.0)):
        for vt in (nat.VTRUE_EXP, nat.VTRUE_QUAD, nat.VTRUE_COMMITTOR):
            rc, _, msg = _query(_cfg(kind=kind, a=a, b=b, vt=vt))
            assert rc == 0, (kind, vt, msg)


# ---- the sampler's mirror ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 20])
def test_mirror_ball_is_uniform_in_the_ball(d):
    R = 1.5
    s = sm.sample(sm.BALL, d, 20000, 0.0, R, seed=7)
    assert s["radius"].max() < R and s["keep"].all()
    assert abs(np.mean(s["radius"] ** 2) / R ** 2 - d / (d + 2.0)) < 0.02
    assert np.all((s["t"] > 0) & (s["t"] < 1.0)) and abs(np.mean(s["t"]) - 0.5) < 0.01
    assert np.abs(np.mean(s["x"], 0)).max() < 0.03 * R       # no direction is preferred


def test_mirror_box_is_uniform():
    lo, hi = -2.0, 1.0
    s = sm.sample(sm.BOX, 5, 20000, lo, hi, seed=3)
    assert s["x"].min() > lo and s["x"].max() < hi
    assert np.abs(np.mean(s["x"], 0) - 0.5 * (lo + hi)).max() < 0.01 * (hi - lo)
    assert np.abs(np.var(s["x"], 0) - (hi - lo) ** 2 / 12).max() < 0.02 * (hi - lo) ** 2


def test_mirror_annulus_keeps_the_outer_shell():
    d, r1, r2 = 4, 1.0, 2.0
    s = sm.sample(sm.ANNULUS, d, 20000, r1, r2, seed=11)
    assert s["radius"].max() < r2
    assert np.all(s["radius"][s["keep"]] > r1) and np.all(s["radius"][~s["keep"]] <= r1)
    assert abs(np.mean(s["keep"]) - (1 - (r1 / r2) ** d)) < 0.02


def test_mirror_streams_depend_on_every_counter_word():
    base = sm.sample(sm.BALL, 3, 64, 0.0, 1.0, seed=42, iteration=0)["x"]
    assert not np.allclose(base, sm.sample(sm.BALL, 3, 64, 0.0, 1.0, seed=42, iteration=1)["x"])
    assert not np.allclose(base, sm.sample(sm.BALL, 3, 64, 0.0, 1.0, seed=42 + (1 << 32), iteration=0)["x"])
    shifted = sm.sample(sm.BALL, 3, 64, 0.0, 1.0, seed=42, iteration=0, k_offset=5)["x"]
    assert np.array_equal(shifted[:59], base[5:])            # the global point index is the counter


# ---- native_vtrue_spec ------------------------------------------------------------------------------------------------
def _problems():
    dev = "cpu"
    return [psp.ExponentialOnSphere(d=4, alpha=0.7, device=dev), psp.ExponentialOnBallNonlinear(d=5, device=dev),
            psp.ExponentialOnBallNonlinearSin(d=3, alpha=1.3, device=dev), psp.ExponentialOnBallNonlinearSinHessian(d=6, device=dev),
            psp.ExponentialOnSphereNonlinearParabolic(d=4, T=0.8, alpha=0.9, device=dev), psp.HeatEquation(d=7, T=1.5, device=dev),
            psp.problems.QuadraticOnBox(d=3, device=dev), psp.problems.QuadraticOnBox(d=3, parabolic=False, device=dev),
            psp.problems.Committor(d=3, device=dev), psp.problems.Committor(d=10, device=dev)]


@pytest.mark.parametrize("i", range(10))
def test_vtrue_spec_reproduces_v_true(i):
    pb = _problems()[i]
    spec = pb.native_vtrue_spec()
    g = torch.Generator().manual_seed(5 + i)
    x = torch.randn(200, pb.d, generator=g, dtype=torch.float64)
    x = x / x.norm(dim=1, keepdim=True) * (1.05 + 0.9 * torch.rand(200, 1, generator=g, dtype=torch.float64))   # 1.05 <= |x| < 1.95
    t = torch.rand(200, generator=g, dtype=torch.float64) * float(getattr(pb, "T", 1.0))
    timed = isinstance(pb, (psp.ExponentialOnSphereNonlinearParabolic, psp.HeatEquation))
    want = (pb.v_true(x, t) if timed else pb.v_true(x)).double().numpy()
    got = sm.v_true(spec["kind"], spec["par"], x.numpy(), t.numpy() if timed else None)
    assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-12


def test_tabulated_problems_have_no_spec():
    for cls in (psp.DoubleWell, psp.DoubleWell_multidim, psp.problems.DoubleWell_multidim_for_general_solver, psp.AllenCahn):
        assert not hasattr(cls, "native_vtrue_spec")


# ---- the keyword ------------------------------------------------------------------------------------------------------
def test_bogus_test_log_is_rejected_at_construction():
    pb = psp.ExponentialOnBallNonlinear(d=3, device="cpu")
    with pytest.raises(ValueError, match="test_log"):
        psp.EllipticSolver(pb, "x", K=8, N=2, L=1, K_test_log=16, test_log="bogus", device="cpu")
    with pytest.raises(ValueError, match="test_log"):
        psp.GeneralSolver(psp.HeatEquation(d=2, device="cpu"), "x", K=8, N=2, L=1, test_log="bogus", device="cpu")
    assert psp.EllipticSolver(pb, "x", K=8, N=2, L=1, device="cpu").test_log == "reference"


def test_device_log_without_a_spec_raises_at_train():
    pb = psp.problems.DoubleWell_multidim_for_general_solver(d=2, device="cpu")
    model = psp.GeneralSolver(pb, "x", K=8, N=2, L=1, K_test_log=16, test_log="device", device="cpu", verbose=False)
    with pytest.raises(ValueError, match="native_vtrue_spec"):
        model.train()
    assert model.V_test_L2 == [] and model.loss_log == []


def test_device_log_with_a_replaced_v_true_raises_at_train():
    pb = psp.ExponentialOnBallNonlinear(d=3, device="cpu")
    pb.v_true = lambda x: torch.ones(x.shape[0])
    model = psp.EllipticSolver(pb, "x", K=8, N=2, L=1, K_test_log=16, test_log="device", device="cpu", verbose=False)
    with pytest.raises(ValueError, match="v_true"):
        model.train()


def test_native_entry_names_what_it_does_not_cover():
    from path_space_pde_solver_amd.utilities import compute_test_error_native
    pb = psp.ExponentialOnBallNonlinear(d=3, device="cpu")
    model = psp.EllipticSolver(pb, "x", K=8, N=2, L=1, device="cpu", verbose=False)
    pb.boundary = "square-corner"
    with pytest.raises(NotImplementedError, match="square-corner"):
        compute_test_error_native(model, pb, 16, "elliptic")
    pb.boundary = "sphere"
    model.V = psp.DenseNet(d_in=3, d_out=1, lr=1e-3, arch=[30, 30, 30, 30, 30])
    with pytest.raises(NotImplementedError, match="hidden layers"):
        compute_test_error_native(model, pb, 16, "elliptic")
    model.V = psp.MySequential(3, 1, 1e-3, seed=1)
    with pytest.raises(NotImplementedError, match="dense-concat"):
        compute_test_error_native(model, pb, 16, "elliptic")
    dw = psp.problems.DoubleWell_multidim_for_general_solver(d=2, device="cpu")
    with pytest.raises(NotImplementedError, match="native_vtrue_spec"):
        compute_test_error_native(model, dw, 16, "parabolic")


def test_default_keeps_the_host_log_on_the_composite_plan():
    pb = psp.ExponentialOnBallNonlinear(d=3, device="cpu")
    logs = []
    for kw in (dict(), dict(test_log="device")):                 # the composite plan keeps the host log whatever the keyword says
        model = psp.EllipticSolver(pb, "x", K=8, N=2, L=2, K_test_log=16, device="cpu", verbose=False, **kw)
        model.train()
        assert model.plan_name == "torch" and len(model.V_test_L2) == 2
        logs.append((model.loss_log, model.V_test_L2, model.V_test_abs, model.V_test_rel_abs))
    assert logs[0] == logs[1]
