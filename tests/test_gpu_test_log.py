"""The device-side K_test_log diagnostic on the GPU (psp_genl_test_error, csrc/genl_eval_kernels.h): V against a float64
forward of the same net on supplied points, the sampled points against the numpy mirror of the sampler
(tests/sampler_mirror.py), v_true and the reduced statistics against float64 recomputations from the per-point dumps, and
the solvers' ``test_log='device'``.

Measured on an MI355X (the maxima the tests print):
  V, supplied points          max |V_dev - V_64| / max(1, |V_64|) = 3.0e-6 ([110, 110, 50] at d_in = 101)       (bound 1e-4)
  sampled points              max |x_dev - x_64| / R = 8.6e-7, max |t_dev - t_64| / T = 7.0e-8                   (bounds 1e-4, 1e-6)
  v_true                      max relative error 4.6e-7 (committor d = 3; 8.0e-8 at d = 10, exp 1.4e-7, quad 1.1e-7)   (bound 2e-5)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sampler_mirror as sm
from util_cases import psp

pytestmark = pytest.mark.gpu
nat = psp.native
HI_SEED = (0xDEADBEEF << 32) | 77


def dev():
    return torch.device("cuda:0")


def _blocks(n):
    return (n + 15) // 16


def _net(kind, d_in, arch, seed=3):
    """A value net with non-zero biases (the classes draw zero ones)."""
    if kind == "linear":
        net = psp.DenseNet_tanh(d_in=d_in, d_out=1, lr=1e-3, arch=arch, seed=seed)
    else:
        net = psp.DenseNet(d_in=d_in, d_out=1, lr=1e-3, arch=arch, seed=seed, activation=kind)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return net.to(dev())


def _spec(net, d_in):
    from path_space_pde_solver_amd.plan_general_deep import value_net_spec
    spec = value_net_spec(net, d_in)
    assert not isinstance(spec, str), spec
    return spec


def forward64(spec, x):
    """The dense-concat forward of the net in float64 on the CPU."""
    params = [p.detach().double().cpu() for p in spec["params"]]
    x = x.double().cpu()
    n = len(params) // 2
    for i in range(n):
        W = params[2 * i].t() if spec["linear"] else params[2 * i]
        z = x @ W + params[2 * i + 1]
        if i == n - 1:
            return z[:, 0].numpy()
        h = torch.relu(z) ** 2 if spec["act"] == "relu2" else (torch.tanh(z) ** 2 if spec["act"] == "tanh2" else torch.tanh(z))
        x = torch.cat([x, h], 1)


def _config(spec, d, has_time, K, kind, a=0.0, b=1.0, T=1.0, vt=nat.VTRUE_QUAD, par=(0.0, 0.0, 0.0, 0.0), slots=4, k_offset=0):
    c = nat.GenlEvalConfig()
    dims = spec["dims"]
    c.d, c.has_time, c.n_hidden = d, 1 if has_time else 0, len(dims) - 2
    for i, w in enumerate(dims[1:-1]):
        c.widths[i] = w
    c.activation = {"relu2": nat.ACT_RELU2, "tanh2": nat.ACT_TANH2, "tanh": nat.ACT_TANH}[spec["act"]]
    c.linear_layout = 1 if spec["linear"] else 0
    c.K_points, c.k_offset, c.sample_kind, c.bound_a, c.bound_b, c.T = K, k_offset, kind, a, b, T
    c.vtrue_kind = vt
    for i, v in enumerate(par):
        c.vtrue_par[i] = v
    c.log_slots = slots
    return c


def call(cfg, spec, x=None, t=None, seed=42, it=0, slot=0, slot_dev=None, log=None):
    """One psp_genl_test_error call with every dump; returns (sizes, dict of host arrays, the log tensor)."""
    lib = nat.load()
    sz = nat.GenlEvalSizes()
    nat.check(lib.psp_genl_eval_query(C.byref(cfg), C.byref(sz)), "psp_genl_eval_query")
    d0, K, d = dev(), cfg.K_points, cfg.d
    flat = torch.cat([p.detach().reshape(-1).float() for p in spec["params"]]).contiguous()
    assert flat.numel() == sz.n_params
    tables = torch.empty(sz.table_bytes // 4, dtype=torch.float32, device=d0)
    partial = torch.full((sz.partial_bytes // 8,), float("nan"), dtype=torch.float64, device=d0)
    if log is None:
        log = torch.full((cfg.log_slots, 4), -7.0, dtype=torch.float64, device=d0)
    nan32 = dict(dtype=torch.float32, device=d0)
    out = dict(x=torch.full((K, d), float("nan"), **nan32), t=torch.full((K,), float("nan"), **nan32),
               v=torch.full((K,), float("nan"), **nan32), v_true=torch.full((K,), float("nan"), **nan32),
               keep=torch.full((K,), -1, dtype=torch.int32, device=d0))
    nat.check(lib.psp_genl_test_error(C.byref(cfg), nat.ptr(flat), nat.ptr(x), nat.ptr(t), seed, it, nat.ptr(tables), nat.ptr(partial),
                                      nat.ptr(log), slot, nat.ptr(slot_dev), nat.ptr(out["x"]), nat.ptr(out["t"]), nat.ptr(out["v"]),
                                      nat.ptr(out["v_true"]), nat.ptr(out["keep"]), nat.stream_ptr(d0)), "psp_genl_test_error")
    torch.cuda.synchronize()
    return sz, {k: v.cpu().numpy() for k, v in out.items()}, log


# ---- 1. V on supplied points --------------------------------------------------------------------------------------------
# (kind, d_in, arch, time input, K): every activation, both weight layouts, with and without a time input, the input widths
# 1, 16, 17, 101, 112, the hidden shapes of the issue, K = 1, 16, 37
V_CASES = [("relu2", 1, [13], False, 1), ("tanh2", 16, [64, 64], True, 16), ("linear", 17, [30, 30, 30, 30], False, 37),
           ("relu2", 101, [110, 110, 50], True, 37), ("tanh", 112, [128, 1], False, 16), ("linear", 17, [13], True, 1),
           ("relu2", 112, [30, 30, 30, 30], True, 37), ("tanh2", 1, [128, 1], False, 37), ("linear", 16, [110, 110, 50], False, 16),
           ("tanh", 101, [64, 64], True, 37), ("relu2", 17, [64, 64], False, 16)]
_measured = {}


def _small(case):
    """One wave per tile holds at most 8 hidden and 16 concatenation blocks (make_genl_plan)."""
    hb = sum(_blocks(h) for h in case[2])
    return hb <= 8 and _blocks(case[1]) + hb <= 16


V_RUNS = [(c, nw) for c in V_CASES for nw in ("1", "8") if nw == "8" or _small(c)]       # both waves-per-tile instances


@pytest.mark.parametrize("case,nw", V_RUNS, ids=["%s-%d-%s-%s-K%d-NW%s" % (c[0], c[1], "x".join(map(str, c[2])), "t" if c[3] else "x", c[4], nw)
                                                 for c, nw in V_RUNS])
def test_value_matches_float64_forward(case, nw, monkeypatch):
    kind, d_in, arch, has_time, K = case
    monkeypatch.setenv("PSP_GENL_NW", nw)
    net = _net(kind, d_in, arch)
    spec = _spec(net, d_in)
    d = d_in - (1 if has_time else 0)
    g = torch.Generator().manual_seed(K + d_in)
    pts = torch.rand(K, d_in, generator=g) * 2 - 1
    x = pts[:, :d].contiguous().to(dev())
    t = pts[:, d].contiguous().to(dev()) if has_time else None
    sz, out, _ = call(_config(spec, d, has_time, K, nat.TSAMPLE_SUPPLIED), spec, x=x, t=t)
    assert sz.waves_per_tile == int(nw)
    v64 = forward64(spec, pts)
    err = np.max(np.abs(out["v"] - v64) / np.maximum(1.0, np.abs(v64)))
    _measured["V"] = max(_measured.get("V", 0.0), float(err))
    print("V %s NW=%s: max |V_dev - V_64| / max(1, |V_64|) = %.2e (running max %.2e)" % (case, nw, err, _measured["V"]))
    assert np.array_equal(out["x"], x.cpu().numpy()) and out["keep"].all()
    assert np.all(np.abs(out["v"] - v64) <= 1e-4 * np.maximum(1.0, np.abs(v64)))


# ---- 2. sampled points against the mirror -----------------------------------------------------------------------------
S_CASES = [(sm.BALL, 3, 37, 0.0, 1.5), (sm.BALL, 3, 1000, 0.0, 1.5), (sm.BALL, 20, 37, 0.0, 1.0), (sm.BALL, 20, 1000, 0.0, 1.0),
           (sm.BALL, 100, 37, 0.0, 2.0), (sm.BALL, 100, 1000, 0.0, 2.0), (sm.BOX, 5, 37, -2.0, 1.0), (sm.BOX, 5, 1000, -2.0, 1.0),
           (sm.ANNULUS, 4, 37, 1.0, 2.0), (sm.ANNULUS, 4, 1000, 1.0, 2.0)]


@pytest.mark.parametrize("case", S_CASES, ids=lambda c: "%s-d%d-K%d" % ({1: "ball", 2: "annulus", 3: "box"}[c[0]], c[1], c[2]))
def test_sampled_points_match_the_mirror(case):
    kind, d, K, a, b = case
    T, k_offset, it = 0.75, 12345, 9
    net = _net("relu2", d + 1, [13])
    spec = _spec(net, d + 1)
    cfg = _config(spec, d, True, K, kind, a, b, T=T, k_offset=k_offset)
    sz, out, log = call(cfg, spec, seed=HI_SEED, it=it, slot=1)
    ref = sm.sample(kind, d, K, a, b, T=T, seed=HI_SEED, iteration=it, k_offset=k_offset)
    R = (b - a) if kind == sm.BOX else b
    ok = np.ones(K, dtype=bool) if kind == sm.BOX else ref["gnorm"] >= 0.1
    assert np.mean(~ok) <= 0.01                                  # at d >= 3 a draw with |g| < 0.1 is rare
    ex = np.max(np.abs(out["x"][ok] - ref["x"][ok])) / R
    et = np.max(np.abs(out["t"] - ref["t"])) / T
    print("sampler %s: max |x_dev - x_64| / R = %.2e, max |t_dev - t_64| / T = %.2e" % (case, ex, et))
    assert ex <= 1e-4 and et <= 1e-6
    near = np.abs(ref["radius"] - a) <= 1e-4 if kind == sm.ANNULUS else np.zeros(K, dtype=bool)
    assert np.mean(near) <= 0.01
    assert np.array_equal(out["keep"][~near] != 0, ref["keep"][~near])
    rows = log.cpu().numpy()
    assert rows[1, 3] == out["keep"].sum() and np.all(rows[[0, 2, 3]] == -7.0)
    if kind == sm.ANNULUS:
        assert 0 < out["keep"].sum() < K or K < 100
    # the net saw the dumped points
    v64 = forward64(spec, torch.cat([torch.from_numpy(out["x"]), torch.from_numpy(out["t"])[:, None]], 1))
    assert np.all(np.abs(out["v"] - v64) <= 1e-4 * np.maximum(1.0, np.abs(v64)))


# ---- 3. v_true and the statistics -------------------------------------------------------------------------------------
T_CASES = [("exp", 5, sm.BALL, 0.0, 1.0, nat.VTRUE_EXP, (1.0, 1.0, 0.0, 0.0), True),
           ("exp_elliptic", 20, sm.BALL, 0.0, 1.0, nat.VTRUE_EXP, (0.7, 0.0, 0.0, 0.0), False),
           ("quad", 6, sm.BOX, -1.0, 1.0, nat.VTRUE_QUAD, (12.0, 1.0, 0.0, 0.0), True),
           ("committor3", 3, sm.ANNULUS, 1.0, 2.0, nat.VTRUE_COMMITTOR, (1.0, 2.0, 3.0, 0.0), False),
           ("committor10", 10, sm.ANNULUS, 1.0, 2.0, nat.VTRUE_COMMITTOR, (1.0, 2.0, 10.0, 0.0), False)]


@pytest.mark.parametrize("case", T_CASES, ids=lambda c: c[0])
def test_v_true_and_statistics(case):
    name, d, kind, a, b, vt, par, has_time = case
    K = 1000
    d_in = d + (1 if has_time else 0)
    net = _net("tanh2", d_in, [30, 30])
    spec = _spec(net, d_in)
    cfg = _config(spec, d, has_time, K, kind, a, b, T=1.0, vt=vt, par=par)
    sz, out, log = call(cfg, spec, seed=5, it=3, slot=0)
    want = sm.v_true(vt, par, out["x"], out["t"] if has_time else None)
    rel = np.max(np.abs(out["v_true"] - want) / np.abs(want))
    print("v_true %s: max relative error %.2e" % (name, rel))
    assert rel <= 2e-5
    keep = out["keep"] != 0
    e = out["v_true"].astype(np.float64)[keep] - out["v"].astype(np.float64)[keep]
    sums = np.array([np.sum(e ** 2), np.sum(np.abs(e)), np.sum(np.abs(e) / out["v_true"].astype(np.float64)[keep]), keep.sum()])
    rows = log.cpu().numpy()
    assert np.all(np.abs(rows[0] - sums) <= 1e-12 * np.abs(sums)), (rows[0], sums)
    assert np.all(rows[1:] == -7.0)
    # a second identical call: bit-identical
    _, out2, log2 = call(cfg, spec, seed=5, it=3, slot=0)
    assert torch.equal(log, log2) and all(np.array_equal(out[k], out2[k], equal_nan=True) for k in out)
    # the slot from a device integer
    slot_dev = torch.tensor([2], dtype=torch.int32, device=dev())
    _, _, log3 = call(cfg, spec, seed=5, it=3, slot=0, slot_dev=slot_dev)
    rows3 = log3.cpu().numpy()
    assert np.array_equal(rows3[2], rows[0]) and np.all(rows3[[0, 1, 3]] == -7.0)
    # a device slot outside the log is dropped
    slot_dev.fill_(4)
    _, _, log4 = call(cfg, spec, seed=5, it=3, slot=0, slot_dev=slot_dev)
    assert np.all(log4.cpu().numpy() == -7.0)


# ---- 4. the solvers ---------------------------------------------------------------------------------------------------
def _solver(which, **kw):
    common = dict(K=64, N=5, L=3, noise="philox", backend="native", device=dev(), verbose=False, seed=42)
    common.update(kw)
    if which == "parabolic":
        pb = psp.ExponentialOnSphereNonlinearParabolic(d=4, device=dev())
        return pb, psp.GeneralSolver(pb, "test log", **common)
    pb = psp.ExponentialOnBallNonlinear(d=5, device=dev())
    model = psp.EllipticSolver(pb, "test log", **common)
    if which == "deep":
        model.V = psp.DenseNet(d_in=5, d_out=1, lr=1e-3, arch=[30, 30, 30], seed=42).to(dev())
    return pb, model


@pytest.mark.parametrize("which", ["elliptic", "deep", "parabolic"])
def test_solver_device_log(which):
    from path_space_pde_solver_amd.utilities import compute_test_error_native
    modus = "parabolic" if which == "parabolic" else "elliptic"
    pb, model = _solver(which, K_test_log=512, test_log="device")
    plan = model._choose_plan()
    assert type(plan).__name__ == ("GeneralDeepPlan" if which == "deep" else "GeneralNativePlan")
    step, seen = plan.iteration, []

    def watched(l):                                             # nothing of the log reaches the host between iterations
        out = step(l)
        seen.append(len(model.V_test_L2) + len(model.V_test_abs) + len(model.V_test_rel_abs))
        return out
    plan.iteration = watched
    model.train()
    assert model.plan_name == "native" and model._gen_plan is plan and seen == [0, 0, 0]
    assert len(model.V_test_L2) == len(model.V_test_abs) == len(model.V_test_rel_abs) == 3
    l2, mae, mre, pts = compute_test_error_native(model, pb, 512, modus, seed=model.seed, iteration=2, return_points=True)
    assert (model.V_test_L2[-1], model.V_test_abs[-1], model.V_test_rel_abs[-1]) == (l2, mae, mre)
    assert compute_test_error_native(model, pb, 512, modus, iteration=2) == (l2, mae, mre)
    # float64 evaluation on the returned points, within the per-point bounds of the tests above
    x, t = pts["x"].double().cpu(), pts["t"].double().cpu()
    spec = _spec(model.V, pb.d + (1 if modus == "parabolic" else 0))
    v64 = forward64(spec, torch.cat([x, t[:, None]], 1) if modus == "parabolic" else x)
    vt64 = (pb.v_true(x, t) if modus == "parabolic" else pb.v_true(x)).numpy()
    assert pts["keep"].all()
    dv = 1e-4 * np.maximum(1.0, np.abs(v64)) + 2e-5 * np.abs(vt64)          # bound on |e_dev - e_64| per point
    e = vt64 - v64
    assert abs(mae - np.mean(np.abs(e))) <= np.mean(dv)
    assert abs(l2 - np.mean(e ** 2)) <= np.mean(2 * np.abs(e) * dv + dv ** 2)
    assert abs(mre - np.mean(np.abs(e) / vt64)) <= np.mean(dv / vt64 + (np.abs(e) + dv) / vt64 * 4e-5)
    assert np.isfinite([l2, mae, mre]).all() and l2 > 0
    # the device log consumes no training randomness
    _, plain = _solver(which, K_test_log=None)
    plain.train()
    assert plain.V_test_L2 == [] and plain.loss_log == model.loss_log
    for p, q in zip(model.V.parameters(), plain.V.parameters()):
        assert torch.equal(p, q)
