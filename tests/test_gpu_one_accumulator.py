"""The one-accumulator split products of the narrow forward (csrc/hjb_kernels.h: split_tab, gemm_Tx ONE; hjb_fwd_kernel MODE 2):
both operands of a product carry a power of two, the three f16 products of an fp32 product share one accumulator, and the factor
2048 leaves where a multiplication stands anyway.  The backward (hjb_bwd3_kernel) keeps its two chains -- the one-accumulator form
was measured slower there (profiles/one_accumulator_ab.json).

Forward: the split kernel against its fp32-MFMA twin on the same inputs and against a float64 evaluation of the same rollout (the
kernel's own fp32 numbers cast to double: parameters, coefficients, x_0 and the increments read back from the path store), N = 4,
K = 40 (three tiles, a ragged last one), one shape per tail kind of SplitGeo -- (100, 64) full steps plus the exact fp32 step (in
the sigma basis, the headline's instance, and in the x basis, where the B v product runs too), (40, 32) and (7, 16) the 16x16x16 tail
(behind a full step / alone in one padded block), (64, 32) no tail.  The error against float64 is held to 1.5 x what the
two-chain kernels of the parent commit give on the same case (PARENT below, measured with this file on that build; the margin is
for the two extra roundings per k-step in the shared accumulator); the distance to the twin to the sum of the two errors a pair of
fp32-grade kernels may have, 1.5 x PARENT + the twin's own.  The same with states and weights scaled by 2^-10: lo parts below the
f16 normal range, where a bad division of the 11 bits between the operands shows.

Backward: unchanged native code, run on the store the NEW forward writes -- hjb_bwd3_kernel against hjb_bwd2_kernel as
tests/test_gpu_narrow_exchange.py runs them (its shapes, its bound, its ragged K), both store_path instances, per workgroup (the
per-row bound of tests/test_gpu_range_guard.py) and in total; the two instances bit-equal to each other and three runs bit-equal.

Range: the thresholds of the scaled operands (include/psp.h: range_flag) -- a state entry beyond f16 altogether (7e4) and one
between the new input threshold and the old one (3000 > 65504 / 32) send the guarded iteration to the fp32 twin; half the new
threshold stays on the split kernels.
"""
import math

import pytest
import torch

from test_gpu_narrow_exchange import N_STEPS, SHAPES, ragged_K
from test_gpu_range_guard import _bwd, nat
from util_cases import assert_blocks, flat_params, psp

pytestmark = pytest.mark.gpu
F64 = torch.float64
N_FWD, K_FWD = 4, 40
MARGIN = 1.5

# max |kernel - float64| of the parent commit's hjb_fwd_kernel<.., MODE 2> on these cases: (D, X, h1, h2)
PARENT = {
    "d100-H64-sigma": (3.008e-06, 5.964e-07, 1.427e-07, 1.344e-07),
    "d100-H64-x": (6.194e-06, 8.365e-07, 1.645e-07, 1.303e-07),
    "d40-H32-x": (1.555e-06, 5.334e-07, 1.324e-07, 1.241e-07),
    "d64-H32-x": (2.832e-06, 5.408e-07, 1.415e-07, 1.300e-07),
    "d7-H16-x": (5.079e-07, 3.088e-07, 1.342e-07, 1.233e-07),
    "d40-H32-x-small": (5.780e-07, 2.206e-07, 8.959e-08, 8.619e-08),
}
FWD_CASES = [(100, 64, "sigma", (100, 64)), (100, 64, "x", (100, 64)), (40, 32, "x", (48, 32)), (64, 32, "x", (64, 32)),
             (7, 16, "x", (16, 16))]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def tile_per_wave_forward(monkeypatch):
    """K = 40 is small enough for the library's small-K forwards; pin both modes to hjb_fwd_kernel (tests/test_gpu_range_guard.py)."""
    monkeypatch.setenv("PSP_FWD_VARIANT", "1")
    monkeypatch.delenv("PSP_STATE_BASIS", raising=False)


def _solver(d, H, mlp, basis="x", K=K_FWD, N=N_FWD, small=False, x0="spread", path_noise="store", loss="log-variance", **kw):
    prob = psp.LLGC(d=d, off_diag=0.1 / d ** 0.5, T=(N + 0.5) * 0.01, seed=42, device=dev())
    if x0 is not None:                                   # (None: the problem's own X_0)
        prob.X_0 = (torch.linspace(-1.0, 1.0, d) if isinstance(x0, str) else x0).to(dev())
    if small:
        prob.X_0 = prob.X_0 * 2.0 ** -10
    m = psp.Solver("one", prob, lr=1e-3, L=1, K=K, delta_t=0.01, loss_method=loss, time_approx="inner",
                   adaptive_forward_process=True, detach_forward=True, u_l2_error_flag=False, verbose=False, seed=42, device=dev(),
                   backend="native", noise="philox", widths=(H, H), mlp_dtype=mlp, path_noise=path_noise, state_basis=basis, **kw)
    m.X_0 = prob.X_0.clone()
    if small:
        with torch.no_grad():
            for p in m.z_n.parameters():
                p.mul_(2.0 ** -10)
    return prob, m


def _images(plan, N, K):
    """X_n (N, K, d_pad), h1, h2 (N, K, H_pad), xi_{n+1} (N, K, d_pad) from the register images of the path store: block (n, tile)
    = [X | h1 | h2 | xi], image float ks * 64 + 16 q + j = feature 16 (ks // 4) + 4 (ks % 4) + q of sample j (Geo::pX ..)."""
    nt, dp, Hp = (K + 15) // 16, plan.d_pad, plan.H_pad
    DB, HB = (dp + 15) // 16, (Hp + 15) // 16
    blocks = plan.path.view(-1)[:N * nt * 64 * 8 * (DB + HB)].view(N, nt, -1)

    def take(off, NB, width):
        img = blocks[:, :, off:off + 4 * NB * 64].reshape(N, nt, NB, 4, 4, 16)          # (b, r, q, j)
        return img.permute(0, 1, 5, 2, 3, 4).reshape(N, nt * 16, NB * 16)[:, :K, :width].double().cpu()
    return take(0, DB, dp), take(4 * DB * 64, HB, Hp), take(4 * (DB + HB) * 64, HB, Hp), take(4 * (DB + 2 * HB) * 64, DB, dp)


def _ref64(plan, prob, params, xi, N, K):
    """The rollout of the kernel's own problem in float64: (D (K), X (N, K, d_pad), h1, h2)."""
    dp, Hp, d = plan.d_pad, plan.H_pad, prob.d
    P = params.double().cpu()
    o = 0
    W1 = P[o:o + Hp * (dp + 1)].view(Hp, dp + 1); o += Hp * (dp + 1)
    b1 = P[o:o + Hp]; o += Hp
    W2 = P[o:o + Hp * Hp].view(Hp, Hp); o += Hp * Hp
    b2 = P[o:o + Hp]; o += Hp
    W3 = P[o:o + dp * Hp].view(dp, Hp); o += dp * Hp
    b3 = P[o:o + dp]
    A, B = prob.A.double().cpu().numpy(), prob.B.double().cpu().numpy()
    al, x0 = prob.alpha[:, 0].double().cpu().numpy(), prob.X_0.double().cpu().numpy()
    if plan.state_basis == "sigma":                      # what plan_native.py hands the kernels: fp64 on the host, rounded to fp32
        M, al, x0 = psp.plan_native.sigma_basis_problem(A, B, al, x0)
        A, B = torch.from_numpy(M).float().double(), torch.eye(d, dtype=F64)
        al, x0 = torch.from_numpy(al).float().double(), torch.from_numpy(x0).float().double()
    else:
        A, B, al, x0 = torch.from_numpy(A), torch.from_numpy(B), torch.from_numpy(al), torch.from_numpy(x0)

    def pad(v, n):
        return torch.cat([v, torch.zeros(*v.shape[:-1], n - v.shape[-1], dtype=F64)], -1)
    Ap, Bp = torch.zeros(dp, dp, dtype=F64), torch.zeros(dp, dp, dtype=F64)
    Ap[:d, :d], Bp[:d, :d] = A, B
    dt, sq = float(plan.cfg.dt), float(plan.cfg.sqrt_dt)
    X, Y = pad(x0, dp).repeat(K, 1), torch.zeros(K, dtype=F64)
    Xs, H1, H2 = [], [], []
    for n in range(N):
        tn = float(torch.tensor(float(n)) * torch.tensor(dt))                       # the kernel's fp32 n * dt
        h1 = torch.tanh(tn * W1[:, 0] + X @ W1[:, 1:].t() + b1)
        h2 = torch.tanh(h1 @ W2.t() + b2)
        Z = h2 @ W3.t() + b3
        Xs.append(X); H1.append(h1); H2.append(h2)
        v = sq * xi[n] - dt * Z
        X = X + dt * (X @ Ap.t()) + v @ Bp.t()
        Y = Y - 0.5 * (Z * Z).sum(1) * dt + (Z * xi[n]).sum(1) * sq
    return Y - X @ pad(al, dp), torch.stack(Xs), torch.stack(H1), torch.stack(H2)


def _forward(d, H, mlp, basis, inst, small):
    prob, m = _solver(d, H, mlp, basis, small=small)
    params0 = flat_params(m.z_n)
    m.train()
    plan = m._native_plan
    assert m.N == N_FWD and plan.matrix_mode == mlp and plan.family == 1 and plan.state_basis == basis
    assert (plan.d_pad, plan.H_pad) == inst and plan.cfg.store_path == 1 and m.range_fallback_iterations == 0
    # the kernel-layout parameters of the rollout (train() took an Adam step since): sigma basis -- the plan's own buffer, which
    # holds W1x B; x basis -- the saved ones, padded
    params = plan.flat_k.clone() if basis == "sigma" else plan.pad.scatter_params(params0.to(dev()), plan.pad.new_padded_params())
    X, h1, h2, xi = _images(plan, N_FWD, K_FWD)
    return prob, plan, params, dict(D=plan.D.double().cpu(), X=X, h1=h1, h2=h2), xi


def _forward_case(d, H, basis, inst, small=False):
    """(errors of the split kernel against float64, of the fp32 twin, distance between the two), each (D, X, h1, h2)"""
    prob, plan, params, x3, xi = _forward(d, H, "f16x3", basis, inst, small)
    _, plan2, params2, f32, xi2 = _forward(d, H, "fp32", basis, inst, small)
    assert torch.equal(params, params2) and torch.equal(xi, xi2), "same inputs"
    D, X, h1, h2 = _ref64(plan, prob, params, xi, N_FWD, K_FWD)
    ref = dict(D=D, X=X, h1=h1, h2=h2)
    keys = ("D", "X", "h1", "h2")
    assert all(bool(torch.isfinite(x3[k]).all()) for k in keys)
    return (tuple(float((x3[k] - ref[k]).abs().max()) for k in keys), tuple(float((f32[k] - ref[k]).abs().max()) for k in keys),
            tuple(float((x3[k] - f32[k]).abs().max()) for k in keys))


def _hold(tag, e3, e2, e32):
    print("one_accumulator %s: x3-f64 %s  fp32-f64 %s  x3-fp32 %s  parent %s" % (
        tag, " ".join("%.3e" % e for e in e3), " ".join("%.3e" % e for e in e2), " ".join("%.3e" % e for e in e32), PARENT[tag]))
    for name, a, b, c, p in zip(("D", "X", "h1", "h2"), e3, e2, e32, PARENT[tag]):
        assert a <= MARGIN * p, (tag, name, a, p)
        assert c <= MARGIN * p + b, (tag, name, c, p, b)


@pytest.mark.parametrize("d,H,basis,inst", FWD_CASES, ids=["d%d-H%d-%s" % c[:3] for c in FWD_CASES])
def test_forward_against_float64_and_the_fp32_twin(d, H, basis, inst):
    _hold("d%d-H%d-%s" % (d, H, basis), *_forward_case(d, H, basis, inst))


def test_forward_small_operands():
    """States and weights times 2^-10 on the (40, 32) case: pre-activations ~ 1e-4, the lo parts of the scaled operands subnormal
    f16.  Absolute errors, as above."""
    _hold("d40-H32-x-small", *_forward_case(40, 32, "x", (48, 32), True))


# ---- backward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H,inst", SHAPES, ids=["d%d-H%d" % s[:2] for s in SHAPES])
def test_backward_against_the_fp32_twin_per_workgroup_and_in_total(d, H, inst):
    K, N = ragged_K(torch.cuda.get_device_properties(dev()).multi_processor_count), N_STEPS
    g = torch.Generator(device="cpu").manual_seed(11)
    w = (torch.randn(K, generator=g) * (2.0 / K)).to(dev())
    got = {}
    for store_path in (1, 4):
        prob, m = _solver(d, H, "f16x3", "auto", K=K, N=N, x0=None, path_noise="store" if store_path == 1 else "auto")
        params0 = flat_params(m.z_n)
        m.train()
        plan = m._native_plan
        assert m.N == N and plan.matrix_mode == "f16x3" and plan.family == 1
        assert (plan.d_pad, plan.H_pad) == inst and plan.cfg.store_path == store_path
        params0 = plan.pad.scatter_params(params0.to(dev()), plan.pad.new_padded_params())
        g3, rows3 = _bwd(plan, m, params0, w, nat.MLP_F16X3)
        g2, rows2 = _bwd(plan, m, params0, w, nat.MLP_FP32)
        scale = float(g2.abs().max())
        err = float((g3 - g2).abs().max())
        rs = rows2.abs().max(dim=1).values.clamp_min(1e-30)
        rel = (rows3 - rows2).abs().max(dim=1).values / rs
        print("one_accumulator bwd d=%d H=%d store_path=%d: total %.3e of %.3e, worst workgroup %.3e" % (
            d, H, store_path, err / scale, scale, float(rel.max())))
        assert scale > 0 and torch.isfinite(g3).all() and not torch.equal(g3, g2)
        assert err <= 2e-5 * scale
        assert_blocks(g3, g2, plan.d_pad, plan.H_pad, 2e-5, tag="x3 vs fp32 on the one-accumulator forward's store d=%d H=%d" % (d, H))
        assert float(rel.max()) <= 1e-4, (int(rel.argmax()), float(rel.max()))
        for _ in range(2):
            g3b, rows3b = _bwd(plan, m, params0, w, nat.MLP_F16X3)
            assert torch.equal(g3b, g3) and torch.equal(rows3b, rows3)
        got[store_path] = (g3, rows3)
    assert torch.equal(got[1][0], got[4][0]) and torch.equal(got[1][1], got[4][1]), "stored and regenerated increments: one result"


# ---- range ----------------------------------------------------------------------------------------------------------------------
def _ranged(mlp, entry, **kw):
    x0 = torch.linspace(-1.0, 1.0, 100)
    x0[3] = entry
    prob, m = _solver(100, 64, mlp, "x", x0=x0, loss="moment", **kw)
    m.train()
    return m


@pytest.mark.parametrize("entry", [7.0e4, 3000.0], ids=["beyond_f16", "between_new_and_old_threshold"])
def test_state_beyond_the_scaled_range_takes_the_fp32_twin(entry):
    got, ref = _ranged("f16x3", entry), _ranged("fp32", entry)
    assert got._native_plan.matrix_mode == "f16x3" and got.range_fallback_iterations == 1
    assert math.isfinite(ref.loss_log[0]) and got.loss_log == ref.loss_log
    assert torch.equal(got._native_plan.grad, ref._native_plan.grad) and torch.equal(got._native_plan.D, ref._native_plan.D)
    raw = _ranged("f16x3", entry, range_guard=False)                    # the test means something: unguarded, the split forward is NaN
    assert not math.isfinite(raw.loss_log[0])


def test_half_the_input_threshold_stays_on_the_split_kernels():
    """|input| < 65504 / 2^kLgFwdB = 2047 (csrc/hjb_kernels.h): an entry at 1023 is in range -- no fallback, the unguarded result."""
    got, raw = _ranged("f16x3", 1023.0), _ranged("f16x3", 1023.0, range_guard=False)
    assert got._native_plan.range_flag is not None and got.range_fallback_iterations == 0
    assert math.isfinite(got.loss_log[0]) and got.loss_log == raw.loss_log
    assert torch.equal(got._native_plan.grad, raw._native_plan.grad)
