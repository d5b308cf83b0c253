"""The case table of tests/test_gpu_block_gradients.py (GPU) and of the regime check in tests/test_ref64.py (CPU): one list, so that
both iterate over the same cases.

Every case scales the initial N(0, 0.01) weights of the tanh net (default_scale below: x 30 for d <= 40, x 15 for d = 100 .. 130,
x 10 from d = 200 on, where x 30 saturates the hidden layers; less for the double well, whose X_0 = -1 feeds the first layer d
inputs of size one) so that the activations are O(1): tanh' = 1 - h^2 then differs from 1 by tens of per cent and every block of the
gradient carries signal.  The CPU test asserts exactly that of every case's float64 reference.

BF16_CASES (below) is the table of tests/test_gpu_bf16_blocks.py and tests/test_ref64_bf16.py: Solver(mlp_dtype='bf16') against
the float64 reference with bf16 operands, with the criterion both files share (bf16_errors, assert_bf16).
"""
import torch

from util_cases import BLOCK_NAMES, block_errors, make_oracle

import ref64

ASSUMED_CUS = 256           # the CPU regime check sizes the 'cu' case for an MI355X; the GPU test reads the device


def default_scale(kind, d):
    """Chosen on the CPU from the float64 reference (tests/test_ref64.py asserts the outcome: median |h1|, |h2| in [0.15, 0.85])."""
    if kind == "DoubleWell_multidim":
        return 15.0 if d <= 40 else 10.0
    return 30.0 if d <= 40 else (15.0 if d < 200 else 10.0)


def _c(route, kind, d, H, K, N, detach, mode, expect, loss="log-variance", dt=0.05, noise="reference", env=None, scale=None, regen=False):
    """expect = (family, d_pad, H_pad); env: the kernel switches the case pins (PSP_FWD_VARIANT, PSP_WIDE_BWD_X3), read per launch."""
    env = dict(env or {})
    if scale is None:
        scale = default_scale(kind, d)
    cid = "%s-%s-d%d-H%d-K%s-%s-%s-%s%s" % (route, kind[:4], d, H, K, "det" if detach else "att", mode, loss[:6],
                                            "".join("-%s%s" % (k[4:].lower(), v) for k, v in sorted(env.items())))
    return dict(id=cid, route=route, kind=kind, d=d, H=H, K=K, N=N, detach=detach, mode=mode, expect=expect, loss=loss, dt=dt,
                noise=noise, env=env, scale=scale, regen=regen)


def _narrow():
    out = []
    V = lambda v: {"PSP_FWD_VARIANT": str(v)}
    # padded shapes, ragged K: one hidden block / three hidden blocks; every forward of the family, detached and attached
    for kind, d, H, K, exp in (("LLGC", 12, 16, 37, (1, 16, 16)), ("LQGC", 20, 40, 72, (1, 32, 48))):
        for detach in (True, False):
            for v in (1, 2, 3):
                out.append(_c("narrow-fp32-v%d" % v, kind, d, H, K, 4, detach, "fp32", exp, env=V(v)))
            out.append(_c("narrow-f16x3", kind, d, H, K, 4, detach, "f16x3", exp))
    # the exact (100, 64) instance
    for detach in (True, False):
        out.append(_c("narrow-fp32-v1", "LLGC", 100, 64, 48, 3, detach, "fp32", (1, 100, 64), env=V(1)))
        out.append(_c("narrow-f16x3", "LLGC", 100, 64, 48, 3, detach, "f16x3", (1, 100, 64)))
    # several backward rounds per workgroup (N * ceil(K / 16) / 4 rounds on one workgroup per CU), ragged last tile
    out.append(_c("narrow-rounds", "LQGC", 20, 40, 9001, 4, True, "fp32", (1, 32, 48), env=V(1)))
    out.append(_c("narrow-rounds", "LQGC", 20, 40, 9001, 4, True, "f16x3", (1, 32, 48)))
    out.append(_c("narrow-rounds", "LLGC", 40, 48, 9001, 4, False, "f16x3", (1, 48, 48)))
    # store_path 4: the backward regenerates xi (on-device noise, detached, more than two tiles per CU)
    for mode in ("f16x3", "fp32"):
        out.append(_c("narrow-store4", "LLGC", 20, 40, "cu", 3, True, mode, (1, 32, 48), noise="philox", regen=True,
                      env=V(1) if mode == "fp32" else None))
    # relative entropy (store_path 3) and a loss on generic trajectory weights
    for mode in ("fp32", "f16x3"):
        env = V(1) if mode == "fp32" else None
        out.append(_c("narrow-relent", "LLGC", 17, 33, 40, 4, False, mode, (1, 32, 48), loss="relative_entropy", env=env))
        out.append(_c("narrow-variance", "LQGC", 33, 17, 40, 4, False, mode, (1, 48, 32), loss="variance", env=env))
        # element-wise drift and its Jacobian in the adjoint sweep
        out.append(_c("narrow-doublewell", "DoubleWell_multidim", 30, 64, 50, 4, False, mode, (1, 32, 64), env=env))
    return out


def _wide():
    out = []
    X3 = lambda v: {"PSP_WIDE_BWD_X3": str(v)}
    for d, H, exp in ((120, 64, (2, 128, 64)), (200, 64, (2, 200, 64)), (250, 50, (2, 256, 64))):
        out.append(_c("wide-fp32", "LLGC", d, H, 48, 3, True, "fp32", exp))
        out.append(_c("wide-fp32", "LLGC", d, H, 48, 3, False, "fp32", exp))
        out.append(_c("wide-f16x3-bwdx3", "LLGC", d, H, 48, 3, True, "f16x3", exp, env=X3(1)))
        out.append(_c("wide-f16x3-bwdfp32", "LLGC", d, H, 48, 3, True, "f16x3", exp, env=X3(0)))
        out.append(_c("wide-f16x3-adjoint", "LLGC", d, H, 48, 3, False, "f16x3", exp))
    # d > 256: the streaming split backward and, with on-device noise, the cooperative forward
    e320 = (2, 320, 64)
    out.append(_c("wide-fp32", "LLGC", 320, 64, 48, 3, True, "fp32", e320))
    out.append(_c("wide-fp32", "LLGC", 320, 64, 48, 3, False, "fp32", e320))
    out.append(_c("wide-f16x3-stream", "LLGC", 320, 64, 48, 3, True, "f16x3", e320))
    out.append(_c("wide-f16x3-stream-coop", "LLGC", 320, 64, 48, 3, True, "f16x3", e320, noise="philox"))
    out.append(_c("wide-f16x3-adjoint", "LLGC", 320, 64, 48, 3, False, "f16x3", e320, noise="philox"))
    # running cost + quadratic terminal cost
    for mode in ("fp32", "f16x3"):
        out.append(_c("wide-lqgc", "LQGC", 130, 40, 40, 3, False, mode, (2, 192, 64)))
    # several rounds per workgroup, ragged last tile
    out.append(_c("wide-rounds", "LLGC", 200, 64, 9001, 3, True, "fp32", (2, 200, 64)))
    out.append(_c("wide-rounds", "LLGC", 200, 64, 9001, 3, True, "f16x3", (2, 200, 64), env=X3(1)))
    out.append(_c("wide-rounds", "LLGC", 320, 64, 9001, 3, True, "f16x3", e320, noise="philox"))
    for mode in ("fp32", "f16x3"):
        out.append(_c("wide-doublewell", "DoubleWell_multidim", 150, 64, 50, 4, False, mode, (2, 192, 64)))
    return out


CASES = _narrow() + _wide()
assert len({c["id"] for c in CASES}) == len(CASES)


def _bf16():
    """Solver(mlp_dtype='bf16'): hjb_fwd_kernel<D, H, MODE = 1, FAST = 0 | 1> -- supplied noise launches FAST = 0, Philox noise the
    FAST = 1 instance -- followed by the fp32 backward (detached: hjb_bwd2, attached: hjb_adj).  Judged against ref64.iteration(...,
    operands='bf16') by tests/test_gpu_bf16_blocks.py; the conditions on the table are asserted by tests/test_ref64_bf16.py.

    The first four instances are those whose W1 table is larger as a bf16 image than as an fp32 one (Geo::tbl, d <= 12); each runs
    on both noise modes, once detached and once attached."""
    out = []
    b = lambda route, kind, d, H, K, N, detach, exp, noise, **kw: out.append(
        _c(route, kind, d, H, K, N, detach, "bf16", exp, noise=noise, **kw))
    for noise, detach in (("reference", True), ("philox", False)):
        b("bf16-d10", "LLGC", 10, 30, 65, 20, detach, (1, 10, 30), noise)
        # (x 30: at the double well's x 15 the rounding error of W1x's block, 6e-4, is within x 3 of the fp32 block bound)
        b("bf16-d4", "DoubleWell_multidim", 4, 30, 40, 4, detach, (1, 4, 30), noise, scale=30.0)
    for noise, detach in (("reference", False), ("philox", True)):
        b("bf16-d2", "LLGC", 2, 30, 48, 4, detach, (1, 2, 30), noise)
        b("bf16-d8", "LQGC", 8, 30, 40, 4, detach, (1, 8, 30), noise)
    # d = 5, H = 20: padded onto the cheapest instance that covers it (native_shapes.candidates), (8, 30) -- an overrunning one
    b("bf16-pad-d5", "LLGC", 5, 20, 37, 4, True, (1, 8, 30), "philox")
    # the two images of every table exactly equal (16 features = half a bf16 k-step, zero-filled)
    b("bf16-16x16", "LLGC", 16, 16, 37, 4, True, (1, 16, 16), "reference")
    b("bf16-16x16", "LLGC", 16, 16, 37, 4, False, (1, 16, 16), "philox")
    # exact (20, 30); ragged K over 19 tiles
    b("bf16-20x30", "LLGC", 20, 30, 299, 4, False, (1, 20, 30), "reference")
    # odd block counts: the zero-filled half k-step of gemm_Tb on every product (48, 48), on the state only (100, 64: DB = 7)
    b("bf16-48x48", "LLGC", 40, 48, 72, 4, True, (1, 48, 48), "reference")
    b("bf16-48x48", "LQGC", 40, 48, 72, 4, False, (1, 48, 48), "philox")
    b("bf16-48x64", "LQGC", 33, 50, 40, 4, False, (1, 48, 64), "reference")
    b("bf16-100x64", "LLGC", 100, 64, 32, 5, True, (1, 100, 64), "philox")
    b("bf16-100x64", "LLGC", 100, 64, 32, 5, False, (1, 100, 64), "reference")
    # store_path 4: the backward regenerates xi (more than two tiles per CU, detached, Philox noise).  LQGC: over these 8208
    # trajectories the fp32 stand-in's worst D is 0.16 of the rounding error here, 0.26 on LLGC -- past the stand-in's 1/4
    b("bf16-store4", "LQGC", 20, 40, "cu", 3, True, (1, 32, 48), "philox", regen=True)
    return out


BF16_CASES = _bf16()
assert len({c["id"] for c in BF16_CASES}) == len(BF16_CASES)
BF16_OVERRUN = ((2, 30), (4, 30), (8, 30), (10, 30))       # instances whose bf16 W1 image exceeds the fp32 one


def case_K(c, cus=ASSUMED_CUS):
    """'cu': one tile more than two per CU -- the smallest K at which the plan picks store_path 4."""
    return 16 * (2 * cus + 1) if c["K"] == "cu" else c["K"]


def golden_style(c, K):
    """The case in the layout util_cases.make_pkg_solver / make_oracle take."""
    kind, d, N, dt = c["kind"], c["d"], c["N"], c["dt"]
    T = (N + 0.5) * dt                                       # floor(T / dt) = N whatever the rounding of N * dt
    if kind == "DoubleWell_multidim":
        d_2 = max(1, d // 15)                                # (eta = 1 on these: 4 per component in g(X_0), keeps |D| moderate)
        kwargs = dict(d=d, d_1=d - d_2, d_2=d_2, T=T, eta=0.05, kappa=0.5)
    elif kind == "LQGC":
        kwargs = dict(d=d, off_diag=0.05, T=T, seed=42, delta_t=dt)
    else:
        kwargs = dict(d=d, off_diag=0.3 / d ** 0.5, T=T, seed=42)
    solver = dict(loss_method=c["loss"], time_approx="inner", adaptive_forward_process=True, detach_forward=c["detach"],
                  early_stopping_time=None, L=1, lr=0.001, seed=42, delta_t=dt, K=K, u_l2_error_flag=False)
    return dict(name="blocks", family="solver", problem=dict(kind=kind, kwargs=kwargs), solver=solver,
                net=dict(kind="tanh_mlp", widths=[c["H"], c["H"]], seed=123))


def scaled_oracle(c, K):
    """(OracleProblem, HJBConfig, TanhMLP with its weights x scale)."""
    oprob, ocfg, omodels = make_oracle(golden_style(c, K), L=1)
    with torch.no_grad():
        for p in omodels[0].parameters():
            p.mul_(c["scale"])
    return oprob, ocfg, omodels[0]


def host_noise(seed, K, d, N):
    """What noise='reference' draws in the first iteration with a fixed X_0 (solver.py:422, :381; hjb_train does the same)."""
    torch.manual_seed(seed)
    return torch.randn(K, d, N + 1)


def reference_key(c, K):
    return (c["kind"], c["d"], c["H"], K, c["N"], c["detach"], c["loss"], c["dt"], c["scale"], c["noise"])


_REFS = {}


def reference(c, K, noise, operands="fp32", dtype=torch.float64):
    """ref64.iteration of the case, computed once per (problem, shape, flags, noise mode) -- the matrix mode and the kernel switches
    do not enter -- and never modified.  `noise`: a callable returning (K, d, N + 1), evaluated on a miss only.  operands, dtype:
    ref64.iteration's (the bf16-operand model and its fp32 stand-in), each kept under a key of its own."""
    key = reference_key(c, K) + (() if (operands, dtype) == ("fp32", torch.float64) else (operands, dtype))
    if key not in _REFS:
        oprob, ocfg, z = scaled_oracle(c, K)
        _REFS[key] = ref64.iteration(oprob, ocfg, z, noise(), operands=operands, dtype=dtype)
    return _REFS[key]


BF16_C = 0.5                # tests/test_gpu_bf16_blocks.py; the CPU stand-in of tests/test_ref64_bf16.py is held to half of it


def bf16_errors(c, got, model, exact):
    """The three-value criterion of the bf16 tests.  got / model / exact: dict(D, loss, grad) of the implementation under test, of
    the float64 reference with bf16 operands and of the exact float64 reference.  Returns (e_kernel, e_model), each a dict with D
    (of max(1, max |D|)), loss (relative) and blocks (util_cases.block_errors): e_kernel = |got - model|, e_model = |model - exact|.
    For the loss e_model is max(e_model(loss), e_model(D)): one realised scalar difference can cancel by chance."""
    def errs(a, r):
        D, Dr = a["D"].double().cpu(), r["D"].double()
        assert D.shape == Dr.shape and bool(torch.isfinite(D).all())
        return dict(D=float((D - Dr).abs().max()) / max(1.0, float(Dr.abs().max())), loss=abs(a["loss"] - r["loss"]) / abs(r["loss"]),
                    blocks=block_errors(a["grad"], r["grad"], c["d"], c["H"]))
    ek, em = errs(got, model), errs(model, exact)
    em["loss"] = max(em["loss"], em["D"])
    return ek, em


def assert_bf16(c, got, model, exact, coeff, d_tol, block_tol, tag=""):
    """e_kernel <= coeff e_model + (the fp32 siblings' bound) for D, the loss and each of the seven blocks; prints every figure
    before it asserts.  Returns (e_kernel, e_model)."""
    ek, em = bf16_errors(c, got, model, exact)
    tol_l = first_loss_tol(loss_values(c["loss"], model["D"]), model["loss"])
    rows = [("D", ek["D"], em["D"], d_tol), ("loss", ek["loss"], em["loss"], tol_l)]
    rows += [(n, a, b, block_tol) for n, a, b in zip(BLOCK_NAMES, ek["blocks"], em["blocks"])]
    print("%s  " % tag + "  ".join("%s %.2e/%.2e" % r[:3] for r in rows) + "   (e_kernel/e_model)")
    bad = [r for r in rows if not r[1] <= coeff * r[2] + r[3]]
    assert not bad, (tag, coeff, bad)
    return ek, em


def loss_values(loss, D):
    """The per-trajectory values whose spread the loss measures: exp(D) = exp(Y - g) for the variance loss, D otherwise."""
    return torch.exp(D.double()) if loss == "variance" else D.double()


def first_loss_tol(values, loss_ref):
    """The conditioning rule of test_gpu_parity.check_first_iteration: an fp32 implementation of mean(v^2) - mean(v)^2 is off by
    about eps * mean(v^2) / |loss|; never below 2e-5, capped by the contract's 1e-4."""
    cond = float((values.double() ** 2).mean()) / max(abs(loss_ref), 1e-30)
    return min(1e-4, max(2e-5, 4 * 6e-8 * cond))
