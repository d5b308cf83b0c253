"""The case table of tests/test_gpu_block_gradients.py (GPU) and of the regime check in tests/test_ref64.py (CPU): one list, so that
both iterate over the same cases.

Every case scales the initial N(0, 0.01) weights of the tanh net (default_scale below: x 30 for d <= 40, x 15 for d = 100 .. 130,
x 10 from d = 200 on, where x 30 saturates the hidden layers; less for the double well, whose X_0 = -1 feeds the first layer d
inputs of size one) so that the activations are O(1): tanh' = 1 - h^2 then differs from 1 by tens of per cent and every block of the
gradient carries signal.  The CPU test asserts exactly that of every case's float64 reference.
"""
import torch

from util_cases import make_oracle

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


def reference(c, K, noise):
    """ref64.iteration of the case, computed once per (problem, shape, flags, noise mode) -- the matrix mode and the kernel switches
    do not enter -- and never modified.  `noise`: a callable returning (K, d, N + 1), evaluated on a miss only."""
    key = reference_key(c, K)
    if key not in _REFS:
        oprob, ocfg, z = scaled_oracle(c, K)
        _REFS[key] = ref64.iteration(oprob, ocfg, z, noise())
    return _REFS[key]


def loss_values(loss, D):
    """The per-trajectory values whose spread the loss measures: exp(D) = exp(Y - g) for the variance loss, D otherwise."""
    return torch.exp(D.double()) if loss == "variance" else D.double()


def first_loss_tol(values, loss_ref):
    """The conditioning rule of test_gpu_parity.check_first_iteration: an fp32 implementation of mean(v^2) - mean(v)^2 is off by
    about eps * mean(v^2) / |loss|; never below 2e-5, capped by the contract's 1e-4."""
    cond = float((values.double() ** 2).mean()) / max(abs(loss_ref), 1e-30)
    return min(1e-4, max(2e-5, 4 * 6e-8 * cond))
