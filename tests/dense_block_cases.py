"""The case table of tests/test_gpu_dense_block_gradients.py (GPU) and of the regime check in tests/test_ref64_dense.py (CPU): one
list, so that both iterate over the same cases of the DenseNet-control kernels (csrc/hjbd_kernels.h, plan_dense_native.py).

At its initial state (weights 0.1 randn, ALL-ZERO biases, X_0 = 0 on LLGC / LQGC) the family's gradient is nearly all b3: with
time_approx='outer' every hidden unit of the step-0 net is exactly zero, and relu(.)**2 of the small later activations leaves the
W2[h1] rows at 3e-5 of the maximum.  Every case here therefore
  * scales the weight matrices (`scale`; relu(.)**2 grows quadratically, so the window is narrow and chosen per shape),
  * draws the biases N(0, bias_std) from a seeded generator, in parameter order, the same numbers on both sides, and
  * starts LLGC / LQGC from X_0 = x0 * cos(i) (the double wells keep their own X_0 = -1),
chosen on the CPU from the float64 reference until every block of every parameter set carries signal; tests/test_ref64_dense.py
asserts that of every case.

Instances and backward routes (csrc/dense_instances.def, DnetLaunch::kPasses): the hand-written backward runs in ONE launch on
(16 .. 128, 32) and (16 .. 64, 64), in TWO column passes on (112, 64) and (128, 64), and not at all on (256, .), where the plan takes
the library-GEMM formulation (also forced by PSP_DENSE_BWD=gemm).  Detached adaptive f16x3 runs take the split-product outer
products (store_path 1), every other f16x3 run the fp32 ones; attached runs and the relative entropy go through hjbd_adj_kernel.
The SPEC forward is chosen for f16x3 + Philox noise + LLGC + 'outer' (no time feature) + adaptive, not the relative entropy.
"""
import torch

from util_cases import orc

import ref64

X0_AMPLITUDE = 0.5          # X_0[i] = 0.5 cos(i) where the problem's own X_0 is zero
BIAS_STD = 0.1
BIAS_SEED = 7


def default_scale(tmode, kind, d, H):
    """Weight matrices x this.  Chosen on the CPU from the float64 reference (tests/test_ref64_dense.py asserts the outcome)."""
    if kind == "DoubleWell_multidim":                        # X_0 = -1 feeds the first layer d inputs of size one
        return 0.8 if d <= 100 else 0.5
    if d <= 24:
        return 2.0
    if d <= 64:
        return 1.0
    return 0.7 if d <= 130 else 0.5


def _c(tmode, kind, d, H, K, N, detach, mode, expect, bwd, loss="log-variance", dt=0.05, noise="reference", env=None, adaptive=True,
       scale=None, bias_std=BIAS_STD, x0=X0_AMPLITUDE, slices_gt1=False):
    """expect = (d_pad, H_pad); bwd: 'kernel1' / 'kernel2' (hjbd_bwd_kernel in one launch / two column passes) or 'gemm'."""
    env = dict(env or {})
    attached = adaptive and not detach
    relent = loss == "relative_entropy"
    spec = mode == "f16x3" and noise == "philox" and kind == "LLGC" and tmode == "outer" and adaptive and not relent
    fwd = "spec" if spec else mode
    if bwd == "gemm":
        back = "gemm"
    elif attached:
        back = "adj" + ("-x3" if mode == "f16x3" else "-fp32")
    else:
        back = "bwd-x3" if (mode == "f16x3" and adaptive) else "bwd-fp32"
    route = "%dx%d/%s/%s%s%s" % (expect[0], expect[1], fwd, back, "-relent" if relent else "", "-2pass" if bwd == "kernel2" else "")
    if scale is None:
        scale = default_scale(tmode, kind, d, H)
    cid = "%s-%s-d%d-H%d-K%d-N%d-%s%s-%s-%s%s%s" % (tmode, kind[:4], d, H, K, N, "det" if detach else "att", "" if adaptive else "-nonadp",
                                                   mode, loss[:6], "-philox" if noise == "philox" else "",
                                                   "".join("-%s" % v for _, v in sorted(env.items())))
    return dict(id=cid, route=route, tmode=tmode, kind=kind, d=d, H=H, K=K, N=N, detach=detach, mode=mode, expect=expect, bwd=bwd,
                loss=loss, dt=dt, noise=noise, env=env, adaptive=adaptive, scale=scale, bias_std=bias_std, x0=x0, slices_gt1=slices_gt1,
                spec=spec)


def _cases():
    out = []
    four = [(True, "fp32"), (True, "f16x3"), (False, "fp32"), (False, "f16x3")]
    gemm = {"PSP_DENSE_BWD": "gemm"}
    # (16, 32) padded, ragged K;  (32, 64): running cost and time rows;  exact (64, 64)
    for detach, mode in four:
        out.append(_c("outer", "LLGC", 12, 16, 37, 4, detach, mode, (16, 32), "kernel1"))
    for detach, mode in four:
        out.append(_c("inner", "LQGC", 20, 40, 72, 4, detach, mode, (32, 64), "kernel1"))
    for detach, mode in four:
        out.append(_c("inner", "LLGC", 64, 64, 48, 3, detach, mode, (64, 64), "kernel1"))
    # (112, 32), the benchmark instance
    b = ("outer", "LLGC", 100, 30, 48, 3)
    out.append(_c(*b, True, "fp32", (112, 32), "kernel1"))
    out.append(_c(*b, True, "f16x3", (112, 32), "kernel1"))
    out.append(_c(*b, False, "f16x3", (112, 32), "kernel1"))
    for mode in ("fp32", "f16x3"):                             # store_path 3, nu weights
        out.append(_c(*b, False, mode, (112, 32), "kernel1", loss="relative_entropy"))
    out.append(_c(*b, True, "f16x3", (112, 32), "kernel1", noise="philox"))            # the SPEC forward
    out.append(_c(*b, False, "f16x3", (112, 32), "kernel1", noise="philox"))
    # Philox noise off the SPEC forward: a running cost, and the fp32 forward
    out.append(_c("outer", "LQGC", 24, 20, 40, 4, True, "f16x3", (32, 32), "kernel1", noise="philox"))
    out.append(_c("outer", "LQGC", 24, 20, 40, 4, True, "fp32", (32, 32), "kernel1", noise="philox"))
    # two column passes: (112, 64) and (128, 64); generic trajectory weights, explicit wT
    for detach, mode in four:
        out.append(_c("inner", "LLGC", 100, 64, 48, 3, detach, mode, (112, 64), "kernel2"))
    out.append(_c("inner", "LLGC", 100, 64, 48, 3, False, "fp32", (112, 64), "kernel2", loss="cross_entropy"))
    out.append(_c("outer", "LLGC", 120, 50, 48, 3, True, "f16x3", (128, 64), "kernel2"))
    out.append(_c("outer", "LLGC", 120, 50, 48, 3, False, "fp32", (128, 64), "kernel2"))
    # (exp(D) is what the variance loss averages: a shorter step keeps the spread of D = Y - sum_i X_N[i] at d = 120 moderate)
    out.append(_c("outer", "LLGC", 120, 50, 48, 3, True, "f16x3", (128, 64), "kernel2", loss="variance", dt=0.02))
    # element-wise drift and its Jacobian in the adjoint sweep; the non-adaptive image (fp32 backward even in f16x3).  d = 65 runs on
    # (112, 32) since that instance exists (_instance_for takes the cheapest cover); d = 115 is what reaches (128, 32)
    for d, exp in ((65, (112, 32)), (115, (128, 32))):
        dw = ("inner", "DoubleWell_multidim", d, 30, 50, 4)
        out.append(_c(*dw, False, "fp32", exp, "kernel1"))
        out.append(_c(*dw, False, "f16x3", exp, "kernel1"))
        out.append(_c(*dw, True, "f16x3", exp, "kernel1", adaptive=False))
    # the library-GEMM backward: (256, .), and forced on the two smallest cases
    for mode in ("fp32", "f16x3"):
        out.append(_c("outer", "LLGC", 130, 40, 24, 3, True, mode, (256, 64), "gemm"))
        out.append(_c("inner", "LQGC", 200, 16, 20, 3, True, mode, (256, 32), "gemm", x0=0.15, dt=0.04, scale=1.0))   # (200 quadratic cost terms: |D| <= 50)
    out.append(_c("outer", "LLGC", 12, 16, 37, 4, True, "fp32", (16, 32), "gemm", env=gemm))
    out.append(_c("inner", "LQGC", 20, 40, 72, 4, True, "fp32", (32, 64), "gemm", env=gemm))
    # several slices per step and several rounds per backward workgroup, ragged last tile
    r = ("outer", "LLGC", 20, 30, 9001, 4)
    out.append(_c(*r, True, "fp32", (32, 32), "kernel1", slices_gt1=True))
    out.append(_c(*r, True, "f16x3", (32, 32), "kernel1", slices_gt1=True))
    out.append(_c(*r, False, "f16x3", (32, 32), "kernel1", slices_gt1=True))
    out.append(_c(*r, True, "f16x3", (32, 32), "kernel1", slices_gt1=True, noise="philox"))
    # N = 1
    out.append(_c("outer", "LQGC", 17, 33, 16, 1, True, "f16x3", (32, 64), "kernel1", loss="moment"))
    out.append(_c("outer", "LQGC", 17, 33, 16, 1, False, "fp32", (32, 64), "kernel1", loss="moment"))
    return out


CASES = _cases()
assert len({c["id"] for c in CASES}) == len(CASES)


def golden_style(c):
    """The problem / solver keywords of the case in the layout of the golden cases."""
    kind, d, N, dt = c["kind"], c["d"], c["N"], c["dt"]
    T = (N + 0.5) * dt                                       # floor(T / dt) = N whatever the rounding of N * dt
    if kind == "DoubleWell_multidim":
        d_2 = max(1, d // 15) if d <= 100 else 2             # (eta = 1 on these: 4 per component in g(X_0), keeps |D| moderate)
        kwargs = dict(d=d, d_1=d - d_2, d_2=d_2, T=T, eta=0.05, kappa=0.5)
    elif kind == "LQGC":
        kwargs = dict(d=d, off_diag=0.05, T=T, seed=42, delta_t=dt)
    else:
        kwargs = dict(d=d, off_diag=0.3 / d ** 0.5, T=T, seed=42)
    solver = dict(loss_method=c["loss"], time_approx=c["tmode"], adaptive_forward_process=c["adaptive"], detach_forward=c["detach"],
                  early_stopping_time=None, L=1, lr=0.001, seed=42, delta_t=dt, K=c["K"], u_l2_error_flag=False)
    return dict(name="dblocks", family="solver", problem=dict(kind=kind, kwargs=kwargs), solver=solver)


def x0_of(c, X_0):
    """The case's X_0 (fp32, CPU) given the problem's own: a zero X_0 is replaced by x0 * cos(i)."""
    X_0 = torch.as_tensor(X_0, dtype=torch.float32).detach().cpu()
    if float(X_0.abs().max()) == 0.0 and c["x0"] != 0.0:
        return (c["x0"] * torch.cos(torch.arange(c["d"], dtype=torch.float32))).contiguous()
    return X_0


def net_specs(c):
    """[(d_in, seed)] of the case's nets: one per step for 'outer', one with the time input for 'inner'."""
    if c["tmode"] == "outer":
        return [(c["d"], 5 + n) for n in range(c["N"])]
    return [(c["d"] + 1, 5)]


def prepare_nets(c, nets):
    """Weight matrices x scale; biases N(0, bias_std) from ONE seeded CPU generator in parameter order (net by net) -- the same
    numbers whichever side (oracle on the CPU, package on the GPU) the nets live on."""
    gen = torch.Generator().manual_seed(BIAS_SEED)
    with torch.no_grad():
        for net in nets:
            for p in net.parameters():
                if p.dim() == 1:
                    p.copy_((torch.randn(p.shape, generator=gen) * c["bias_std"]).to(p.device))
                else:
                    p.mul_(c["scale"])


def scaled_oracle(c):
    """(OracleProblem with the case's X_0, HJBConfig, [DenseNetOracle] prepared)."""
    case = golden_style(c)
    oprob = orc.make_problem(case["problem"]["kind"], **case["problem"]["kwargs"])
    oprob.X_0 = x0_of(c, oprob.X_0)
    s = case["solver"]
    ocfg = orc.HJBConfig(K=s["K"], delta_t=s["delta_t"], lr=s["lr"], L=1, seed=s["seed"], loss_method=s["loss_method"],
                         time_approx=s["time_approx"], adaptive_forward_process=s["adaptive_forward_process"],
                         detach_forward=s["detach_forward"])
    nets = [orc.DenseNetOracle(d_in, c["d"], s["lr"], arch=[c["H"], c["H"]], seed=seed) for d_in, seed in net_specs(c)]
    prepare_nets(c, nets)
    return oprob, ocfg, nets


def host_noise(seed, K, d, N):
    """What noise='reference' draws in the first iteration with a fixed X_0 (solver.py:422, :381; hjb_train does the same)."""
    torch.manual_seed(seed)
    return torch.randn(K, d, N + 1)


def reference_key(c):
    return (c["tmode"], c["kind"], c["d"], c["H"], c["K"], c["N"], c["detach"], c["adaptive"], c["loss"], c["dt"], c["scale"],
            c["bias_std"], c["x0"], c["noise"])


_REFS = {}


def reference(c, noise, stream="host"):
    """ref64.iteration_dense of the case, computed once per (problem, shape, flags, noise mode) -- the matrix mode and the backward
    switch do not enter -- and never modified.  `noise`: a callable returning (K, d, N + 1), evaluated on a miss only.  `stream`
    names where a Philox stream was materialised ('host': oracle/philox_oracle.py in double; 'device': psp_philox_normal_fill, whose
    fp32 Box-Muller differs from it in the last bits), so that a process running the CPU and the GPU tests keeps the two apart."""
    key = reference_key(c) + ((stream,) if c["noise"] == "philox" else ())
    if key not in _REFS:
        oprob, ocfg, nets = scaled_oracle(c)
        _REFS[key] = ref64.iteration_dense(oprob, ocfg, nets, noise())
    return _REFS[key]
