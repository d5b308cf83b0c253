"""The case table of tests/test_gpu_solver_ul2.py (GPU) and tests/test_ref64_ul2.py (CPU): the control-ansatz Solver with
u_l2_error_flag=True, one list for both, in the layout of tests/block_cases.py (whose helpers build every case).

N = 3 or 4, dt = 0.05, L = 1, the weights scaled (block_cases.default_scale) so that Z is O(1) and the log depends on the net.  Every
case carries expect = (family, d_pad, H_pad) and `ukind`, the description of u* it exercises (tests/ref64_ul2.py): 'table' (LLGC,
accumulated inside the forward kernels), 'gains' (LQGC) and 'grid' (the double wells), both decoded from the path store.
"""
import torch

import block_cases as bc
import ref64
import ref64_ul2 as r64u
from util_cases import make_oracle, make_pkg_problem

UKIND = {"LLGC": "table", "LQGC": "gains", "DoubleWell": "grid", "DoubleWell_multidim": "grid"}
NX = 300                    # grid points of the double wells' u* tables (dx = 5 / 300)
V = lambda v: {"PSP_FWD_VARIANT": str(v)}


def _u(route, kind, d, H, K, N, mode, expect, noise, detach=True, adaptive=True, basis=None, plan_basis=None, **kw):
    """basis: Solver(state_basis=...) where the case asks for one; plan_basis: the basis the plan rolls out in ('x' unless stated)."""
    c = bc._c(route, kind, d, H, K, N, detach, mode, expect, noise=noise, **kw)
    c.update(ukind=UKIND[kind], adaptive=adaptive, basis=basis, plan_basis=plan_basis or basis or "x")
    c["id"] = "%s-%s%s%s" % (c["id"], noise[:3], "" if adaptive else "-nonadaptive", "-%s" % basis if basis else "")
    return c


def _table():
    out = []
    # the three narrow forwards x the two noise modes: hjb_fwd_kernel<.., MODE 0, FAST 0>, hjbs_fwd_kernel, hjbq_fwd_kernel (u_ref set:
    # no FAST instance), one and three hidden blocks, ragged K
    for d, H, K, exp in ((12, 16, 37, (1, 16, 16)), (20, 40, 72, (1, 32, 48))):
        for v in (1, 2, 3):
            for noise in ("reference", "philox"):
                out.append(_u("table-narrow-v%d" % v, "LLGC", d, H, K, 4, "fp32", exp, noise, env=V(v)))
    # D < 16: the feature mask inside ONE state block (exact d = 2; d = 7 padded to 8)
    for d, K, exp in ((2, 48, (1, 2, 30)), (7, 40, (1, 8, 30))):
        out.append(_u("table-small-d", "LLGC", d, 30, K, 4, "fp32", exp, "reference", env=V(1)))
        out.append(_u("table-small-d", "LLGC", d, 30, K, 4, "fp32", exp, "philox", env=V(3)))
    # the exact (100, 64) instance
    out.append(_u("table-100x64", "LLGC", 100, 64, 48, 3, "fp32", (1, 100, 64), "reference", env=V(1)))
    out.append(_u("table-100x64", "LLGC", 100, 64, 48, 3, "f16x3", (1, 100, 64), "reference"))
    # several tiles per wave and workgroup, ragged last tile (more than two tiles per CU: state_basis='auto' picks the sigma basis)
    out.append(_u("table-rounds", "LLGC", 20, 40, 9001, 4, "fp32", (1, 32, 48), "reference", env=V(1), plan_basis="sigma"))
    # MODE 2 / MODE 1 of hjb_fwd_kernel with FAST = 0 on BOTH noises (without u_ref, Philox noise launches FAST = 1)
    for mode in ("f16x3", "bf16"):
        for d, H, exp in ((20, 40, (1, 32, 48)), (40, 48, (1, 48, 48))):
            for noise in ("reference", "philox"):
                out.append(_u("table-%s" % mode, "LLGC", d, H, 72, 4, mode, exp, noise))
    # store_path 2 (attached), 3 (relative entropy), and the non-adaptive process
    out.append(_u("table-attached", "LLGC", 20, 40, 72, 4, "fp32", (1, 32, 48), "reference", detach=False, env=V(1)))
    out.append(_u("table-relent", "LLGC", 20, 40, 72, 4, "fp32", (1, 32, 48), "reference", detach=False, loss="relative_entropy",
                  env=V(1)))
    out.append(_u("table-nonadaptive", "LLGC", 20, 40, 72, 4, "fp32", (1, 32, 48), "philox", adaptive=False, env=V(1)))
    # the sigma basis: the kernels roll out X~ = B^-1 X, the table stays u*(t_n)
    out.append(_u("table-sigma-basis", "LLGC", 33, 16, 40, 4, "f16x3", (1, 48, 16), "reference", basis="sigma"))
    # hjbw_fwd_kernel<D, H, LOGU = true>: six instances (d = 500, H = 64 is compiled as an instance of its own, csrc/wide_instances.def,
    # so (512, 64) is reached from d = 505) x two matrix modes (f16x3: the SAME fp32 LOGU forward, then the split
    # backward) x two noises; d = 200 exact: the last state block is masked against a zero-padded table row
    for d, H, K, exp in ((120, 64, 48, (2, 128, 64)), (200, 64, 48, (2, 200, 64)), (250, 50, 48, (2, 256, 64)),
                         (320, 64, 48, (2, 320, 64)), (500, 64, 36, (2, 500, 64)), (505, 64, 36, (2, 512, 64))):
        for mode in ("fp32", "f16x3"):
            for noise in ("reference", "philox"):
                out.append(_u("table-wide-%s" % mode, "LLGC", d, H, K, 3, mode, exp, noise))
    out.append(_u("table-wide-rounds", "LLGC", 200, 64, 9001, 3, "fp32", (2, 200, 64), "philox"))
    return out


WIDE_INSTANCES = ((128, 64), (200, 64), (256, 64), (320, 64), (500, 64), (512, 64))


def _gains():
    out = []
    g = lambda route, d, H, K, mode, exp, noise, **kw: out.append(_u("gains-" + route, "LQGC", d, H, K, 4, mode, exp, noise, **kw))
    g("d2", 2, 30, 48, "fp32", (1, 2, 30), "philox")
    g("fp32", 20, 40, 72, "fp32", (1, 32, 48), "reference", env=V(1))
    g("f16x3", 20, 40, 72, "f16x3", (1, 32, 48), "philox")
    g("bf16", 20, 40, 72, "bf16", (1, 32, 48), "reference")
    g("48x32", 33, 17, 40, "fp32", (1, 48, 32), "philox", env=V(2))
    g("attached", 20, 40, 72, "fp32", (1, 32, 48), "reference", detach=False, env=V(1))
    g("relent", 20, 40, 72, "f16x3", (1, 32, 48), "philox", detach=False, loss="relative_entropy")
    out.append(_u("gains-store4", "LQGC", 20, 40, "cu", 3, "f16x3", (1, 32, 48), "philox", regen=True))
    for mode in ("fp32", "f16x3"):
        out.append(_u("gains-wide", "LQGC", 130, 40, 40, 3, mode, (2, 192, 64), "reference" if mode == "fp32" else "philox"))
    return out


def _grid():
    return [_u("grid-dw1d", "DoubleWell", 1, 30, 112, 4, "fp32", (1, 2, 30), "reference"),
            _u("grid-dw30", "DoubleWell_multidim", 30, 64, 50, 4, "fp32", (1, 32, 64), "philox", env=V(1))]


CASES = _table() + _gains() + _grid()
IDS = [c["id"] for c in CASES]
assert len(set(IDS)) == len(CASES)
BY_ID = {c["id"]: c for c in CASES}


def style(c, K):
    """block_cases.golden_style with the log switched on, the case's process, and the double wells' tables computed."""
    if c["kind"] == "DoubleWell":
        g = bc.golden_style(dict(c, kind="DoubleWell_multidim"), K)
        kw = g["problem"]["kwargs"]
        g["problem"] = dict(kind="DoubleWell", kwargs=dict(d=1, T=kw["T"], eta=kw["eta"], kappa=kw["kappa"]))
    else:
        g = bc.golden_style(c, K)
    g["solver"].update(u_l2_error_flag=True, adaptive_forward_process=c["adaptive"])
    if c["ukind"] == "grid":
        g["problem"]["calls"] = [["compute_reference_solution", {"nx": NX}]]
        if c["kind"] == "DoubleWell_multidim":
            g["problem"]["calls"].append(["compute_reference_solution_2", {"nx": NX}])
    return g


def solver_kwargs(c):
    return dict(state_basis=c["basis"]) if c["basis"] else {}


def scaled_oracle(c, K):
    """(OracleProblem, HJBConfig, TanhMLP with its weights x scale).  DoubleWell(d = 1) is restated as the multidimensional class
    with d_1 = 1, d_2 = 0: the same dynamics and costs, which tests/ref64.py knows."""
    g = style(c, K)
    if c["kind"] == "DoubleWell":
        kw = g["problem"]["kwargs"]
        g["problem"] = dict(kind="DoubleWell_multidim", kwargs=dict(d=1, d_1=1, d_2=0, T=kw["T"], eta=kw["eta"], kappa=kw["kappa"]))
    oprob, ocfg, omodels = make_oracle(g, L=1)
    with torch.no_grad():
        for p in omodels[0].parameters():
            p.mul_(c["scale"])
    return oprob, ocfg, omodels[0]


_PROBLEMS = {}


def pkg_problem(c):
    """The package problem of the case on the CPU (u_true, u_true_tables), built once."""
    key = (c["kind"], c["d"], c["N"], c["dt"])
    if key not in _PROBLEMS:
        _PROBLEMS[key] = make_pkg_problem(style(c, 16)["problem"], "cpu")
    return _PROBLEMS[key]


D_TOL = 2e-5                # tests/test_gpu_block_gradients.py; every case's GPU bound on ul2 must stay below it
_REFS = {}


def gpu_bound(e32):
    """The rule of tests/test_ref64_is.py: eight times the fp32 stand-in's own error against float64, plus 5e-7."""
    return 8.0 * e32 + 5e-7


def references(c, K, noise):
    """The float64 reference of the case on `noise` (a callable returning (K, d, N + 1), evaluated on a miss) and its fp32
    stand-in, computed once per (problem, shape, flags, noise mode) and never modified.  dict:
      r64, r32     ref64.iteration(..., want_path=True) in float64 / float32, each with `ul2` (K,) added
      desc         ref64_ul2.describe of the package problem
      E32          max_k |ul2_32 - ul2_64| / max(1, max_k ul2_64);  bound = gpu_bound(E32)
      delta, near  grid kind: 8 x (max state error of the stand-in) / dx, and near_k of the float64 run (else None, all false)"""
    key = bc.reference_key(c, K) + (c["adaptive"],)
    if key not in _REFS:
        oprob, ocfg, z = scaled_oracle(c, K)
        xi = noise()
        r64 = ref64.iteration(oprob, ocfg, z, xi, want_path=True)
        r32 = ref64.iteration(oprob, ocfg, z, xi, dtype=torch.float32, want_path=True)
        desc = r64u.describe(pkg_problem(c), c["N"], c["dt"])
        dt = float(torch.tensor(ocfg.delta_t))
        delta, near = None, torch.zeros(K, dtype=torch.bool)
        if desc["kind"] == "grid":
            delta = 8.0 * float((r32["X"].double() - r64["X"]).abs().max()) / desc["dx"]
            r64["ul2"], near = r64u.ul2(desc, r64["Z"], r64["X"], dt, delta=delta)
        else:
            r64["ul2"] = r64u.ul2(desc, r64["Z"], r64["X"], dt)
        r32["ul2"] = r64u.ul2(desc, r32["Z"], r32["X"], dt, dtype=torch.float32)
        keep = ~near
        e32 = float((r32["ul2"].double() - r64["ul2"]).abs()[keep].max()) / max(1.0, float(r64["ul2"].max()))
        _REFS[key] = dict(r64=r64, r32=r32, desc=desc, dt=dt, E32=e32, bound=gpu_bound(e32), delta=delta, near=near)
    return _REFS[key]


def bf16_model(c, K, noise):
    """ref64.iteration(operands='bf16', want_path=True) of the case with its `ul2`: the model the bf16 mode is judged against."""
    key = bc.reference_key(c, K) + (c["adaptive"], "bf16")
    if key not in _REFS:
        oprob, ocfg, z = scaled_oracle(c, K)
        r = ref64.iteration(oprob, ocfg, z, noise(), operands="bf16", want_path=True)
        r["ul2"] = r64u.ul2(r64u.describe(pkg_problem(c), c["N"], c["dt"]), r["Z"], r["X"], float(torch.tensor(ocfg.delta_t)))
        _REFS[key] = r
    return _REFS[key]
