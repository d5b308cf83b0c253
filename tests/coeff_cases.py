"""Coefficient sets with DISTINCT per-coordinate entries, and the case table of tests/test_gpu_coeff_vectors.py (GPU) and
tests/test_ref64_coeff.py (CPU).

Every stock problem hands the kernels constant coefficient vectors (LLGC: alpha = 1, A = -I; LQGC: P = I / 2, R = I; the double
well: two constants; X_0 = 0 or -1), so a kernel that reads entry rowmap(i), a neighbouring lane's entry or entry 0 for every
coordinate computes the same numbers.  Here each vector is vec(d, lo, hi, phase)[i] = lo + (hi - lo) frac(i / golden ratio +
phase): injective for d <= 512, without a period of 4, 16 or 64, neighbours 0.38 or 0.62 of the range apart.  A set is applied to
the package problem (attributes, assigned after construction: the catalogue METHODS stay, so the native plan is kept) and to the
OracleProblem (extra[...], .B, .X_0 -- all that tests/ref64.py reads) with the same fp32 tensors.

  set            problem              what varies                                                   kinds (drift x sigma x run x term)
  llgc_diag_sI   LLGC                 A = diag(-a), B = 0.8 I, alpha (sign flipped on i % 3 == 2), X_0   DIAG x SCALED_IDENTITY x - x LINEAR
  llgc_dense     LLGC, stock A, B     alpha, X_0                                                    DENSE x DENSE x - x LINEAR
  lqgc_dense     LQGC, stock A, B     P = diag(p), R = diag(r), X_0                                 DENSE x DENSE x DIAG_QUAD x DIAG_QUAD
  lqgc_diag_I    LQGC, off_diag = 0   A = diag(-a), B = I, P, R, X_0                                DIAG x IDENTITY x DIAG_QUAD x DIAG_QUAD
  dwell          DoubleWell_multidim  kappa_, eta_, X_0                                             DOUBLE_WELL x IDENTITY x - x SHIFTED_QUAD

tests/test_ref64_coeff.py asserts on the float64 reference that each of three planted mis-reads of each vector of each case
(PLANTED below) moves D, and in attached cases a gradient block, by at least ten times the GPU test's bound.
"""
import torch

import block_cases as bc
import dense_block_cases as dc
import ref64
from util_cases import make_oracle, orc, psp

nat = psp.native
GOLDEN = 0.6180339887498949

# (lo, hi, phase): a phase per vector, so that no two vectors of a set are images of each other
RANGES = dict(a=(0.6, 1.4, 0.43), alpha=(0.5, 1.5, 0.29), p=(0.25, 0.75, 0.57), r=(0.5, 1.5, 0.71), kappa=(0.3, 0.7, 0.83),
              eta=(0.03, 0.09, 0.97))
X0_RANGES = {"LLGC": (-0.6, 0.6, 0.11), "LQGC": (-0.6, 0.6, 0.11), "DoubleWell_multidim": (-1.3, -0.7, 0.11)}
SIGMA_SCALE = 0.8

# set -> (problem kind, varied vectors, off_diag forced to zero, (drift, sigma, runcost, term) kinds)
SETS = {
    "llgc_diag_sI": ("LLGC", ("a", "alpha", "X_0"), True, (nat.DRIFT_DIAG, nat.SIGMA_SCALED_IDENTITY, nat.RUNCOST_ZERO, nat.TERM_LINEAR)),
    "llgc_dense": ("LLGC", ("alpha", "X_0"), False, (nat.DRIFT_DENSE, nat.SIGMA_DENSE, nat.RUNCOST_ZERO, nat.TERM_LINEAR)),
    "lqgc_dense": ("LQGC", ("p", "r", "X_0"), False, (nat.DRIFT_DENSE, nat.SIGMA_DENSE, nat.RUNCOST_DIAG_QUAD, nat.TERM_DIAG_QUAD)),
    "lqgc_diag_I": ("LQGC", ("a", "p", "r", "X_0"), True, (nat.DRIFT_DIAG, nat.SIGMA_IDENTITY, nat.RUNCOST_DIAG_QUAD, nat.TERM_DIAG_QUAD)),
    "dwell": ("DoubleWell_multidim", ("kappa", "eta", "X_0"), False,
              (nat.DRIFT_DOUBLE_WELL, nat.SIGMA_IDENTITY, nat.RUNCOST_ZERO, nat.TERM_SHIFTED_QUAD)),
}
PLANTED = ("swap12", "perm4", "entry0")


def vec(d, lo, hi, phase):
    i = torch.arange(d, dtype=torch.float64)
    return (lo + (hi - lo) * torch.frac(i * GOLDEN + phase)).float()


def vectors(cset, d):
    """name -> (d,) fp32 CPU tensor, for every varied vector of the set."""
    kind, names = SETS[cset][:2]
    out = {}
    for n in names:
        v = vec(d, *(X0_RANGES[kind] if n == "X_0" else RANGES[n]))
        if n == "alpha":
            v[2::3] *= -1.0                                      # mixed signs: g(x) = alpha . x is not a plain sum either
        out[n] = v
    return out


def plant(v, which):
    """The vector a mis-indexed read would see: entries 1 and 2 exchanged; the in-block permutation i -> 4 (i & 3) + (i >> 2) of the
    T layout's 16-feature blocks (an entry whose image lies past d stays); entry 0 for every coordinate."""
    d = v.numel()
    i = torch.arange(d)
    if which == "swap12":
        src = i.clone()
        src[1], src[2] = 2, 1
    elif which == "perm4":
        j = i & 15
        src = (i - j) + 4 * (j & 3) + (j >> 2)
        src = torch.where(src < d, src, i)
    else:
        assert which == "entry0"
        src = torch.zeros_like(i)
    return v[src].clone()


def case_vectors(c, planted=None):
    """The case's vectors; planted = (name, which): that one vector as the mis-read would see it."""
    vs = vectors(c["cset"], c["d"])
    if planted is not None:
        vs[planted[0]] = plant(vs[planted[0]], planted[1])
    return vs


def _tensors(cset, d, vs):
    """attribute name (package side) -> fp32 CPU tensor."""
    out = {}
    if "a" in vs:
        out["A"] = torch.diag(-vs["a"])
        out["B"] = (SIGMA_SCALE if cset == "llgc_diag_sI" else 1.0) * torch.eye(d)
    if "alpha" in vs:
        out["alpha"] = vs["alpha"].reshape(d, 1).clone()
    if "p" in vs:
        out["P"], out["R"] = torch.diag(vs["p"]), torch.diag(vs["r"])
    if "kappa" in vs:
        out["kappa_"], out["eta_"] = vs["kappa"].clone(), vs["eta"].clone()
    out["X_0"] = vs["X_0"].clone()
    return out


def apply_to_package(cset, prob, vs, device):
    """Before the Solver is built: it copies X_0."""
    for name, t in _tensors(cset, prob.d, vs).items():
        assert hasattr(prob, name), name
        setattr(prob, name, t.to(device))
    return prob


def apply_to_oracle(cset, oprob, vs):
    for name, t in _tensors(cset, oprob.d, vs).items():
        if name in ("B", "X_0"):
            setattr(oprob, name, t)
        else:
            assert name in oprob.extra, name
            oprob.extra[name] = t
    return oprob


def assert_kinds(c, cfg):
    """On the plan's psp_hjb_config: a set that silently lands on another kind fails instead of passing.  Under
    state_basis='sigma' the kernels are handed identity sigma (plan_native.py)."""
    drift, sigma, run, term = SETS[c["cset"]][3]
    if c.get("basis") == "sigma":
        sigma = nat.SIGMA_IDENTITY
    got = (int(cfg.drift_kind), int(cfg.sigma_kind), int(cfg.runcost_kind), int(cfg.term_kind))
    assert got == (drift, sigma, run, term), (c["id"], got)
    if sigma == nat.SIGMA_SCALED_IDENTITY:
        assert float(cfg.sigma_scale) == float(torch.tensor(SIGMA_SCALE)), float(cfg.sigma_scale)


# ---- the tanh-MLP families ---------------------------------------------------------------------------------------------------------
def _t(cset, route, d, H, K, N, detach, mode, expect, basis=None, coop=None, **kw):
    """block_cases._c of the set's problem kind, plus the set, the state basis asked of the Solver (None: the default) and the
    cooperative forward's tiles per workgroup (None: not that kernel; 0: asserted NOT to run)."""
    c = bc._c(route, SETS[cset][0], d, H, K, N, detach, mode, expect, **kw)
    c.update(cset=cset, basis=basis, coop=coop, family="tanh")
    c["id"] = "%s-%s%s%s" % (c["id"], cset, "-basis_%s" % basis if basis else "", "-philox" if c["noise"] == "philox" else "")
    return c


def _tanh_cases():
    out = []
    V = lambda v: {"PSP_FWD_VARIANT": str(v)}
    every = tuple(SETS)
    three = ("llgc_diag_sI", "lqgc_dense", "dwell")
    # narrow padded: d = 20, H = 40 -> (32, 48); two state blocks, the second with 4 real features; every forward of the family,
    # detached (hjb_bwd2 / hjb_bwd3) and attached (hjb_adj_kernel; hjbq_adj_kernel behind variant 3)
    for cset in every:
        for detach in (True, False):
            for v in (1, 2, 3):
                out.append(_t(cset, "narrow-fp32-v%d" % v, 20, 40, 72, 4, detach, "fp32", (1, 32, 48), env=V(v)))
            out.append(_t(cset, "narrow-f16x3", 20, 40, 72, 4, detach, "f16x3", (1, 32, 48)))
    # narrow exact (100, 64): seven state blocks, the last with 4 features
    for cset in three:
        for detach in (True, False):
            out.append(_t(cset, "narrow-fp32-v1", 100, 64, 48, 3, detach, "fp32", (1, 100, 64), env=V(1)))
            out.append(_t(cset, "narrow-f16x3", 100, 64, 48, 3, detach, "f16x3", (1, 100, 64)))
    # on-device noise: the FAST general instance of hjb_fwd_kernel (a running cost, element-wise drifts)
    for cset in ("lqgc_dense", "llgc_diag_sI", "dwell"):
        for detach in (True, False):
            out.append(_t(cset, "narrow-philox", 20, 40, 72, 4, detach, "fp32", (1, 32, 48), noise="philox", env=V(1)))
            out.append(_t(cset, "narrow-philox", 20, 40, 72, 4, detach, "f16x3", (1, 32, 48), noise="philox"))
    # the state basis: under 'sigma' the kernels get B^T alpha and B^-1 x0 (and, f16x3 on Philox noise, the specialised instances)
    for basis in ("sigma", "x"):
        out.append(_t("llgc_dense", "narrow-basis", 20, 40, 72, 4, True, "fp32", (1, 32, 48), basis=basis, env=V(1)))
        out.append(_t("llgc_dense", "narrow-basis", 20, 40, 72, 4, True, "f16x3", (1, 32, 48), basis=basis))
        out.append(_t("llgc_dense", "narrow-basis", 20, 40, 72, 4, True, "f16x3", (1, 32, 48), basis=basis, noise="philox"))
    # relative entropy (store_path 3) and the variance loss (generic trajectory weights), attached
    for mode in ("fp32", "f16x3"):
        env = V(1) if mode == "fp32" else None
        out.append(_t("lqgc_dense", "narrow-relent", 20, 40, 72, 4, False, mode, (1, 32, 48), loss="relative_entropy", env=env))
        out.append(_t("lqgc_dense", "narrow-variance", 20, 40, 72, 4, False, mode, (1, 32, 48), loss="variance", env=env))
    # wide: padded d = 120 -> (128, 64), exact 200 (12.5 blocks), d = 250 / H = 50 -> (256, 64); both matrix modes, hjbw_adj_kernel
    # (N = 4 at d = 200: exchanging two entries of P moves a gradient block by 9.8 x BLOCK_TOL at N = 3, by 16 x at N = 4;
    #  the double well at d = 250 takes x 7 where block_cases.default_scale's x 10 saturates the first layer: median |h1| 0.88)
    for d, H, N, exp, sets in ((120, 64, 3, (2, 128, 64), ("llgc_diag_sI", "dwell")), (200, 64, 4, (2, 200, 64), ("lqgc_dense", "llgc_diag_sI")),
                               (250, 50, 3, (2, 256, 64), ("lqgc_dense", "dwell"))):
        for cset in sets:
            scale = 7.0 if (cset, d) == ("dwell", 250) else None
            for detach in (True, False):
                for mode in ("fp32", "f16x3"):
                    out.append(_t(cset, "wide-%s" % mode, d, H, 48, N, detach, mode, exp, scale=scale))
    # the cooperative forward (hjbc_fwd_kernel: on-device noise, f16x3): d = 200 (odd block count, a padding block), 320 (idle
    # waves), 500 (every wave owns blocks, the last with 4 features); two and four tiles per workgroup
    for d, K, sets in ((200, 48, ("llgc_diag_sI", "dwell")), (320, 40, ("llgc_diag_sI",)), (500, 36, ("llgc_diag_sI",))):
        for cset in sets:
            for coop in (2, 4):
                out.append(_t(cset, "wide-coop%d" % coop, d, 64, K, 3, True, "f16x3", (2, d, 64), noise="philox", coop=coop,
                              env={"PSP_FWD_COOP": str(coop)}))
    # ... which make_plan keeps away from a running cost
    out.append(_t("lqgc_dense", "wide-runcost-philox", 200, 64, 48, 4, True, "f16x3", (2, 200, 64), noise="philox", coop=0,
                  env={"PSP_FWD_COOP": "2"}))
    return out


TANH_CASES = _tanh_cases()
assert len({c["id"] for c in TANH_CASES}) == len(TANH_CASES)


def golden_style(c, K):
    case = bc.golden_style(c, K)
    if SETS[c["cset"]][2]:
        case["problem"]["kwargs"]["off_diag"] = 0.0
    return case


def scaled_oracle(c, K, planted=None):
    """(OracleProblem with the set applied, HJBConfig, TanhMLP with its weights x scale)."""
    oprob, ocfg, omodels = make_oracle(golden_style(c, K), L=1)
    apply_to_oracle(c["cset"], oprob, case_vectors(c, planted))
    with torch.no_grad():
        for p in omodels[0].parameters():
            p.mul_(c["scale"])
    return oprob, ocfg, omodels[0]


def reference_key(c, K):
    if c["family"] == "tanh":
        return ("tanh", c["cset"]) + bc.reference_key(c, K)
    return ("dense", c["cset"]) + dc.reference_key(c)


_REFS = {}


def reference(c, K, noise, dtype=torch.float64, planted=None, stream="host"):
    """ref64.iteration / iteration_dense of the case, computed once per (set, problem, shape, flags, noise mode, planted error)
    and never modified.  noise: a callable returning (K, d, N + 1), evaluated on a miss only; stream: where a Philox stream was
    materialised (dense_block_cases.reference); dtype: float32 gives the stand-in of a correct fp32 kernel (tanh nets only)."""
    key = reference_key(c, K) + (dtype, planted, stream if c["noise"] == "philox" else "")
    if key not in _REFS:
        if c["family"] == "tanh":
            oprob, ocfg, z = scaled_oracle(c, K, planted)
            _REFS[key] = ref64.iteration(oprob, ocfg, z, noise(), dtype=dtype)
        else:
            assert dtype == torch.float64
            oprob, ocfg, nets = dense_oracle(c, planted)
            _REFS[key] = ref64.iteration_dense(oprob, ocfg, nets, noise())
    return _REFS[key]


# ---- the DenseNet-control family (hjbd_fwd_kernel / hjbd_adj_kernel, kinds 0 - 3) ---------------------------------------------------------
def _d(cset, tmode, d, H, K, N, detach, mode, expect, **kw):
    c = dc._c(tmode, SETS[cset][0], d, H, K, N, detach, mode, expect, "kernel1", **kw)
    c.update(cset=cset, basis=None, coop=None, family="dense")
    if c["noise"] == "philox":                                   # (no set here has the dense drift and sigma of the SPEC forward)
        c.update(spec=False, route=c["route"].replace("/spec/", "/f16x3/") + "-philox")
    c["id"] = "%s-%s" % (c["id"], cset)
    return c


def _dense_cases():
    out = []
    shapes = (("lqgc_dense", "inner", 20, 40, 72, 4, (32, 64)), ("lqgc_diag_I", "inner", 20, 40, 72, 4, (32, 64)),
              ("llgc_diag_sI", "outer", 100, 30, 48, 3, (112, 32)), ("dwell", "inner", 65, 30, 50, 4, (112, 32)))
    for cset, tmode, d, H, K, N, exp in shapes:
        for detach in (True, False):
            for mode in ("fp32", "f16x3"):
                out.append(_d(cset, tmode, d, H, K, N, detach, mode, exp))
        out.append(_d(cset, tmode, d, H, K, N, True, "f16x3", exp, noise="philox"))
    return out


DENSE_CASES = _dense_cases()
assert len({c["id"] for c in DENSE_CASES}) == len(DENSE_CASES)


def dense_golden_style(c):
    case = dc.golden_style(c)
    if SETS[c["cset"]][2]:
        case["problem"]["kwargs"]["off_diag"] = 0.0
    return case


def dense_oracle(c, planted=None):
    """dense_block_cases.scaled_oracle with the set in place of its X_0 = x0 cos(i)."""
    case = dense_golden_style(c)
    oprob = orc.make_problem(case["problem"]["kind"], **case["problem"]["kwargs"])
    apply_to_oracle(c["cset"], oprob, case_vectors(c, planted))
    s = case["solver"]
    ocfg = orc.HJBConfig(K=s["K"], delta_t=s["delta_t"], lr=s["lr"], L=1, seed=s["seed"], loss_method=s["loss_method"],
                         time_approx=s["time_approx"], adaptive_forward_process=s["adaptive_forward_process"],
                         detach_forward=s["detach_forward"])
    nets = [orc.DenseNetOracle(d_in, c["d"], s["lr"], arch=[c["H"], c["H"]], seed=seed) for d_in, seed in dc.net_specs(c)]
    dc.prepare_nets(c, nets)
    return oprob, ocfg, nets


CASES = TANH_CASES + DENSE_CASES


def distinct(cases):
    """One case per float64 reference (the matrix mode, the kernel switches and the state basis do not enter it)."""
    seen, out = set(), []
    for c in cases:
        k = reference_key(c, c["K"])
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out
