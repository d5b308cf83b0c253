"""Case table, input builder and checks of the float64 differential tests of the linear-control kernels (csrc/aff_kernels.h):
shared by tests/test_ref64_affine.py (CPU) and tests/test_gpu_affine_kernels.py (GPU).

Inputs: seeded generators, rounded to fp32, zero padded to the d bucket on the way to the device (pad).  M_n = 0.3 randn / sqrt(d),
c_n = 0.3 randn; X_0[i] = 0.5 cos(i) (1.0 cos(i) for the double well: both wells), plus 0.3 randn per trajectory where the case
has x0_stride = d -- with X_0 = 0, dM_0 would be identically zero; A = -I + 0.3 randn / sqrt(d), B = I + 0.3 randn / sqrt(d);
diagonal drift in [-1.2, -0.8], kappa in [0.5, 1], running and terminal vectors in [0.5, 1.5]; weights w, mu, nu, wT = randn / K
(both signs); u_L2 references 0.3 randn (TABLE) and 0.3 randn / sqrt(d) (LINEAR).

The shapes are the smallest at which each path of make_aff_plan / the kernels can still go wrong; K_big = 64 CUs + 17 is the first
K with 256-thread workgroups and 17 valid lanes in the last one (CUs from the device, 256 -- the library's fallback -- without one).
"""
import ctypes as C
import math

import torch

import ref64_affine as r64
from affine_cases import cus, k_big
from util_cases import psp

nat = psp.native
assert (r64.DRIFT_ZERO, r64.DRIFT_DENSE, r64.DRIFT_DIAG, r64.DRIFT_DWELL) == (nat.DRIFT_ZERO, nat.DRIFT_DENSE, nat.DRIFT_DIAG,
                                                                              nat.DRIFT_DOUBLE_WELL)
assert (r64.SIGMA_IDENTITY, r64.SIGMA_DENSE, r64.SIGMA_SCALED) == (nat.SIGMA_IDENTITY, nat.SIGMA_DENSE, nat.SIGMA_SCALED_IDENTITY)
assert (r64.RUN_ZERO, r64.RUN_DIAGQ) == (nat.RUNCOST_ZERO, nat.RUNCOST_DIAG_QUAD)
assert (r64.TERM_LINEAR, r64.TERM_DIAGQ, r64.TERM_SHIFTED) == (nat.TERM_LINEAR, nat.TERM_DIAG_QUAD, nat.TERM_SHIFTED_QUAD)
assert (r64.UL2_TABLE, r64.UL2_LINEAR) == (nat.UL2_TABLE, nat.UL2_LINEAR)

D_TOL = 2e-5                 # per-trajectory quantities: |diff| <= D_TOL max(1, max |ref|)   (the project's D bound)
BLOCK_TOL = 2e-4             # dM_n, dc_n, dL/dZ_n: of the block's own maximum, per step          (the project's per-block bound)
PHILOX_SEED, PHILOX_ITER = 42, 3


def f32(v):
    """The fp32 value the kernels get for a Python float."""
    return float(torch.tensor(v, dtype=torch.float32))


def bucket(d):
    return 16 if d <= 16 else 32 if d <= 32 else 64


def _case(id, d, K, N, control, drift, sigma, run, term, paths, threads=64, dt=0.05, adaptive=True, scale=1.0, x0_rows=False,
          ul2=None, explicit_wT=False, noise="supplied", multi_stage=False, lds_bytes=None, seed=0):
    return dict(seed=seed, id=id, d=d, K=K, N=N, control=control, drift=drift, sigma=sigma, run=run, term=term, paths=paths, threads=threads,
                dt=dt, adaptive=adaptive, scale=scale, x0_rows=x0_rows, ul2=ul2, explicit_wT=explicit_wT, noise=noise,
                multi_stage=multi_stage, lds_bytes=lds_bytes)


R = r64
BIG = ("big", 0)
CASES = [
    # seed: three trajectories and 200 steps leave the regime (tests/test_ref64_affine.py) to the draw; these draws are in it
    _case("d1", 1, 3, 2, "Affine", R.DRIFT_ZERO, R.SIGMA_IDENTITY, R.RUN_ZERO, R.TERM_LINEAR, (1,), seed=1),
    _case("d16_diag_scaled", 16, 65, 3, "Affine", R.DRIFT_DIAG, R.SIGMA_SCALED, R.RUN_DIAGQ, R.TERM_DIAGQ, (1,), scale=0.7,
          ul2=R.UL2_TABLE),
    _case("d17_denseA_identB", 17, 64, 2, "Linear", R.DRIFT_DENSE, R.SIGMA_IDENTITY, R.RUN_DIAGQ, R.TERM_DIAGQ, (2,),
          explicit_wT=True, ul2=R.UL2_LINEAR),
    _case("d32_dwell_denseB", 32, 97, 4, "Affine", R.DRIFT_DWELL, R.SIGMA_DENSE, R.RUN_ZERO, R.TERM_SHIFTED, (2,), x0_rows=True),
    _case("d33_relent", 33, 130, 3, "Affine", R.DRIFT_DENSE, R.SIGMA_DENSE, R.RUN_DIAGQ, R.TERM_DIAGQ, (3,)),
    _case("d49_philox", 49, 80, 3, "Linear", R.DRIFT_DIAG, R.SIGMA_SCALED, R.RUN_DIAGQ, R.TERM_LINEAR, (1, 2), scale=1.2,
          noise="philox"),
    _case("d5_long", 5, 300, 200, "Constant", R.DRIFT_DIAG, R.SIGMA_IDENTITY, R.RUN_ZERO, R.TERM_LINEAR, (1,), dt=0.002,
          adaptive=False, multi_stage=True, seed=3),
    _case("d64_big_detached", 64, ("big", 47), 3, "Affine", R.DRIFT_DENSE, R.SIGMA_DENSE, R.RUN_ZERO, R.TERM_LINEAR, (1,),
          threads=256, ul2=R.UL2_LINEAR, multi_stage=True, lds_bytes=132096),
    _case("d64_big_attached", 64, ("big", 47), 3, "Affine", R.DRIFT_DENSE, R.SIGMA_DENSE, R.RUN_DIAGQ, R.TERM_DIAGQ, (2,),
          threads=256, multi_stage=True),
    _case("d5_big_relent", 5, BIG, 2, "Linear", R.DRIFT_DIAG, R.SIGMA_SCALED, R.RUN_DIAGQ, R.TERM_DIAGQ, (3,), threads=256,
          scale=0.7, x0_rows=True, ul2=R.UL2_TABLE, multi_stage=True),
    _case("d20_big_const", 20, BIG, 1, "Constant", R.DRIFT_DENSE, R.SIGMA_DENSE, R.RUN_ZERO, R.TERM_LINEAR, (1,), threads=256,
          adaptive=False, multi_stage=True),
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]
RUNS = [(c["id"], sp) for c in CASES for sp in c["paths"]]            # one kernel run per (case, store_path)


def K_of(c):
    return c["K"] if isinstance(c["K"], int) else k_big() + c["K"][1]


def route(c, sp):
    """The name a case's errors are collected under: bucket / workgroup / drift x sigma / store_path."""
    dn = {R.DRIFT_ZERO: "A0", R.DRIFT_DENSE: "Adense", R.DRIFT_DIAG: "Adiag", R.DRIFT_DWELL: "Adwell"}[c["drift"]]
    sn = {R.SIGMA_IDENTITY: "BI", R.SIGMA_DENSE: "Bdense", R.SIGMA_SCALED: "BsI"}[c["sigma"]]
    return "%d/T%d/%s-%s/%s/sp%d%s%s" % (bucket(c["d"]), c["threads"], dn, sn, c["control"], sp, "" if c["adaptive"] else "-nonadaptive",
                                         "-philox" if c["noise"] == "philox" else "")


def build_inputs(c, xi=None):
    """The fp32 inputs of a case, unpadded, on the CPU.  xi: the materialised Philox stream of a Philox case."""
    d, K, N = c["d"], K_of(c), c["N"]
    g = torch.Generator().manual_seed(1000 + 16 * IDS.index(c["id"]) + c["seed"])
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    rd = math.sqrt(d)
    inp = dict(d=d, K=K, N=N)
    inp["dt"], inp["sqdt"] = f32(c["dt"]), float(torch.sqrt(torch.tensor(c["dt"], dtype=torch.float32)))
    inp["M"] = 0.3 * rn(N, d, d) / rd if c["control"] != "Constant" else None
    inp["c"] = 0.3 * rn(N, d) if c["control"] != "Linear" else None
    x0 = (1.0 if c["drift"] == R.DRIFT_DWELL else 0.5) * torch.cos(torch.arange(d, dtype=torch.float32))
    inp["x0"] = (x0 + 0.3 * rn(K, d)) if c["x0_rows"] else x0
    inp["drift"] = {R.DRIFT_ZERO: None, R.DRIFT_DENSE: -torch.eye(d) + 0.3 * rn(d, d) / rd, R.DRIFT_DIAG: -(0.8 + 0.4 * ru(d)),
                    R.DRIFT_DWELL: 0.5 + 0.5 * ru(d)}[c["drift"]]
    inp["sigma"] = torch.eye(d) + 0.3 * rn(d, d) / rd if c["sigma"] == R.SIGMA_DENSE else None
    inp["run"] = 0.5 + ru(d) if c["run"] == R.RUN_DIAGQ else None
    inp["term"] = 0.5 + ru(d)
    inp["ul2"] = None if c["ul2"] is None else 0.3 * rn(N, d) if c["ul2"] == R.UL2_TABLE else 0.3 * rn(N, d, d) / rd
    for name in ("w", "mu", "nu", "wT"):
        inp[name] = rn(K) / K
    inp["xi"] = rn(N + 1, K, d) if xi is None else xi
    assert (c["noise"] == "philox") == (xi is not None) and inp["xi"].shape == (N + 1, K, d)
    return inp


def reference(c, inp, sp, dtype=torch.float64, **kw):
    """The statement of ref64_affine.py for one store_path of the case."""
    attached = sp in (2, 3)
    loss = dict(w=inp["w"]) if sp == 1 else dict(mu=inp["mu"], wT=inp["wT"] if c["explicit_wT"] else None) if sp == 2 else \
        dict(nu=inp["nu"])
    return r64.statement(inp["d"], inp["K"], inp["N"], inp["dt"], inp["sqdt"], inp["M"], inp["c"], (c["drift"], inp["drift"]),
                         (c["sigma"], inp["sigma"]), (c["run"], inp["run"]), (c["term"], inp["term"]), f32(c["scale"]), c["adaptive"],
                         attached, inp["x0"], inp["xi"], relent=sp == 3, ul2=None if c["ul2"] is None else (c["ul2"], inp["ul2"]),
                         dtype=dtype, **loss, **kw)


def image_of(c, inp, ref, sp):
    """What the forward leaves in the image half of the path store (aff_kernels.h): (N, K, d)."""
    xi, Z = inp["xi"][1:].to(ref["Z"].dtype), ref["Z"]
    if sp == 3:
        return Z
    if sp == 2:
        return xi - inp["sqdt"] * Z
    return xi if c["adaptive"] else xi + inp["sqdt"] * Z


def expected_forward(c, inp, ref, sp):
    """The forward kernel's outputs in float64, under the names check_forward compares."""
    out = dict(D=ref["D"], Y=-ref["Zsum"] if sp == 3 else ref["Y"], XN=ref["XN"], X=ref["X"][:-1], image=image_of(c, inp, ref, sp))
    if ref["ul2"] is not None:
        out["ul2"] = ref["ul2"]
    return out


def kernel_like(c, inp, ref, sp):
    """The float64 numbers in the layout the GPU driver returns them (fp32, padded to the bucket): what the planted errors of
    tests/test_ref64_affine.py start from."""
    DB = bucket(c["d"])
    exp = expected_forward(c, inp, ref, sp)
    got = {k: pad(v.float(), DB) if v.dim() > 1 else v.float() for k, v in exp.items()}
    got["dZ"] = ref["dZ"].float()
    got["dM"] = None if ref["dM"] is None else ref["dM"].float()
    got["dc"] = None if ref["dc"] is None else ref["dc"].float()
    return got


def pad(t, DB, square=False):
    """Zero pads the last dimension (square: the last two) to the bucket."""
    if t is None:
        return None
    n = DB - t.shape[-1]
    return torch.nn.functional.pad(t, (0, n, 0, n) if square else (0, n)).contiguous()


def make_config(c, sp, dev_ptrs=None, k_offset=0, K_global=None, ul2_out=None, noise=None):
    """psp_aff_config of a case.  dev_ptrs: name -> padded device tensor (None: a config for psp_aff_query only, whose pointers are
    never dereferenced)."""
    cfg = nat.AffConfig()
    cfg.struct_bytes = C.sizeof(nat.AffConfig)
    b, K = cfg.base, K_of(c)
    b.d, b.H, b.K_local, b.N = bucket(c["d"]), 0, K, c["N"]
    b.k_offset, b.K_global = k_offset, K + k_offset if K_global is None else K_global
    b.dt, b.sqrt_dt = f32(c["dt"]), float(torch.sqrt(torch.tensor(c["dt"], dtype=torch.float32)))
    b.drift_kind, b.sigma_kind, b.sigma_scale, b.runcost_kind, b.term_kind = c["drift"], c["sigma"], c["scale"], c["run"], c["term"]
    b.adaptive, b.store_path, b.mlp_dtype = int(c["adaptive"]), sp, nat.MLP_FP32
    b.loss_kind = nat.LOSS_REL_ENTROPY if sp == 3 else nat.LOSS_WEIGHTS
    b.noise_mode = nat.NOISE_PHILOX if (c["noise"] if noise is None else noise) == "philox" else nat.NOISE_SUPPLIED
    cfg.d_real, cfg.has_matrix, cfg.has_bias = c["d"], int(c["control"] != "Constant"), int(c["control"] != "Linear")
    if c["ul2"] is not None:
        cfg.ul2_kind = c["ul2"]
        b.u_l2_out, cfg.ul2_ref = (8, 8) if dev_ptrs is None else (ul2_out.data_ptr(), dev_ptrs["ul2"].data_ptr())
    if dev_ptrs is not None:
        for name, field in (("drift", "drift"), ("sigma", "sigma"), ("run", "runcost"), ("term", "term")):
            t = dev_ptrs.get(name)
            setattr(b, field, None if t is None else t.data_ptr())
    return cfg


def query(cfg):
    sizes = nat.AffSizes()
    nat.check(nat.load().psp_aff_query(C.byref(cfg), C.byref(sizes)), "psp_aff_query")
    return sizes


def slice_len_of(c, sizes):
    """Trajectories per gradient slice.  psp_aff_sizes names the slice count only, so this restates make_aff_plan (about two rounds
    of workgroups over the chip, slices of whole 32-trajectory stages) and is held to the count the library reports."""
    K, N = K_of(c), c["N"]
    stages = -(-K // 32)
    S = max(1, min((2 * cus() + N // 2) // N, stages))
    slice_len = -(-stages // S) * 32
    assert -(-K // slice_len) == sizes.slices, (c["id"], slice_len, sizes.slices, "make_aff_plan slices differently: restate it here")
    return slice_len


def assert_route(c, sizes):
    """The launch shape the case was built for: a planner change cannot empty a route in silence.  Returns a line for the printout."""
    K, slice_len = K_of(c), slice_len_of(c, sizes)
    assert sizes.fwd_threads == c["threads"], (c["id"], sizes.fwd_threads)
    assert sizes.fwd_workgroups == -(-K // c["threads"])
    if c["multi_stage"]:
        assert sizes.slices * 32 < K and slice_len > 32, (c["id"], sizes.slices, K)      # a slice spans several LDS stages
        assert sizes.slices > 1
    else:
        assert slice_len == 32, (c["id"], slice_len)
    if c["lds_bytes"] is not None:
        assert sizes.lds_bytes == c["lds_bytes"], sizes.lds_bytes
    return "%s: K %d  threads %d x %d workgroups (last: %d lanes)  slices %d of <= %d (last: %d)  slices * 32 %s K  lds %d bytes" % (
        c["id"], K, sizes.fwd_threads, sizes.fwd_workgroups, K - (sizes.fwd_workgroups - 1) * sizes.fwd_threads, sizes.slices,
        slice_len, K - (sizes.slices - 1) * slice_len, "<" if sizes.slices * 32 < K else ">=", sizes.lds_bytes)


def ragged_last_slice(c, sizes):
    return K_of(c) % slice_len_of(c, sizes) != 0


# ---- the checks (shared by the GPU test and the planted errors of the CPU test) ------------------------------------------------
def _abs_err(got, ref):
    return float((got.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def forward_errors(got, exp, d):
    """name -> error of D, Y, XN, ul2, X (path rows) and image against float64, in units of max(1, max |ref|)."""
    return {k: _abs_err(got[k][..., :d] if got[k].dim() > 1 else got[k], v) for k, v in exp.items()}


def check_forward(got, exp, d, tag=""):
    """Every forward output finite, its padded columns exactly zero, and within D_TOL of float64.  Returns the errors."""
    for k, v in exp.items():
        want = v.shape if v.dim() == 1 else v.shape[:-1] + (bucket(d),)
        assert got[k].shape == want, (tag, k, got[k].shape, want)
        assert bool(torch.isfinite(got[k]).all()), (tag, k, "NaN or inf: an element nobody wrote")
        if v.dim() > 1:
            assert not bool(got[k][..., d:].any()), (tag, k, "padded columns are not exactly zero")
    errs = forward_errors(got, exp, d)
    bad = {k: e for k, e in errs.items() if not e <= D_TOL}
    assert not bad, (tag, "forward", bad, D_TOL)
    return errs


def check_partials(fwd_partial, D, threads, tag=""):
    """Per workgroup (sum D, sum D^2) = the float64 sums of the kernel's own fp32 D over the workgroup's lanes in lane order: the
    first bit for bit, the second within 1e-12 (v * v may be contracted into the add)."""
    K = D.numel()
    grid = -(-K // threads)
    assert fwd_partial.shape == (grid, 2) and bool(torch.isfinite(fwd_partial).all()), (tag, fwd_partial.shape)
    lanes = torch.zeros(grid * threads, dtype=torch.float64)
    lanes[:K] = D.double().cpu()
    lanes = lanes.view(grid, threads).numpy()
    s1 = torch.from_numpy(lanes.cumsum(axis=1)[:, -1].copy())
    s2 = torch.from_numpy((lanes * lanes).cumsum(axis=1)[:, -1].copy())
    p = fwd_partial.cpu()
    wrong = (p[:, 0] != s1).nonzero().flatten().tolist()
    assert not wrong, (tag, "sum D of workgroups", wrong[:8], "differs from the lane-order sum")
    rel = float(((p[:, 1] - s2).abs() / s2.abs().clamp_min(1e-300)).max())
    assert rel <= 1e-12, (tag, "sum D^2", rel)
    return p.sum(0)


def step_errors(got, ref):
    """Per step: max |got - ref| over the step / max |ref| over the step."""
    N = ref.shape[0]
    g, r = got.double().reshape(N, -1), ref.reshape(N, -1)
    return [float((g[n] - r[n]).abs().max()) / max(float(r[n].abs().max()), 1e-300) for n in range(N)]


def check_sweep(image_after, sqdt, dZ, tag=""):
    """The image slot the sweep leaves, times sqrt(dt), against dL/dZ_n: per step within BLOCK_TOL of that step's maximum."""
    errs = step_errors(image_after.double() * sqdt, dZ)
    assert all(e <= BLOCK_TOL for e in errs), (tag, "sweep", errs, BLOCK_TOL)
    return max(errs)


def check_gradient(dM, dc, ref, tag=""):
    """dM_n and dc_n SEPARATELY, each per step within BLOCK_TOL of its own maximum.  Returns (worst error, its block)."""
    worst = (0.0, "-")
    for name, got, want in (("dM", dM, ref["dM"]), ("dc", dc, ref["dc"])):
        assert (got is None) == (want is None), (tag, name)
        if want is None:
            continue
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), (tag, name, got.shape)
        errs = step_errors(got, want)
        assert all(e <= BLOCK_TOL for e in errs), (tag, name, errs, BLOCK_TOL)
        worst = max(worst, (max(errs), "%s_%d" % (name, errs.index(max(errs)))))
    return worst


def regime(ref):
    """(smallest block maximum / the larger block of its step, smallest step maximum / the gradient's maximum)."""
    blocks = [b for b in (ref["dM"], ref["dc"]) if b is not None]
    N = blocks[0].shape[0]
    per = [[float(b[n].abs().max()) for b in blocks] for n in range(N)]
    gmax = max(max(p) for p in per)
    return min(min(p) / max(p) for p in per), min(max(p) for p in per) / gmax
