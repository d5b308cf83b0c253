"""Case table and config builder of the per-trajectory tests of psp_is_rollout (csrc/hjbe_kernels.h hjbe_rollout_kernel): shared
by tests/test_ref64_is.py (CPU) and tests/test_gpu_is_kernel.py (GPU).

Synthetic coefficients from seeded numpy generators, rounded to fp32: A = -0.5 I + 0.5 randn / sqrt(d), B = 0.5 I + 0.7 randn /
sqrt(d), gains 0.5 randn / sqrt(d), a TABLE control 0.5 randn, diagonal drift in [-1.2, -0.8], kappa in [0.25, 0.5], running and
terminal vectors in [0.5, 1.5] (the LINEAR terminal vector with both signs), x0 in [-1, 1], dt in [0.01, 0.05], N <= 12, K <= 300.

GRID: G tables of (nrows, ncols) entries 0.5 randn on cells of width dx = 0.25 over [-xb, xb), xb = 2; xhi = xb - 2.5 dx, so that a
state clamped to xhi sits in the middle of a cell; u_row = (3 n + 2) mod nrows is not monotone.  At this dx an fp32 state resolves
the cell of the float64 state except within ref64_is.NEAR_WINDOW of an edge: about 2e-4 d N of the trajectories, hence N <= 4 in
the 32 / 64 buckets.  Three cases carry the edges: 'row_oob' (u_row entries below 0 and >= nrows: kernel and reference clamp),
'x0_low' (x0[0] = -xb - 1: clamped for every step, the last trajectory's cell 0 - 2 wraps to ncols - 2) and 'x0_high'
(x0[1] = 2.5 > xhi).
"""
import ctypes as C

import numpy as np
import torch

import ref64_is as r64
from util_cases import psp

nat = psp.native
assert (r64.DRIFT_ZERO, r64.DRIFT_DENSE, r64.DRIFT_DIAG, r64.DRIFT_DWELL) == (nat.DRIFT_ZERO, nat.DRIFT_DENSE, nat.DRIFT_DIAG,
                                                                              nat.DRIFT_DOUBLE_WELL)
assert (r64.SIGMA_IDENTITY, r64.SIGMA_DENSE, r64.SIGMA_SCALED) == (nat.SIGMA_IDENTITY, nat.SIGMA_DENSE, nat.SIGMA_SCALED_IDENTITY)
assert (r64.RUN_ZERO, r64.RUN_DIAGQ) == (nat.RUNCOST_ZERO, nat.RUNCOST_DIAG_QUAD)
assert (r64.TERM_LINEAR, r64.TERM_DIAGQ, r64.TERM_SHIFTED) == (nat.TERM_LINEAR, nat.TERM_DIAG_QUAD, nat.TERM_SHIFTED_QUAD)
assert (r64.ISC_NONE, r64.ISC_TABLE, r64.ISC_LINEAR, r64.ISC_GRID) == (nat.ISC_NONE, nat.ISC_TABLE, nat.ISC_LINEAR, nat.ISC_GRID)

BUCKETS = (1, 4, 16, 32, 64)
CTRL_NAMES = {r64.ISC_NONE: "NONE", r64.ISC_TABLE: "TABLE", r64.ISC_LINEAR: "LINEAR", r64.ISC_GRID: "GRID"}
GRID_XB, GRID_DX, GRID_NROWS = 2.0, 0.25, 5
PHILOX_SEED, PHILOX_ITER, PHILOX_OFFSET = (7 << 32) | 12345, 9, 12345


def bucket(d):
    return 1 if d <= 1 else 4 if d <= 4 else 16 if d <= 16 else 32 if d <= 32 else 64


def f32(v):
    """The fp32 value the kernel gets for a Python float."""
    return float(np.float32(v))


# drift: 'zero' | 'dense' | 'diag' | 'dwell0' | 'dwell1' (the digit is dwell_form); sigma: 'I' | 'dense' | 'sI'
_DRIFT = {"zero": r64.DRIFT_ZERO, "dense": r64.DRIFT_DENSE, "diag": r64.DRIFT_DIAG, "dwell0": r64.DRIFT_DWELL, "dwell1": r64.DRIFT_DWELL}
_SIGMA = {"I": r64.SIGMA_IDENTITY, "dense": r64.SIGMA_DENSE, "sI": r64.SIGMA_SCALED}
_RUN = {"zero": r64.RUN_ZERO, "diagq": r64.RUN_DIAGQ}
_TERM = {"lin": r64.TERM_LINEAR, "diagq": r64.TERM_DIAGQ, "shift": r64.TERM_SHIFTED}
N_, T_, L_, G_ = r64.ISC_NONE, r64.ISC_TABLE, r64.ISC_LINEAR, r64.ISC_GRID


def _case(id, d, K, N, dt, ctrl, drift, sigma, run, term, scale=1.0, tables=2, edge=None):
    return dict(id=id, d=d, K=K, N=N, dt=dt, ctrl=ctrl, drift=drift, sigma=sigma, run=run, term=term, scale=scale, tables=tables,
                edge=edge)


CASES = [
    # ---- bucket 1
    _case("b1_none", 1, 37, 12, 0.02, N_, "dwell1", "I", "zero", "shift"),
    _case("b1_table", 1, 1, 8, 0.05, T_, "zero", "sI", "diagq", "lin", scale=0.7),
    _case("b1_linear", 1, 256, 6, 0.03, L_, "dense", "dense", "diagq", "diagq"),
    _case("b1_grid", 1, 300, 12, 0.02, G_, "dwell1", "I", "zero", "shift"),
    # ---- bucket 4
    _case("b4_none_d3", 3, 257, 5, 0.04, N_, "diag", "I", "diagq", "diagq"),
    _case("b4_table_d2", 2, 37, 10, 0.03, T_, "diag", "dense", "diagq", "lin"),
    _case("b4_linear_d4", 4, 257, 7, 0.02, L_, "dense", "sI", "diagq", "diagq", scale=1.3),
    _case("b4_grid_d4", 4, 256, 10, 0.02, G_, "dwell0", "I", "zero", "shift"),
    _case("b4_grid_d2_x0_low", 2, 300, 6, 0.02, G_, "zero", "sI", "diagq", "diagq", scale=0.7, edge="x0_low"),
    # ---- bucket 16
    _case("b16_none_d9", 9, 64, 6, 0.05, N_, "dense", "I", "zero", "lin"),
    _case("b16_table_d5", 5, 257, 6, 0.03, T_, "zero", "dense", "diagq", "shift"),
    _case("b16_linear_d16", 16, 37, 5, 0.04, L_, "diag", "sI", "diagq", "diagq", scale=0.7),
    _case("b16_grid_d16_row_oob", 16, 257, 6, 0.02, G_, "diag", "I", "diagq", "lin", tables=3, edge="row_oob"),
    _case("b16_grid_d5_x0_high", 5, 130, 8, 0.02, G_, "dwell0", "sI", "zero", "shift", scale=0.8, edge="x0_high"),
    # ---- bucket 32
    _case("b32_none_d20", 20, 100, 5, 0.02, N_, "dwell1", "dense", "zero", "shift"),
    _case("b32_table_d32", 32, 257, 4, 0.02, T_, "dwell0", "dense", "zero", "shift"),
    _case("b32_linear_d17", 17, 300, 5, 0.03, L_, "dense", "dense", "diagq", "diagq"),
    _case("b32_grid_d17", 17, 257, 4, 0.01, G_, "dwell1", "sI", "zero", "shift", scale=0.8),
    _case("b32_grid_d32", 32, 37, 3, 0.02, G_, "zero", "I", "diagq", "lin", tables=3),
    # ---- bucket 64
    _case("b64_none_d40", 40, 257, 4, 0.03, N_, "diag", "sI", "diagq", "lin", scale=1.2),
    _case("b64_table_d33", 33, 37, 4, 0.05, T_, "diag", "I", "diagq", "diagq"),
    _case("b64_linear_d64", 64, 300, 4, 0.02, L_, "dense", "dense", "diagq", "lin"),
    _case("b64_grid_d64", 64, 257, 3, 0.02, G_, "dwell0", "I", "zero", "shift"),
    _case("b64_grid_d33", 33, 256, 4, 0.01, G_, "zero", "sI", "zero", "diagq", scale=0.7),
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]
assert len(BY_ID) == len(CASES)
GRID_IDS = [c["id"] for c in CASES if c["ctrl"] == G_]
# (c) Philox against supplied mode: per bucket, d at the low edge and at the full width, run at K = 257
PHILOX_IDS = ["b1_grid", "b4_table_d2", "b4_linear_d4", "b16_table_d5", "b16_linear_d16", "b32_linear_d17", "b32_table_d32",
              "b64_table_d33", "b64_linear_d64"]
# (d) sharding at K_global = 300: (k_offset 0, K_local 130) + (k_offset 130, K_local 170) against one call
SHARD_IDS = ["b4_grid_d4", "b32_linear_d17"]
SHARD_K, SHARD_SPLIT = 300, 130
# (e) buffer edges
EDGE_IDS = ["b1_table", "b4_table_d2", "b16_grid_d16_row_oob"]          # K = 1, 37, 257


def route(c):
    """The name a case's errors are collected under: bucket / control kind."""
    return "%d/%s" % (bucket(c["d"]), CTRL_NAMES[c["ctrl"]])


def bit_exact(c):
    """The cases csrc/hjbe_kernels.h promises to round op by op: elementwise drift and sigma, no product in the control."""
    return c["drift"] != "dense" and c["sigma"] != "dense" and c["ctrl"] != L_


def case_seed(c):
    return 1000 + IDS.index(c["id"])


def host_noise(c, K):
    """Supplied noise (N + 1, K, d) fp32; slice 0, which no step reads, is NaN."""
    rng = np.random.default_rng(5000 + case_seed(c))
    xi = rng.standard_normal((c["N"] + 1, K, c["d"])).astype(np.float32)
    xi[0] = np.nan
    return xi


def describe(c, K=None, K_global=None, k_offset=0, noise=None):
    """The ref64_is description of one call of case `c` (K trajectories of K_global from k_offset on; `noise` (N + 1, K, d) or
    the case's own host noise).  The coefficients depend on the case alone, not on K / K_global / k_offset."""
    d, N = c["d"], c["N"]
    K = c["K"] if K is None else K
    rng = np.random.default_rng(case_seed(c))
    f4 = np.float32
    rs = 1.0 / np.sqrt(d)
    A = (-0.5 * np.eye(d) + 0.5 * rs * rng.standard_normal((d, d))).astype(f4)
    B = (0.5 * np.eye(d) + 0.7 * rs * rng.standard_normal((d, d))).astype(f4)
    diag = rng.uniform(-1.2, -0.8, d).astype(f4)
    kappa = rng.uniform(0.25, 0.5, d).astype(f4)
    p = rng.uniform(0.5, 1.5, d).astype(f4)
    tq = rng.uniform(0.5, 1.5, d).astype(f4)
    tl = (rng.uniform(0.5, 1.5, d) * rng.choice([-1.0, 1.0], d)).astype(f4)
    x0 = rng.uniform(-1.0, 1.0, d).astype(f4)
    table = (0.5 * rng.standard_normal((N, d))).astype(f4)
    gains = (0.5 * rs * rng.standard_normal((N, d, d))).astype(f4)
    G = c["tables"]
    ncols = int(round(2 * GRID_XB / GRID_DX))
    tables = (0.5 * rng.standard_normal((G, GRID_NROWS, ncols))).astype(f4)
    group = ((np.arange(d) + 1) % G).astype(np.int32)
    row = ((3 * np.arange(N) + 2) % GRID_NROWS).astype(np.int32)
    if c["edge"] == "row_oob":
        row[1], row[N - 1] = -3, GRID_NROWS + 2
    elif c["edge"] == "x0_low":
        x0[0] = -GRID_XB - 1.0
    elif c["edge"] == "x0_high":
        x0[1] = 2.5
    drift = {"zero": None, "dense": A, "diag": diag, "dwell0": kappa, "dwell1": kappa}[c["drift"]]
    desc = dict(id=c["id"], d=d, K_local=K, K_global=K if K_global is None else K_global, k_offset=k_offset, N=N,
                dt=f32(c["dt"]), sqrt_dt=f32(np.sqrt(c["dt"])),
                drift_kind=_DRIFT[c["drift"]], sigma_kind=_SIGMA[c["sigma"]], runcost_kind=_RUN[c["run"]], term_kind=_TERM[c["term"]],
                dwell_form=1 if c["drift"] == "dwell1" else 0, sigma_scale=f32(c["scale"]),
                drift=drift, sigma=B if c["sigma"] == "dense" else None, runcost=p if c["run"] == "diagq" else None,
                term=tl if c["term"] == "lin" else tq, control_kind=c["ctrl"], x0=x0,
                noise=host_noise(c, K) if noise is None else np.asarray(noise, dtype=f4))
    if c["ctrl"] == T_:
        desc["table"] = table
    elif c["ctrl"] == L_:
        desc["gains"] = gains
    elif c["ctrl"] == G_:
        desc.update(tables=tables, group=group, row=row, xb=f32(GRID_XB), dx=f32(GRID_DX), xhi=f32(GRID_XB - 2.5 * GRID_DX),
                    nrows=GRID_NROWS, ncols=ncols)
    assert desc["noise"].shape == (N + 1, K, d), desc["noise"].shape
    return desc


def device_config(desc, device, noise_mode=None):
    """(nat.IsConfig, the tensors it points to) of a description on `device` ('cpu' serves psp_is_query, which reads no pointer).
    The noise is not part of the config: psp_is_rollout takes it as an argument."""
    keep = []

    def dev_t(a, dtype=torch.float32):
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype).contiguous()
        keep.append(t)
        return nat.ptr(t)

    cfg = nat.IsConfig()
    cfg.d, cfg.K_local, cfg.N, cfg.control_kind = desc["d"], desc["K_local"], desc["N"], desc["control_kind"]
    cfg.K_global, cfg.k_offset = desc["K_global"], desc["k_offset"]
    cfg.dt, cfg.sqrt_dt, cfg.sigma_scale = desc["dt"], desc["sqrt_dt"], desc["sigma_scale"]
    cfg.drift_kind, cfg.sigma_kind = desc["drift_kind"], desc["sigma_kind"]
    cfg.runcost_kind, cfg.term_kind, cfg.dwell_form = desc["runcost_kind"], desc["term_kind"], desc["dwell_form"]
    cfg.noise_mode = nat.NOISE_SUPPLIED if noise_mode is None else noise_mode
    cfg.x0, cfg.drift, cfg.sigma = dev_t(desc["x0"]), dev_t(desc["drift"]), dev_t(desc["sigma"])
    cfg.runcost, cfg.term = dev_t(desc["runcost"]), dev_t(desc["term"])
    kind = desc["control_kind"]
    if kind == nat.ISC_TABLE:
        cfg.u_ref = dev_t(desc["table"])
    elif kind == nat.ISC_LINEAR:
        cfg.u_ref = dev_t(desc["gains"])
    elif kind == nat.ISC_GRID:
        cfg.u_ref = dev_t(desc["tables"])
        cfg.u_group, cfg.u_row = dev_t(desc["group"], torch.int32), dev_t(desc["row"], torch.int32)
        cfg.u_ntables, cfg.u_nrows, cfg.u_ncols = desc["tables"].shape
        cfg.u_xb, cfg.u_dx, cfg.u_xhi = desc["xb"], desc["dx"], desc["xhi"]
    return cfg, keep


def query(cfg):
    """None if psp_is_query accepts the config, else the library's reason."""
    if nat.load().psp_is_query(C.byref(cfg), None) != 0:
        return nat.last_error()
    return None


_REF = {}


def reference(c):
    """(desc, logw64, XN64, keep, E32_w, E32_x, logw32, XN32) of a case at its own K on its host noise, computed once and shared
    (treat as read-only).  keep: the trajectories that count (GRID: not `near`); E32: rollout32 against rollout64 on them."""
    if c["id"] not in _REF:
        _REF[c["id"]] = evaluate(describe(c))
    return _REF[c["id"]]


def evaluate(desc):
    out = r64.rollout64(desc)
    logw64, XN64 = out[0], out[1]
    keep = ~out[2] if desc["control_kind"] == r64.ISC_GRID else np.ones(desc["K_local"], dtype=bool)
    logw32, XN32 = r64.rollout32(desc)
    ew, ex = r64.errors(logw32, XN32, logw64, XN64, keep)
    return desc, logw64, XN64, keep, ew, ex, logw32, XN32


def bounds(ew32, ex32):
    """The GPU bounds of a case: 8 x the float32 recursion's own error (the kernel's sequential fma chains against numpy's order
    in the dense products) + 5e-7 (four fp32 ulps at the normalising scale, where the float32 recursion happens to be exact)."""
    return 8.0 * ew32 + 5e-7, 8.0 * ex32 + 5e-7
