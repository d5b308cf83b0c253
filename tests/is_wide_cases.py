"""Case table of the per-trajectory tests of psp_isw_rollout (csrc/hjbew_kernels.h isw_rollout_kernel): shared by
tests/test_ref64_is_wide.py (CPU) and tests/test_gpu_is_wide_kernel.py (GPU).  Built on tests/is_kernel_cases.py (describe,
evaluate, bounds, device_config: the synthetic coefficients, the float64 reference and the bound rule are those of the narrow
kernel's tests) and on tests/ref64_is.py as they are.

d sits where the tile layout can go wrong: 65 (a fifth 16-feature block holding one feature), 80 (five full blocks), 100, 130
(the 12-block bucket), 200 and 256 (the 16-block bucket, ragged and full: PSP_ISW_MAX_D = 256, so 257 and 500 do not exist), and
16 / 48 for the cross-check with psp_is_rollout.  K in {1, 17, 37, 257}: a lone trajectory, a ragged second tile, a ragged third
tile, a partial last workgroup (four tiles each).  N <= 4; the GRID cases keep d N <= 400, since about 2e-4 d N of their
trajectories are `near` a cell edge (ref64_is.NEAR_WINDOW) and the cap on that share is 10 %.
"""
import ctypes as C

import numpy as np

import is_kernel_cases as ikc
import ref64_is as r64
from util_cases import psp

nat = psp.native
N_, T_, L_, G_ = r64.ISC_NONE, r64.ISC_TABLE, r64.ISC_LINEAR, r64.ISC_GRID
_case = ikc._case

CASES = [
    # ---- d = 65: every control kind
    _case("w65_none", 65, 257, 4, 0.03, N_, "diag", "I", "diagq", "lin"),
    _case("w65_table", 65, 1, 4, 0.05, T_, "zero", "sI", "diagq", "diagq", scale=0.7),
    _case("w65_linear", 65, 257, 3, 0.02, L_, "dense", "dense", "diagq", "diagq"),
    _case("w65_grid_row_oob", 65, 257, 4, 0.02, G_, "dwell0", "I", "zero", "shift", tables=3, edge="row_oob"),
    # ---- d = 80
    _case("w80_none", 80, 17, 4, 0.02, N_, "dwell1", "dense", "zero", "shift"),
    _case("w80_table", 80, 257, 3, 0.03, T_, "diag", "dense", "diagq", "lin"),
    _case("w80_grid_x0_low", 80, 37, 3, 0.02, G_, "zero", "I", "diagq", "diagq", edge="x0_low"),
    # ---- d = 100
    _case("w100_linear", 100, 37, 3, 0.02, L_, "dense", "sI", "diagq", "lin", scale=1.3),
    _case("w100_grid_x0_high", 100, 257, 3, 0.01, G_, "dwell1", "sI", "zero", "shift", scale=0.8, edge="x0_high"),
    # ---- d = 130
    _case("w130_none", 130, 257, 3, 0.02, N_, "dense", "I", "zero", "lin"),
    _case("w130_table", 130, 17, 4, 0.02, T_, "dwell0", "dense", "zero", "shift"),
    _case("w130_grid", 130, 257, 3, 0.01, G_, "diag", "sI", "diagq", "lin", scale=0.7),
    _case("w130_linear", 130, 17, 2, 0.03, L_, "diag", "I", "diagq", "diagq"),
    # ---- d = 200, 256: the 16-block bucket
    _case("w200_none", 200, 37, 3, 0.02, N_, "dense", "dense", "diagq", "lin"),
    _case("w200_linear", 200, 37, 2, 0.02, L_, "zero", "dense", "diagq", "diagq"),
    _case("w200_grid", 200, 257, 2, 0.02, G_, "dwell0", "sI", "zero", "shift", scale=0.8),
    _case("w256_table", 256, 257, 2, 0.02, T_, "dwell1", "I", "zero", "shift"),
    _case("w256_linear", 256, 17, 2, 0.02, L_, "dense", "dense", "diagq", "lin"),
    # ---- d = 16, 48: both kernels take them
    _case("w16_none", 16, 17, 4, 0.04, N_, "zero", "sI", "diagq", "lin", scale=1.2),
    _case("w16_grid", 16, 257, 4, 0.02, G_, "diag", "I", "diagq", "lin", tables=3),
    _case("w48_table", 48, 37, 4, 0.03, T_, "dwell0", "sI", "zero", "shift", scale=0.9),
    _case("w48_linear", 48, 257, 3, 0.02, L_, "dense", "dense", "diagq", "diagq"),
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]
assert len(BY_ID) == len(CASES)
GRID_IDS = [c["id"] for c in CASES if c["ctrl"] == G_]
NARROW_IDS = [c["id"] for c in CASES if c["d"] <= nat.IS_MAX_D]
# (d) Philox against supplied mode at K = 257: d = 65 and the largest case
PHILOX_IDS = ["w65_grid_row_oob", "w256_linear"]
# (e) sharding at K_global = 300: (0, 130) + (130, 170); the GRID case's last trajectory sits in the second call
SHARD_IDS = ["w65_grid_row_oob", "w100_linear"]
# (f) buffer edges at K = 1, 17, 257
EDGE_IDS = ["w65_table", "w80_none", "w65_grid_row_oob"]


def blocks(d):
    """16-feature blocks of the compiled bucket (csrc/hjbew_kernels.h isw_bucket)."""
    nb = (d + 15) // 16
    return 4 if nb <= 4 else 8 if nb <= 8 else 12 if nb <= 12 else 16


def table_bytes(desc):
    """psp_isw_sizes.table_bytes as DESIGN.md states it: P = 64 ceil(d / 64) padded features, five vectors, A and B when dense,
    then N rows (TABLE) or N matrices (LINEAR)."""
    P = 64 * ((desc["d"] + 63) // 64)
    floats = 5 * P + (P * P if desc["drift_kind"] == r64.DRIFT_DENSE else 0) + (P * P if desc["sigma_kind"] == r64.SIGMA_DENSE else 0)
    floats += desc["N"] * {T_: P, L_: P * P}.get(desc["control_kind"], 0)
    return 4 * floats


def route(c):
    """The name a case's errors are collected under: d / control kind."""
    return "%d/%s" % (c["d"], ikc.CTRL_NAMES[c["ctrl"]])


bit_exact = ikc.bit_exact


def case_seed(c):
    return 3000 + IDS.index(c["id"])


def describe(c, **kw):
    """is_kernel_cases.describe of a case of THIS table (its generator seeds come from this table's order)."""
    saved = ikc.case_seed
    ikc.case_seed = case_seed
    try:
        return ikc.describe(c, **kw)
    finally:
        ikc.case_seed = saved


_REF = {}


def reference(c):
    """is_kernel_cases.evaluate of the case at its own K on its host noise, computed once and shared (read-only):
    (desc, logw64, XN64, keep, E32_w, E32_x, logw32, XN32)."""
    if c["id"] not in _REF:
        _REF[c["id"]] = ikc.evaluate(describe(c))
    return _REF[c["id"]]


def sizes(cfg):
    """(nat.IswSizes, None) if psp_isw_query accepts the config, else (None, the library's reason)."""
    s = nat.IswSizes()
    rc = nat.load().psp_isw_query(C.byref(cfg), C.byref(s))
    return (s, None) if rc == 0 else (None, nat.last_error())
