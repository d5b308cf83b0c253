"""The case table of psp_isw_rollout's GPU tests (tests/is_wide_cases.py) against the float64 reference, psp_isw_query and the
``wide_states`` keyword of utilities.do_importance_sampling_me, checked without a GPU and without the kernel:

* the float32 recursion against rollout64 on every case: E32_w, E32_x <= 1e-4 (the error scale the GPU bounds are built from);
* the share of `near` trajectories of every GRID case <= 10 % (the cap of tests/test_ref64_is.py), the last global trajectory
  never among them; the coverage the table promises;
* psp_isw_query: every refusal with its message, table_bytes against DESIGN.md's formula, struct_bytes, the accepted d range;
  psp_is_query keeps refusing d = 70 with -2;
* the keyword: default 'torch', ValueError on other values, and on a CPU model 'native' raises "not on a GPU" with
  backend='native' and returns the composite result with backend='auto'.
"""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import is_kernel_cases as ikc
import is_wide_cases as wc
import ref64_is as r64
from util_cases import psp

nat = psp.native
NEAR_CAP = 0.10


@pytest.fixture(scope="module")
def lib():
    if not nat.is_built():
        import __graft_entry__
        __graft_entry__.build()
    return nat.load()


# ---- the case table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", wc.IDS)
def test_float32_recursion_is_well_conditioned(cid):
    c = wc.BY_ID[cid]
    desc, logw64, XN64, keep, ew, ex, logw32, XN32 = wc.reference(c)
    print("%s %s: E32_w %.2e  E32_x %.2e  max |logw| %.3g  max |XN| %.3g  kept %d / %d"
          % (cid, wc.route(c), ew, ex, np.abs(logw64).max(), np.abs(XN64).max(), keep.sum(), keep.size))
    assert np.all(np.isfinite(logw64)) and np.all(np.isfinite(XN64))
    assert ew <= 1e-4 and ex <= 1e-4, (ew, ex)
    bw, bx = ikc.bounds(ew, ex)
    assert bw <= 1e-3 and bx <= 1e-3


@pytest.mark.parametrize("cid", wc.GRID_IDS)
def test_near_share_of_the_grid_cases(cid):
    c = wc.BY_ID[cid]
    desc, logw64, XN64, keep = wc.reference(c)[:4]
    share = 1.0 - keep.mean()
    print("%s: near share %.4f (2e-4 d N = %.4f)" % (cid, share, 2e-4 * c["d"] * c["N"]))
    assert share <= NEAR_CAP
    assert r64.last_local(desc) == c["K"] - 1 and keep[c["K"] - 1], "the last global trajectory must count"
    assert c["d"] * c["N"] <= 400


def test_case_table_coverage():
    kinds = {nat.ISC_NONE, nat.ISC_TABLE, nat.ISC_LINEAR, nat.ISC_GRID}
    assert {c["ctrl"] for c in wc.CASES if c["d"] == 65} == kinds
    assert {c["ctrl"] for c in wc.CASES if c["d"] > 65} == kinds
    assert {c["d"] for c in wc.CASES} == {16, 48, 65, 80, 100, 130, 200, 256}
    assert max(c["d"] for c in wc.CASES) == nat.ISW_MAX_D
    assert {wc.blocks(c["d"]) for c in wc.CASES} == {4, 8, 12, 16}
    assert {(wc.blocks(c["d"]), c["ctrl"]) for c in wc.CASES} == {(b, k) for b in (4, 8, 12, 16) for k in kinds}
    assert {c["K"] for c in wc.CASES} == {1, 17, 37, 257} and all(1 <= c["N"] <= 4 for c in wc.CASES)
    pairs = {(c["drift"], c["sigma"]) for c in wc.CASES}
    assert pairs >= {(a, b) for a in ("zero", "dense", "diag", "dwell0", "dwell1") for b in ("I", "dense", "sI")}
    assert {c["run"] for c in wc.CASES} == {"zero", "diagq"} and {c["term"] for c in wc.CASES} == {"lin", "diagq", "shift"}
    assert {c["edge"] for c in wc.CASES if c["ctrl"] == nat.ISC_GRID} >= {"row_oob", "x0_low", "x0_high"}
    exact = [c for c in wc.CASES if wc.bit_exact(c)]
    assert {c["ctrl"] for c in exact} == {nat.ISC_NONE, nat.ISC_TABLE, nat.ISC_GRID} and {wc.blocks(c["d"]) for c in exact} == {4, 8, 12, 16}
    assert [wc.BY_ID[i]["K"] for i in wc.EDGE_IDS] == [1, 17, 257]
    assert [wc.BY_ID[i]["d"] for i in wc.PHILOX_IDS] == [65, nat.ISW_MAX_D]
    assert wc.BY_ID[wc.SHARD_IDS[0]]["ctrl"] == nat.ISC_GRID
    assert sorted(wc.BY_ID[i]["d"] for i in wc.NARROW_IDS) == [16, 16, 48, 48]
    for c in wc.CASES:                                                    # the edges reach the description
        desc = wc.describe(c)
        if c["edge"] == "row_oob":
            assert np.any(desc["row"] < 0) and np.any(desc["row"] >= desc["nrows"])
        if c["edge"] == "x0_low":
            assert desc["x0"][0] <= -desc["xb"]
        if c["edge"] == "x0_high":
            assert desc["x0"][1] > desc["xhi"]
    a, b = wc.describe(wc.CASES[0]), wc.describe(wc.CASES[0])            # (and the narrow table's seeds are left alone)
    assert np.array_equal(a["x0"], b["x0"]) and ikc.case_seed(ikc.CASES[0]) == 1000


# ---- psp_isw_query -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", wc.IDS)
def test_every_config_is_accepted_with_the_documented_sizes(lib, cid):
    c = wc.BY_ID[cid]
    desc = wc.describe(c)
    cfg, keep = ikc.device_config(desc, torch.device("cpu"))
    s, why = wc.sizes(cfg)
    assert why is None, (cid, why)
    assert s.struct_bytes == C.sizeof(nat.IswSizes) == 24 and s.max_d == nat.ISW_MAX_D == 256
    assert s.table_bytes == wc.table_bytes(desc), (cid, s.table_bytes, wc.table_bytes(desc))
    assert s.workgroups == -(-(-(-c["K"] // 16)) // 4)
    assert s.lds_bytes == (4 * desc["tables"].shape[0] * desc["ncols"] if c["ctrl"] == nat.ISC_GRID else 0)


def _plain(d):
    keep = (C.c_float * 8)()
    cfg = nat.IsConfig()
    cfg.d, cfg.K_local, cfg.N, cfg.K_global = d, 100, 3, 100
    cfg.x0 = cfg.term = C.cast(keep, C.c_void_p)
    return cfg, keep


def test_isw_query_accepts_the_whole_range(lib):
    for d in (1, 64, 65, nat.ISW_MAX_D):
        cfg, keep = _plain(d)
        s, why = wc.sizes(cfg)
        assert why is None, (d, why)
        assert s.table_bytes == 4 * 5 * 64 * ((d + 63) // 64) and s.workgroups == 2 and s.lds_bytes == 0
    cfg, keep = _plain(nat.ISW_MAX_D + 1)
    s = nat.IswSizes()
    assert lib.psp_isw_query(C.byref(cfg), C.byref(s)) == -2
    assert "d = 257 is outside the native range d <= 256" in nat.last_error()
    assert lib.psp_isw_rollout(C.byref(cfg), None, 1, 0, None, None, None, None) == -2


def test_isw_query_refusals(lib):
    def refused(cfg, sizes=None):
        s = nat.IswSizes() if sizes is None else sizes
        return lib.psp_isw_query(C.byref(cfg), C.byref(s)), nat.last_error()

    cfg, keep = _plain(100)
    ptr = C.cast(keep, C.c_void_p)
    bad = nat.IswSizes()
    bad.struct_bytes = 16
    rc, msg = refused(cfg, bad)
    assert rc == -1 and "struct_bytes = 16" in msg and "24 bytes" in msg
    assert lib.psp_isw_query(C.byref(cfg), None) == -1 and "null sizes" in nat.last_error()
    assert lib.psp_isw_query(None, C.byref(nat.IswSizes())) == -1 and "null config" in nat.last_error()
    cfg.d = 0
    assert refused(cfg) == (-1, "non-positive d / K / N")
    cfg.d, cfg.control_kind = 100, 9
    rc, msg = refused(cfg)
    assert rc == -1 and "control_kind out of range" in msg
    cfg.control_kind, cfg.drift_kind = nat.ISC_NONE, 7
    assert refused(cfg) == (-1, "config enum out of range")
    cfg.drift_kind, cfg.noise_mode = nat.DRIFT_ZERO, 5
    assert refused(cfg) == (-1, "config enum out of range")
    cfg.noise_mode, cfg.K_global = nat.NOISE_SUPPLIED, 99
    assert refused(cfg) == (-1, "K_global must cover k_offset + K_local")
    cfg.K_global, cfg.k_offset = 100, 1
    assert refused(cfg) == (-1, "K_global must cover k_offset + K_local")
    cfg.k_offset, cfg.x0 = 0, None
    assert refused(cfg) == (-1, "null x0 in psp_is_config")
    cfg.x0, cfg.term = ptr, None
    assert refused(cfg) == (-1, "terminal-cost vector missing")
    cfg.term, cfg.drift_kind = ptr, nat.DRIFT_DENSE
    assert refused(cfg) == (-1, "drift parameters missing")
    cfg.drift, cfg.sigma_kind = ptr, nat.SIGMA_DENSE
    assert refused(cfg) == (-1, "sigma matrix missing")
    cfg.sigma, cfg.runcost_kind = ptr, nat.RUNCOST_DIAG_QUAD
    assert refused(cfg) == (-1, "running-cost vector missing")
    cfg.runcost, cfg.control_kind = ptr, nat.ISC_LINEAR
    assert refused(cfg) == (-1, "control kinds TABLE / LINEAR / GRID need u_ref")
    cfg.u_ref = ptr
    s, why = wc.sizes(cfg)
    assert why is None and s.table_bytes == 4 * (5 * 128 + 2 * 128 * 128 + 3 * 128 * 128)
    cfg.control_kind = nat.ISC_GRID
    assert refused(cfg) == (-1, "control kind PSP_ISC_GRID needs u_group and u_row")
    cfg.u_group = cfg.u_row = ptr
    assert refused(cfg) == (-1, "u_ntables / u_nrows / u_ncols must be positive")
    cfg.u_ntables, cfg.u_nrows, cfg.u_ncols = 2, 10, 999
    assert refused(cfg) == (-1, "u_xb / u_dx must be positive")
    cfg.u_xb, cfg.u_dx = 2.5, 0.005
    s, why = wc.sizes(cfg)
    assert why is None and s.lds_bytes == 4 * 2 * 999
    cfg.u_ncols = 30000
    rc, msg = refused(cfg)
    assert rc == -3 and "do not fit the 160 KiB LDS" in msg
    # the rollout makes the same checks before it touches the device, and its own of the buffers
    assert lib.psp_isw_rollout(C.byref(cfg), None, 1, 0, None, None, None, None) == -3
    cfg.u_ncols = 999
    assert lib.psp_isw_rollout(C.byref(cfg), None, 1, 0, None, None, None, None) == -1 and "null logw_out" in nat.last_error()
    assert lib.psp_isw_rollout(C.byref(cfg), None, 1, 0, None, ptr, None, None) == -1 and "tables" in nat.last_error()


def test_the_narrow_query_keeps_its_range(lib):
    cfg, keep = _plain(70)
    assert lib.psp_is_query(C.byref(cfg), None) == -2 and "native range d <= 64" in nat.last_error()
    assert nat.IS_MAX_D == 64


# ---- the keyword -------------------------------------------------------------------------------------------------------------------
def test_wide_states_keyword_on_a_cpu_model():
    assert inspect.signature(psp.do_importance_sampling_me).parameters["wide_states"].default == "torch"
    assert inspect.signature(psp.Solver.__init__).parameters["IS_wide_states"].default == "torch"
    torch.set_num_threads(1)
    prob = psp.LLGC(d=70, off_diag=0.0, T=0.05, seed=42, device="cpu")
    model = psp.Solver("w", prob, L=0, K=16, delta_t=0.01, time_approx="inner", verbose=False, device="cpu")
    assert model.IS_wide_states == "torch"
    for bad in ("hip", None, True, "Native"):
        with pytest.raises(ValueError):
            psp.do_importance_sampling_me(prob, model, 64, control="true", simulate_naive=True, wide_states=bad)
    with pytest.raises(ValueError):
        psp.Solver("w", prob, L=0, K=16, delta_t=0.01, verbose=False, device="cpu", IS_wide_states="hip")
    res = {}
    for ws in ("torch", "native"):                                        # backend='auto': the composite result either way
        torch.manual_seed(3)
        res[ws] = psp.do_importance_sampling_me(prob, model, 64, control="true", simulate_naive=True, wide_states=ws)
    assert len(res["torch"]) == 6 and res["native"] == res["torch"]
    model.backend = "native"
    with pytest.raises(NotImplementedError) as e:
        psp.do_importance_sampling_me(prob, model, 64, control="true", simulate_naive=True, wide_states="native")
    assert "not on a GPU" in str(e.value)
    with pytest.raises(NotImplementedError) as e:                         # ('torch' keeps today's reason)
        psp.do_importance_sampling_me(prob, model, 64, control="true", simulate_naive=True)
    assert "native range" in str(e.value)
