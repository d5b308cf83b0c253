"""The float64 reference of psp_is_rollout (tests/ref64_is.py) and the case table of its GPU tests (tests/is_kernel_cases.py),
checked without a GPU and without the kernel:

* rollout64 against utilities._is_composite_full (reference utilities.py:296-337 restated) run in float64 on the CPU on the same
  noise: per-trajectory log-weights and final states to 1e-10, for the naive path and for control='true', on DoubleWell(d = 1),
  DoubleWell_multidim(d = 4), LLGC(d = 6) and LQGC(d = 3).  delta_t = 1/64, so that dt and sqrt(dt) = 1/8 are the same numbers in
  fp32 and in float64.  The composite plan casts u* with Tensor.float(); for this run the cast keeps float64.
* rollout32 against rollout64 on every case: E32_w, E32_x <= 1e-4 (the error scale the GPU bounds are built from).
* the share of `near` trajectories of every GRID case <= 10 %, the last global trajectory never among them.
* the coverage the case table promises, so that a later edit cannot quietly shrink it.
"""
import contextlib
from unittest import mock

import numpy as np
import pytest
import torch

import is_kernel_cases as kc
import ref64_is as r64
from util_cases import psp

nat = psp.native
NEAR_CAP = 0.10


# ---- rollout64 against the composite plan in float64 -----------------------------------------------------------------------------
@contextlib.contextmanager
def float64_composite(noise):
    """torch in float64 with torch.randn handing out `noise` slice by slice (slice n + 1 at the n-th call)."""
    calls = [0]

    def randn(K, d):
        calls[0] += 1
        assert noise[calls[0]].shape == (K, d)
        return torch.from_numpy(noise[calls[0]].astype(np.float64))

    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        with mock.patch.object(torch, "randn", randn), mock.patch.object(torch.Tensor, "float", lambda t: t.double()):
            yield
    finally:
        torch.set_default_dtype(old)


def _to_double(problem):
    """The problem's tensors in float64 (the same numbers).  The double wells start at X_0 = -1, which is the edge between two
    cells of their u* tables ((-1 + 2.5) / 0.005 = 300): every trajectory would be `near` at step 0, so they start next to it."""
    if hasattr(problem, "u_true_tables"):
        problem.X_0 = problem.X_0 + 0.00127
    for name, v in list(vars(problem).items()):
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(problem, name, v.double())
    return problem


class _Model:
    """What _is_composite_full reads of a solver."""
    device = torch.device("cpu")
    u_l2_error_flag = True

    def __init__(self, problem):
        self.f = problem.f


DT = 1.0 / 64


def _dw1():
    p = psp.DoubleWell(d=1, T=0.25, eta=3.0, kappa=5.0, device="cpu")
    p.compute_reference_solution()
    return p


def _dw4():
    p = psp.DoubleWell_multidim(d=4, d_1=2, d_2=2, T=0.25, eta=2.0, kappa=3.0, device="cpu")
    p.compute_reference_solution()
    p.compute_reference_solution_2()
    return p


PROBLEMS = {"dw1d": _dw1, "dw4": _dw4, "llgc6": lambda: psp.LLGC(d=6, off_diag=0.1, T=0.25, seed=42, device="cpu"),
            "lqgc3": lambda: psp.LQGC(d=3, off_diag=0.1, T=0.25, seed=42, delta_t=DT, device="cpu")}
_KIND_OF_UL2 = {nat.UL2_TABLE: nat.ISC_TABLE, nat.UL2_LINEAR: nat.ISC_LINEAR, nat.UL2_GRID: nat.ISC_GRID}


def _describe_problem(problem, kind, K, noise):
    """The description of a catalogue problem's call, from native_spec and ul2_reference as utilities._is_config forms it."""
    d = problem.d
    N = int(np.ceil(problem.T / DT))
    spec = problem.native_spec()
    num = lambda t: None if t is None else np.asarray(t.detach().cpu())
    desc = dict(d=d, K_local=K, K_global=K, k_offset=0, N=N, dt=kc.f32(DT), sqrt_dt=kc.f32(np.sqrt(DT)),
                drift_kind=spec["drift"][0], sigma_kind=spec["sigma"][0], sigma_scale=float(spec["sigma"][2]),
                runcost_kind=spec["runcost"][0], term_kind=spec["term"][0], dwell_form=1 if isinstance(problem, psp.DoubleWell) else 0,
                drift=num(spec["drift"][1]), sigma=num(spec["sigma"][1]), runcost=num(spec["runcost"][1]), term=num(spec["term"][1]),
                control_kind=kind, x0=num(torch.as_tensor(problem.X_0).reshape(-1)), noise=noise)
    if kind != nat.ISC_NONE:
        ref = psp.plan_dense_native.ul2_reference(problem, N, DT, d, K, 0)
        if kind == nat.ISC_TABLE:
            desc["table"] = num(ref["table"])
        elif kind == nat.ISC_LINEAR:
            desc["gains"] = num(ref["gains"])
        else:
            desc.update(tables=num(ref["tables"]), group=num(ref["group"]), row=num(ref["row"]), xb=ref["xb"], dx=ref["dx"],
                        xhi=ref["xhi"], nrows=ref["nrows"], ncols=ref["ncols"])
    return desc


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_rollout64_matches_the_composite_plan_in_float64(name):
    assert kc.f32(DT) == DT and kc.f32(np.sqrt(DT)) == np.sqrt(DT)
    K = 64
    problem = _to_double(PROBLEMS[name]())
    d, N = problem.d, int(np.ceil(problem.T / DT))
    noise = np.random.default_rng(77).standard_normal((N + 1, K, d)).astype(np.float32)
    kind = _KIND_OF_UL2[psp.plan_dense_native.ul2_kind(problem)]
    with float64_composite(noise):
        w_naive, w_is, X, X_u = psp.utilities._is_composite_full(problem, _Model(problem), K, "true", True, DT)
        descs = {"naive": _describe_problem(problem, nat.ISC_NONE, K, noise), "true": _describe_problem(problem, kind, K, noise)}
    assert w_is.dtype == torch.float64 and X_u.dtype == torch.float64
    for tag, w, Xc in (("naive", w_naive, X), ("true", w_is, X_u)):
        out = r64.rollout64(descs[tag])
        keep = np.ones(K, dtype=bool)
        if descs[tag]["control_kind"] == nat.ISC_GRID:
            print("%s/%s: near share %.3f" % (name, tag, out[2].mean()))
            assert out[2].mean() <= NEAR_CAP
            keep = ~out[2]
        lw = np.log(w.numpy())
        ew = np.abs(out[0] - lw)[keep] / np.maximum(1.0, np.abs(lw[keep]))
        ex = np.abs(out[1] - Xc.numpy())[keep] / np.maximum(1.0, np.abs(Xc.numpy()[keep]))
        print("%s/%s: log-weight %.2e, state %.2e (%d trajectories)" % (name, tag, ew.max(), ex.max(), keep.sum()))
        assert ew.max() <= 1e-10 and ex.max() <= 1e-10
        assert np.abs(out[0]).max() > 1e-3                                 # (not a comparison of zeros)


# ---- rollout32 against rollout64: the error scale of the GPU bounds --------------------------------------------------------------
@pytest.mark.parametrize("cid", kc.IDS)
def test_float32_recursion_is_well_conditioned(cid):
    c = kc.BY_ID[cid]
    desc, logw64, XN64, keep, ew, ex, logw32, XN32 = kc.reference(c)
    print("%s %s: E32_w %.2e  E32_x %.2e  max |logw| %.3g  max |XN| %.3g  kept %d / %d"
          % (cid, kc.route(c), ew, ex, np.abs(logw64).max(), np.abs(XN64).max(), keep.sum(), keep.size))
    assert np.all(np.isfinite(logw64)) and np.all(np.isfinite(XN64))
    assert logw32.dtype == np.float32 and XN32.dtype == np.float32
    assert ew <= 1e-4 and ex <= 1e-4, (ew, ex)


@pytest.mark.parametrize("cid", kc.GRID_IDS)
def test_near_share_of_the_grid_cases(cid):
    c = kc.BY_ID[cid]
    desc, logw64, XN64, keep = kc.reference(c)[:4]
    share = 1.0 - keep.mean()
    print("%s: near share %.4f (2e-4 d N = %.4f)" % (cid, share, 2e-4 * c["d"] * c["N"]))
    assert share <= NEAR_CAP
    assert keep[r64.last_local(desc)], "the last global trajectory must count"
    if kc.bucket(c["d"]) >= 32:
        assert c["N"] <= 4


def test_the_last_trajectory_rule_changes_its_control():
    """The GRID kind's last-trajectory rule must be visible in the result: without it (K_global past this call) the last
    trajectory's log-weight differs by far more than any bound; every other trajectory is unchanged."""
    for cid in kc.GRID_IDS:
        c = kc.BY_ID[cid]
        desc, logw64 = kc.reference(c)[:2]
        other = r64.rollout64(dict(desc, K_global=desc["K_global"] + 1))[0]
        kl = r64.last_local(desc)
        assert kl == c["K"] - 1
        assert abs(other[kl] - logw64[kl]) > 1e-3 * max(1.0, abs(logw64[kl])), cid
        assert np.array_equal(np.delete(other, kl), np.delete(logw64, kl))


@pytest.mark.parametrize("cid", kc.IDS)
def test_the_bounds_catch_planted_errors(cid):
    """What the GPU bounds 8 x E32 + 5e-7 must catch, planted in the float32 recursion's inputs: the noise read one slice early
    (step n driven by slice n), the control taken after the update instead of before (u_ref of step n + 1), and a single
    trajectory -- the first lane of the second workgroup, or the last one -- driven by its neighbour's noise."""
    c = kc.BY_ID[cid]
    desc, logw64, XN64, keep, ew32, ex32 = kc.reference(c)[:6]
    bw, bx = kc.bounds(ew32, ex32)
    assert bw <= 1e-3 and bx <= 1e-3

    def caught(planted):
        lw, XN = r64.rollout32(planted)
        ew, ex = r64.errors(lw, XN, logw64, XN64, keep)
        return ew > bw or ex > bx

    early = desc["noise"].copy()
    early[1:] = np.concatenate([np.zeros_like(early[:1]), early[1:-1]])
    assert caught(dict(desc, noise=early))
    if c["ctrl"] in (nat.ISC_TABLE, nat.ISC_LINEAR) and c["N"] > 1:
        key = "table" if c["ctrl"] == nat.ISC_TABLE else "gains"
        assert caught(dict(desc, **{key: np.roll(desc[key], -1, axis=0)}))
    if c["K"] > 1:
        k = 256 if c["K"] > 256 else c["K"] - 1
        one = desc["noise"].copy()
        one[:, k] = one[:, k - 1]
        if keep[k]:
            assert caught(dict(desc, noise=one))


def test_wrap_case_reads_the_row_from_its_end():
    c = kc.BY_ID["b4_grid_d2_x0_low"]
    desc = kc.describe(c)
    X = np.tile(desc["x0"].astype(np.float64), (c["K"], 1))
    cell = r64._grid_cells(X, desc, np.float64)[0]
    assert cell[-1, 0] == desc["ncols"] - 2 and np.all(cell[:-1, 0] == 0)
    c = kc.BY_ID["b16_grid_d5_x0_high"]
    desc = kc.describe(c)
    assert desc["x0"][1] > desc["xhi"]
    cell = r64._grid_cells(desc["x0"].astype(np.float64)[None, :].repeat(2, 0), dict(desc, K_local=2, K_global=9), np.float64)[0]
    assert cell[0, 1] == int(np.floor((desc["xhi"] + desc["xb"]) / desc["dx"]))


# ---- the coverage of the case table ----------------------------------------------------------------------------------------------
def test_case_table_limits():
    for c in kc.CASES:
        assert 1 <= c["N"] <= 12 and 1 <= c["K"] <= 300 and 0.01 <= c["dt"] <= 0.05, c["id"]
        desc = kc.describe(c)
        free = np.ones(c["d"], dtype=bool)
        if c["edge"] == "x0_low":
            free[0] = False
        if c["edge"] == "x0_high":
            free[1] = False
        assert np.all(np.abs(desc["x0"][free]) <= 1.0)
        for key in ("x0", "drift", "sigma", "runcost", "term", "noise"):
            assert desc[key] is None or desc[key].dtype == np.float32
        assert np.all(np.isnan(desc["noise"][0])) and np.all(np.isfinite(desc["noise"][1:]))


def test_every_instance_and_bucket_edge_is_covered():
    pairs = {(kc.bucket(c["d"]), c["ctrl"]) for c in kc.CASES}
    assert pairs == {(b, k) for b in kc.BUCKETS for k in (nat.ISC_NONE, nat.ISC_TABLE, nat.ISC_LINEAR, nat.ISC_GRID)}
    controlled = {c["d"] for c in kc.CASES if c["ctrl"] != nat.ISC_NONE}
    assert {1, 2, 5, 17, 33} <= controlled and {1, 4, 16, 32, 64} <= controlled
    assert [kc.bucket(d) for d in (1, 2, 5, 17, 33)] == list(kc.BUCKETS) and [kc.bucket(d) for d in kc.BUCKETS] == list(kc.BUCKETS)
    assert [kc.bucket(d - 1) for d in (2, 5, 17, 33)] == [1, 4, 16, 32]
    assert {1, 37, 256, 257, 300} <= {c["K"] for c in kc.CASES}


def test_every_coefficient_kind_is_covered():
    pairs = {(c["drift"], c["sigma"]) for c in kc.CASES}
    assert pairs >= {(a, b) for a in ("zero", "dense", "diag", "dwell0", "dwell1") for b in ("I", "dense", "sI")}
    assert any(c["drift"] == "dense" and c["sigma"] == "sI" and c["ctrl"] == nat.ISC_LINEAR for c in kc.CASES)
    assert any(c["drift"] == "diag" and c["sigma"] == "dense" and c["ctrl"] != nat.ISC_NONE for c in kc.CASES)
    assert any(c["sigma"] == "I" and c["ctrl"] != nat.ISC_NONE for c in kc.CASES)
    assert {c["run"] for c in kc.CASES} == {"zero", "diagq"} and {c["term"] for c in kc.CASES} == {"lin", "diagq", "shift"}
    assert any(c["term"] == "shift" and not c["drift"].startswith("dwell") for c in kc.CASES)
    for c in kc.CASES:                                                    # the names reach the description as the enums
        desc = kc.describe(c)
        assert desc["dwell_form"] == (1 if c["drift"] == "dwell1" else 0)
        assert (desc["drift"] is None) == (c["drift"] == "zero") and (desc["sigma"] is None) == (c["sigma"] != "dense")
        assert (desc["runcost"] is None) == (c["run"] == "zero")
        if c["drift"] == "dense":
            assert desc["drift"].shape == (c["d"], c["d"])


def test_grid_cases_carry_their_edges():
    edges = set()
    for cid in kc.GRID_IDS:
        c = kc.BY_ID[cid]
        desc = kc.describe(c)
        row = desc["row"]
        assert desc["tables"].shape[0] >= 2 and len(set(desc["group"].tolist())) >= (2 if c["d"] > 1 else 1)
        assert np.any(np.diff(row) < 0) and np.any(np.diff(row) > 0), (cid, row)
        assert 0 < desc["xhi"] < desc["xb"] and abs((desc["xhi"] + desc["xb"]) / desc["dx"] % 1.0 - 0.5) < 1e-3
        if np.any(row < 0) and np.any(row >= desc["nrows"]):
            edges.add("row_oob")
        elif c["edge"] != "row_oob":
            assert np.all((row >= 0) & (row < desc["nrows"]))
        if np.any(desc["x0"] <= -desc["xb"]):
            edges.add("x0_low")
        if np.any(desc["x0"] > desc["xhi"]):
            edges.add("x0_high")
    assert edges == {"row_oob", "x0_low", "x0_high"}


def test_selections_of_the_gpu_module():
    assert sorted(kc.BY_ID[i]["d"] for i in kc.PHILOX_IDS) == [1, 2, 4, 5, 16, 17, 32, 33, 64]
    ctrls = [kc.BY_ID[i]["ctrl"] for i in kc.SHARD_IDS]
    assert ctrls == [nat.ISC_GRID, nat.ISC_LINEAR]
    assert [kc.BY_ID[i]["K"] for i in kc.EDGE_IDS] == [1, 37, 257]
    exact = [c for c in kc.CASES if kc.bit_exact(c)]                     # (b): every bucket, the three kinds it covers
    assert {kc.bucket(c["d"]) for c in exact} == set(kc.BUCKETS)
    assert {c["ctrl"] for c in exact} == {nat.ISC_NONE, nat.ISC_TABLE, nat.ISC_GRID}
    assert {c["drift"] for c in exact} == {"zero", "diag", "dwell0", "dwell1"} and {c["sigma"] for c in exact} == {"I", "sI"}


@pytest.fixture(scope="module")
def lib():
    if not nat.is_built():
        import __graft_entry__
        __graft_entry__.build()
    return nat.load()


@pytest.mark.parametrize("cid", kc.IDS)
def test_every_config_is_accepted_by_the_library(lib, cid):
    c = kc.BY_ID[cid]
    for desc in (kc.describe(c), kc.describe(c, K=257, K_global=kc.PHILOX_OFFSET + 300, k_offset=kc.PHILOX_OFFSET,
                                             noise=np.zeros((c["N"] + 1, 257, c["d"]), np.float32))):
        cfg, keep = kc.device_config(desc, torch.device("cpu"))
        assert kc.query(cfg) is None, (cid, kc.query(cfg))
