"""The float64 statement of the Solver's per-trajectory u_L2 log (tests/ref64_ul2.py) and the case table of its GPU test
(tests/ul2_cases.py), checked without a GPU and without a kernel:

* the mean of ul2_64 on the reference's host noise against the recorded u_L2_loss[0] of the four fixtures ref64.iteration can
  restate, within the fp32 reference's own rounding (4 x |mean ul2_32 - mean ul2_64|, at least 1e-6 relative);
* the three descriptions of u* against problem.u_true on random states, the grid's ends and the last-trajectory rule included;
* per case: E32 = max_k |ul2_32 - ul2_64| / max(1, max_k ul2_64) and the GPU bound 8 E32 + 5e-7 <= 2e-5 (a case that breaks the
  condition is changed, not the rule); Z x (1 + 1e-3) moves some trajectory by more than 4 x that bound; at most K / 8 trajectories
  of a grid case are `near` a cell edge;
* five planted errors exceed the bound; the first, one wrong trajectory among K, is invisible to the 1e-4 criterion on the mean that
  the golden tests apply;
* the coverage the table promises.

Philox cases are judged here on host noise of the same shape: the conditions are statements about the problem, not the stream.

E32 and the bound per distinct reference (host noise, seed 42):
  narrow LLGC d12 K37 7.4e-8 / 1.1e-6   d20 K72 1.2e-7 / 1.5e-6   d2 8.5e-8 / 1.2e-6   d7 1.3e-7 / 1.6e-6   d100 1.6e-7 / 1.8e-6
  d20 K9001 1.7e-7 / 1.9e-6   d40 1.5e-7 / 1.7e-6   non-adaptive 1.4e-7 / 1.6e-6   sigma basis d33 1.2e-7 / 1.5e-6
  wide LLGC d120 1.2e-7 / 1.5e-6   d200 1.0e-7 / 1.3e-6   d250 1.5e-7 / 1.7e-6   d320 1.2e-7 / 1.5e-6   d500 1.1e-7 / 1.4e-6
  d505 1.3e-7 / 1.5e-6   d200 K9001 1.7e-7 / 1.9e-6
  LQGC d2 8.4e-8 / 1.2e-6   d20 9.9e-8 / 1.3e-6   d33 1.5e-7 / 1.7e-6   d20 K8208 1.9e-7 / 2.0e-6   d130 1.1e-7 / 1.4e-6
  double wells d1 4.8e-8 / 8.8e-7 (delta 7.1e-5 cells, 0 near)   d30 1.2e-7 / 1.4e-6 (delta 9.6e-5 cells, 1 of 50 near)
"""
import numpy as np
import pytest
import torch

import block_cases as bc
import ref64
import ref64_ul2 as r64u
import ul2_cases as uc
from util_cases import make_oracle, make_pkg_problem

FIXTURES = ("llgc_d8_logvar_ul2", "lqgc_d2_logvar", "dw1d_logvar_ul2", "dw_d6_mixed_logvar_ul2")
MEAN_TOL = 1e-4             # what the golden tests hold the logged mean to


def _case_reference(c):
    K = bc.case_K(c)
    return K, uc.references(c, K, lambda: bc.host_noise(42, K, c["d"], c["N"]))


# ---- anchor: the reference's own recorded log ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_mean_matches_the_recorded_log_of_the_reference(golden, name):
    rec = golden(name)
    case = rec["case"]
    problem = make_pkg_problem(case["problem"], "cpu")
    ocase = dict(case)
    if case["problem"]["kind"] == "DoubleWell":                           # (ref64 knows the multidimensional class: d_1 = 1, d_2 = 0)
        kw = case["problem"]["kwargs"]
        ocase["problem"] = dict(kind="DoubleWell_multidim", kwargs=dict(d=1, d_1=1, d_2=0, T=kw["T"], eta=kw["eta"], kappa=kw["kappa"]))
    oprob, ocfg, omodels = make_oracle(ocase, L=1)
    s = case["solver"]
    N = int(np.floor(oprob.T / s["delta_t"]))
    assert N == rec["expected"]["N"]
    xi = bc.host_noise(s["seed"], s["K"], oprob.d, N)
    desc = r64u.describe(problem, N, s["delta_t"])
    dt = float(torch.tensor(s["delta_t"]))
    means = {}
    for dtype in (torch.float64, torch.float32):
        r = ref64.iteration(oprob, ocfg, omodels[0], xi, dtype=dtype, want_path=True)
        means[dtype] = float(r64u.ul2(desc, r["Z"], r["X"], dt, dtype=dtype).double().mean())
    want = rec["expected"]["u_L2_loss"][0]
    m64, m32 = means[torch.float64], means[torch.float32]
    tol = max(4.0 * abs(m32 - m64), 1e-6 * abs(m64))
    print("%s [%s]: mean ul2_64 %.9g  ul2_32 %.9g  recorded %.9g  |diff| %.2e (<= %.2e)" % (name, desc["kind"], m64, m32, want,
                                                                                         abs(m64 - want), tol))
    assert abs(m64 - want) <= tol


# ---- the three descriptions against problem.u_true -------------------------------------------------------------------------------
def _u_true(problem, X, t):
    return torch.tensor(np.asarray(problem.u_true(X, t))).t().float()    # (K, d), as solver.py:493 forms it


@pytest.mark.parametrize("cid", ["table-small-d-LLGC-d7-H30-K40-det-fp32-log-va-fwd_variant1-ref", "gains-48x32-LQGC-d33-H17-K40-det-fp32-log-va-fwd_variant2-phi",
                                 "grid-dw1d-Doub-d1-H30-K112-det-fp32-log-va-ref", "grid-dw30-Doub-d30-H64-K50-det-fp32-log-va-fwd_variant1-phi"])
def test_descriptions_reproduce_u_true(cid):
    c = uc.BY_ID[cid]
    problem = uc.pkg_problem(c)
    desc = r64u.describe(problem, c["N"], c["dt"])
    assert desc["kind"] == c["ukind"]
    K, d = 37, c["d"]
    g = torch.Generator().manual_seed(11)
    X = 1.5 * torch.randn(K, d, generator=g)
    if desc["kind"] == "grid":
        xb = problem.xb
        X[0], X[1] = xb + 0.7, -xb - 0.3                                  # beyond the grid on both sides
        X[2] = xb - 2 * problem.dx                                        # the upper clamp bound itself
        X[-1] = -xb + 0.25 * torch.rand(d, generator=g) * (xb / 100)      # last trajectory in the first cells: cell - 2 < 0
    for n in range(c["N"]):
        want = _u_true(problem, X, n * c["dt"])
        got32 = r64u.u_star(desc, X, n, last=True, dtype=torch.float32)[0]
        got64 = r64u.u_star(desc, X, n, last=True)[0]
        if desc["kind"] == "grid":
            assert torch.equal(got32, want), (cid, n)                     # the same fp32 cell arithmetic: bit-equal
            assert torch.equal(got64.float(), want), (cid, n)             # (no state of this set sits on a cell edge)
        else:
            scale = max(1.0, float(want.abs().max()))
            assert float((got32 - want).abs().max()) <= 1e-6 * scale and float((got64 - want.double()).abs().max()) <= 1e-6 * scale
    if desc["kind"] == "grid":                                            # without the last-trajectory rule only row K - 1 changes
        other = r64u.u_star(desc, X, 1, last=False)[0]
        got = r64u.u_star(desc, X, 1, last=True)[0]
        assert torch.equal(other[:-1], got[:-1]) and not torch.equal(other[-1], got[-1])


# ---- per case: E32, the GPU bound, sensitivity, near share -----------------------------------------------------------------------
@pytest.mark.parametrize("cid", uc.IDS)
def test_fp32_stand_in_sets_a_bound_below_d_tol(cid):
    c = uc.BY_ID[cid]
    K, R = _case_reference(c)
    u64 = R["r64"]["ul2"]
    zero = r64u.ul2(R["desc"], torch.zeros_like(R["r64"]["Z"]), R["r64"]["X"], R["dt"])
    share = abs(float(u64.mean()) - float(zero.mean())) / float(u64.mean())
    print("%s: E32 %.2e  bound %.2e  mean ul2 %.4g  max %.4g  median |Z| %.2f  Z-dependent share of the mean %.1f %% "
          "(fixtures llgc_d8_logvar_ul2 / llgc_d40_moment_ul2: 0.9 %% / 0.16 %%)"
          % (cid, R["E32"], R["bound"], float(u64.mean()), float(u64.max()), float(R["r64"]["Z"].abs().median()), 100 * share))
    assert bool(torch.isfinite(u64).all()) and R["r32"]["ul2"].dtype == torch.float32
    assert R["bound"] <= uc.D_TOL, (cid, R["E32"])
    assert c["N"] in (3, 4) and c["dt"] == 0.05 and c["expect"][0] in (1, 2)
    assert share >= 0.02, "the log of this case depends on the net no more than that of the fixtures"
    # sensitivity: a relative error of 1e-3 in Z
    moved = r64u.ul2(R["desc"], R["r64"]["Z"] * (1.0 + 1e-3), R["r64"]["X"], R["dt"])
    assert float((moved - u64).abs().max()) > 4.0 * R["bound"] * max(1.0, float(u64.max()))


@pytest.mark.parametrize("cid", [i for i in uc.IDS if uc.BY_ID[i]["ukind"] == "grid"])
def test_near_share_of_the_grid_cases(cid):
    c = uc.BY_ID[cid]
    K, R = _case_reference(c)
    n_near = int(R["near"].sum())
    print("%s: delta %.2e cells, %d of %d trajectories near a cell edge (cap %d)" % (cid, R["delta"], n_near, K, K // 8))
    assert 0.0 < R["delta"] < 1e-3
    assert n_near <= K // 8


# ---- planted errors --------------------------------------------------------------------------------------------------------------
def _planted(c, R):
    """name -> ul2 (K,) float64 with one error planted in the float64 statement."""
    desc, Z, X, dt, d = R["desc"], R["r64"]["Z"], R["r64"]["X"], R["dt"], c["d"]
    u64 = R["r64"]["ul2"]
    out = {}
    gaps = (u64[1:] - u64[:-1]).abs()
    limit = 4.0 * R["bound"] * max(1.0, float(u64.max()))
    k = 1 + int(torch.argmin(torch.where(gaps > limit, gaps, torch.full_like(gaps, float("inf")))))
    nb = u64.clone()
    nb[k] = u64[k - 1]                                                    # a wrong k in a.ul2[k] / a padding row of a ragged tile
    out["neighbour"] = nb
    if desc["kind"] == "table":
        # one feature past d: Z is zero there (zero-padded W3, b3), the table holds the next row's first entry (zero after the
        # last row) -- what a `<=` in the wide kernel's last-block mask would read at an exact instance
        nxt = torch.cat([desc["table"][1:, 0], torch.zeros(1)]).double()
        out["extra feature"] = u64 + dt * float((nxt ** 2).sum())
        out["row n + 1"] = r64u.ul2(dict(desc, table=torch.roll(desc["table"], -1, 0)), Z, X, dt)
    else:
        key = "gains" if desc["kind"] == "gains" else "row"
        rolled = torch.roll(desc["gains"], -1, 0) if key == "gains" else desc["row"][1:] + desc["row"][:1]
        out["row n + 1"] = r64u.ul2(dict(desc, **{key: rolled}), Z, X, dt)
        out["X_n for X_n+1"] = r64u.ul2(desc, Z, torch.cat([X[:1], X[:-1]]), dt)
        if d > 1:                                                         # the last feature left out of the sum
            drop = sum(torch.sum((-Z[n] - r64u.u_star(desc, X[n + 1], n)[0])[:, :d - 1] ** 2, 1) for n in range(c["N"])) * dt
            out["feature dropped"] = drop
    out["Z - u*"] = r64u.ul2(desc, -Z, X, dt)
    return out, k


@pytest.mark.parametrize("cid", uc.IDS)
def test_the_bound_catches_planted_errors(cid):
    c = uc.BY_ID[cid]
    K, R = _case_reference(c)
    u64, keep = R["r64"]["ul2"], ~R["near"]
    limit = R["bound"] * max(1.0, float(u64.max()))
    planted, k = _planted(c, R)
    for name, got in planted.items():
        worst = float((got - u64).abs()[keep].max())
        mean_err = abs(float(got.mean()) - float(u64.mean())) / float(u64.mean())
        print("%s / %s: worst trajectory %.2e (limit %.2e), mean moves by %.2e" % (cid, name, worst, limit, mean_err))
        assert worst > limit, (cid, name)
    assert keep[k]


def test_one_wrong_trajectory_escapes_the_criterion_on_the_mean():
    """The neighbour's value in one trajectory (the pair of adjacent trajectories closest to each other that the bound still tells
    apart) moves the mean by less than the 1e-4 the golden tests allow: in at least three quarters of the cases -- at K = 37 .. 48
    the closest pair can be 1e-2 apart -- and in every case of a route the issue names: K = 9001, the wide instances, the grid."""
    escaped = {}
    for c in uc.CASES:
        K, R = _case_reference(c)
        u64 = R["r64"]["ul2"]
        nb = _planted(c, R)[0]["neighbour"]
        escaped[c["id"]] = abs(float(nb.mean()) - float(u64.mean())) / float(u64.mean()) <= MEAN_TOL
    print("escapes the mean criterion: %d of %d cases" % (sum(escaped.values()), len(escaped)))
    assert 4 * sum(escaped.values()) >= 3 * len(escaped)
    for c in uc.CASES:
        if c["K"] == 9001 or c["expect"][0] == 2 or c["ukind"] == "grid":
            assert escaped[c["id"]], c["id"]


# ---- coverage --------------------------------------------------------------------------------------------------------------------
def test_case_table_coverage():
    C = uc.CASES
    table = [c for c in C if c["ukind"] == "table"]
    assert {c["ukind"] for c in C} == {"table", "gains", "grid"}
    # every narrow forward x noise mode, with the log accumulated in the kernel
    for v in "123":
        for noise in ("reference", "philox"):
            assert any(c["env"].get("PSP_FWD_VARIANT") == v and c["noise"] == noise and c["expect"][0] == 1 for c in table), (v, noise)
    for mode in ("f16x3", "bf16"):
        for noise in ("reference", "philox"):
            got = {c["expect"][1:] for c in table if c["mode"] == mode and c["noise"] == noise and c["expect"][0] == 1}
            assert {(32, 48), (48, 48)} <= got, (mode, noise)
    # the wide LOGU instances, each in both matrix modes on both noises
    for inst in uc.WIDE_INSTANCES:
        combos = {(c["mode"], c["noise"]) for c in table if c["expect"] == (2,) + inst}
        assert combos == {(m, n) for m in ("fp32", "f16x3") for n in ("reference", "philox")}, inst
    assert {(128, 64), (200, 64), (256, 64), (320, 64), (512, 64)} <= set(uc.WIDE_INSTANCES)
    assert any(c["expect"] == (2, 200, 64) and c["K"] == 9001 for c in table)
    assert any(c["expect"] == (1, 32, 48) and c["K"] == 9001 for c in table)
    assert {(2, 30), (8, 30), (100, 64)} <= {c["expect"][1:] for c in table if c["expect"][0] == 1}
    assert any(c["basis"] == "sigma" for c in table) and any(not c["adaptive"] for c in table)
    # every store_path, for the kernels' log and for the decode of the path store
    store = lambda c: 3 if c["loss"] == "relative_entropy" else (2 if not c["detach"] else (4 if c["regen"] else 1))
    assert {store(c) for c in table} == {1, 2, 3}                          # (store_path 4 needs no u_ref: LQGC below)
    gains = [c for c in C if c["ukind"] == "gains"]
    assert {store(c) for c in gains} == {1, 2, 3, 4}
    assert {c["mode"] for c in gains if c["expect"] == (1, 32, 48)} == {"fp32", "f16x3", "bf16"}
    assert {c["mode"] for c in gains if c["expect"] == (2, 192, 64)} == {"fp32", "f16x3"}
    assert {(2, 30), (48, 32)} <= {c["expect"][1:] for c in gains}
    grid = [c for c in C if c["ukind"] == "grid"]
    assert {(c["kind"], c["d"], c["K"]) for c in grid} == {("DoubleWell", 1, 112), ("DoubleWell_multidim", 30, 50)}
    mdw = uc.pkg_problem([c for c in grid if c["d"] == 30][0])
    assert (mdw.d_1, mdw.d_2) == (28, 2) and len(mdw.u_true_tables()["tables"]) == 2
