"""tests/ref64_general.py (the float64 reference of one GeneralSolver / EllipticSolver iteration) and the block comparison of
tests/general_block_cases.py, checked on the CPU:

  a. the judge is finer than what it judges: on every case of the table the fp32 oracle (oracle/pathspace_oracle.py) agrees with the
     float64 reference per block to a tenth of the GPU test's bound (2e-5 of the block's own maximum), the loss to 5e-6, and every
     discrete decision (K_count, active steps per trajectory, executed loop steps) exactly;
  b. every case satisfies the conditions the GPU test relies on: in every block the kernels' part of the gradient reaches half of
     the block's maximum, no block is under the floor, relu^2 pre-activations keep 8 e_fp32 of the sum of the absolute terms of
     their dot product away from zero, exit-test and time-test quantities keep 1e-5 (relative) away from their thresholds, and the
     cases meant to leave the time loop early do;
  c. five planted errors, each ACCEPTED by the whole-gradient criterion of the existing GPU tests (max |g - g_ref| <= 5e-4 max |g_ref|)
     and REJECTED by the block criterion at 2e-4 by a factor of at least ten."""
import math

import pytest
import torch

import general_block_cases as gc
from ref64_general import E32

BLOCK_TOL = 2e-4            # the GPU test's bound per block
JUDGE_TOL = BLOCK_TOL / 10  # the fp32 oracle against the float64 reference, per block
LOSS_TOL = 5e-6
FLAT_TOL = 5e-4             # the whole-gradient criterion of tests/test_gpu_genl_fuzz.py and the other value-net GPU tests
MIN_MARGIN = 1e-5
RELU_MARGIN = 8 * E32
IDS = [c["id"] for c in gc.CASES]


def per_trajectory_errors(tr, ref, elliptic):
    """{quantity: max |fp32 oracle - float64| / max(1, max |float64|)} of the end points of the rollout."""
    out = {}
    for name, key in (("YN", "Y_N"), ("VN", "V_N"), ("XN", "X_N")) + (() if elliptic else (("tN", "t_N"),)):
        want = ref[name]
        out[name] = float((tr[key].double() - want).abs().max()) / max(1.0, float(want.abs().max()))
    return out


@pytest.mark.parametrize("c", gc.CASES, ids=IDS)
def test_fp32_oracle_matches_the_float64_reference_per_block(c):
    run = gc.runs(c)
    tr, ref = run["trace"], run["ref"]
    lay, kw = gc.layout(c)
    g32 = torch.cat([g.reshape(-1) for g in tr["grads"]])
    assert g32.shape == ref["grad"].shape and bool(torch.isfinite(ref["grad"]).all())
    names, errs = gc.assert_general_blocks(g32, ref["grad"], lay, JUDGE_TOL, tag="fp32 oracle vs ref64 " + c["id"], **kw)
    el = abs(run["loss32"] - ref["loss"]) / abs(ref["loss"])
    pt = per_trajectory_errors(tr, ref, c["family"] == "elliptic")
    print("%s: loss %.9g / %.9g (rel %.1e)  worst block %.2e (%s)  per trajectory %s" % (
        c["id"], run["loss32"], ref["loss"], el, max(errs), names[errs.index(max(errs))], "  ".join("%s %.1e" % kv for kv in pt.items())))
    assert el <= LOSS_TOL, (run["loss32"], ref["loss"])
    assert run["K_log32"] == ref["K_count"]
    assert torch.equal(torch.as_tensor(tr["steps"]), ref["steps"])
    assert len(tr["xi"]) == ref["n_loop"]


@pytest.mark.parametrize("c", gc.CASES, ids=IDS)
def test_cases_satisfy_the_conditions(c):
    ref = gc.runs(c)["ref"]
    lay, kw = gc.layout(c)
    names, blocks = gc.general_grad_blocks(ref["grad"], *lay, **kw)
    _, dom = gc.general_grad_blocks(ref["grad_domain"], *lay, **kw)
    gmax = float(ref["grad"].abs().max())
    share = {n: float(b.abs().max()) / gmax for n, b in zip(names, blocks)}
    domain = {n: float(q.abs().max()) / float(b.abs().max()) for n, b, q in zip(names, blocks, dom)}
    m = ref["margins"]
    ts = ref["tile_steps"]
    print("%s: smallest block %.2e (%s)  smallest domain part %.2f (%s)  margins exit %.1e time %.1e relu %.1e  K_count %d  "
          "tile steps %d..%d  loop %d" % (c["id"], min(share.values()), min(share, key=share.get), min(domain.values()),
                                           min(domain, key=domain.get), m["exit"], m["time"], m["relu"], ref["K_count"], int(ts.min()),
                                           int(ts.max()), ref["n_loop"]))
    assert all(v >= gc.BLOCK_FLOOR for v in share.values()), share
    assert all(v >= 0.5 for v in domain.values()), domain
    assert m["exit"] >= MIN_MARGIN and m["time"] >= MIN_MARGIN, m
    assert m["relu"] >= RELU_MARGIN, m
    assert ref["K_count"] > 0 and math.isfinite(ref["loss"])
    if c["early"]:
        assert int(ts.min()) < int(ts.max()) or ref["n_loop"] < c["solver"]["N"], ts
    if c["solver"]["loss_with_stopped"]:
        assert bool((ref["steps"] < c["solver"]["N"]).any())


def test_table_covers_the_routes():
    C = gc.CASES
    gen = [c for c in C if c["route"]["plan"] == "gen"]
    genl = [c for c in C if c["route"]["plan"] == "genl"]
    for inst in ((6, 30), (10, 24), (100, 64), (16, 32), (48, 48)):
        assert {c["mode"] for c in gen if c["route"]["inst"] == inst} == {"fp32", "f16x3"}, inst
    assert {c["solver"]["K"] for c in gen} >= {1, 16, 40, 257}
    assert any(c["family"] == "elliptic" for c in gen) and any(c["solver"]["loss_with_stopped"] for c in gen)
    assert any(c["solver"].get("boundary_type") == "Neumann" for c in gen)
    assert {c["solver"]["loss_method"] for c in gen} == {"diffusion", "BSDE"}
    assert {c["solver"]["adaptive_forward_process"] for c in gen} == {True, False}
    assert {c["route"]["fwd"] for c in genl} == {1, 4, 8}
    assert {c["route"]["bwd"] for c in genl} == {"genl_bwd_kernel<1>", "genl_bwd_kernel<8, 3>", "genl_bwd_kernel<8, 4>"}
    assert {len(c["net"]["arch"]) for c in genl} == {1, 2, 3, 4}
    assert {h for c in genl for h in c["net"]["arch"]} >= {1, 17, 33, 65, 110, 128}
    d_in = {c["problem"]["kwargs"]["d"] + (0 if c["family"] == "elliptic" else 1) for c in genl}
    assert d_in >= {2, 16, 17, 112}, d_in
    assert {c["net"]["kind"] for c in genl} == {"densenet", "user_tanh2", "densenet_tanh", "densenet_concat_tanh"}
    assert sum(c["dense"] for c in genl) >= 1 and any(c["early"] for c in genl)
    import ref64_general as r64
    assert {c["problem"]["kind"] for c in C} == set(r64.KINDS)
    hb = lambda c: sum((h + 15) // 16 for h in c["net"]["arch"])
    assert {24, 25} <= {hb(c) for c in genl}
    assert all(c["solver"]["K"] <= 257 and c["solver"]["N"] <= 7 for c in C)


def test_philox_table_covers_the_routes():
    """PHILOX_CASES (tests/test_gpu_general_philox_blocks.py) reaches every forward instance that noise='philox' selects; no GPU
    call.  A specialised case must satisfy, in its own description, what GenLaunch::spec_kind asks of the launch."""
    P = gc.PHILOX_CASES
    assert all(c["noise"] == "philox" and c["solver"]["L"] == c["it"] + 1 for c in P)
    assert all(c["solver"]["K"] <= 257 and c["solver"]["N"] <= 7 for c in P)
    gen = [c for c in P if c["route"]["plan"] == "gen"]
    genl = [c for c in P if c["route"]["plan"] == "genl"]
    spec = [c for c in gen if c["route"]["spec"] is not None]
    off = [c for c in gen if c["route"]["spec"] is None]
    kinds = {gc.SPEC_ALLEN_CAHN: "AllenCahn", gc.SPEC_DWELL: "DoubleWell_multidim_for_general_solver"}
    for c in spec:                                               # unbounded, not adaptive, split products or bf16
        assert c["problem"]["kind"] == kinds[c["route"]["spec"]] and c["family"] == "general", c["id"]
        assert not c["solver"]["adaptive_forward_process"] and c["mode"] in ("f16x3", "bf16"), c["id"]
    for c in off:                                                # fp32 never specialises; else adaptive, bounded or another problem
        assert c["mode"] == "fp32" or c["solver"]["adaptive_forward_process"] or c["family"] != "general" \
            or c["problem"]["kind"] not in kinds.values(), c["id"]
    exact, padded = lambda c: c["route"]["inst"] in ((6, 30), (10, 24), (100, 64)), lambda c: c["route"]["inst"] in ((16, 32), (48, 48))
    for kind in kinds:
        x3 = [c for c in spec if c["route"]["spec"] == kind and c["mode"] == "f16x3"]
        assert any(exact(c) for c in x3) and any(padded(c) for c in x3), kind
        assert any(c["mode"] == "bf16" for c in spec if c["route"]["spec"] == kind), kind
        assert any(c["it"] == 1 for c in x3), kind
    assert {c["route"]["inst"] for c in spec if c["mode"] == "f16x3"} == {(6, 30), (10, 24), (16, 32), (48, 48), (100, 64)}
    assert {c["solver"]["K"] for c in spec} >= {1, 40, 257}
    assert {c["mode"] for c in off} == {"fp32", "f16x3"}
    assert {c["route"]["inst"] for c in off if c["mode"] == "f16x3"} == {(10, 24), (16, 32), (48, 48), (100, 64)}
    assert any(c["it"] == 1 for c in gen) and any(c["it"] == 1 for c in genl)          # iter = 1 on each plan
    base = {c["id"] for c in gc.CASES if c["route"]["plan"] == "genl"}
    assert {c["id"][len("philox-"):] for c in genl if c["it"] == 0} == base                # every run-time-shaped case
    assert {c["route"]["fwd"] for c in genl} == {1, 4, 8}
    assert sum(c["dense"] for c in genl) >= 3 and any(c["early"] for c in genl)
    d_in = {c["problem"]["kwargs"]["d"] + (0 if c["family"] == "elliptic" else 1) for c in genl}
    assert d_in >= {2, 16, 17, 112}, d_in
    assert {c["it"] for c in genl if c["problem"]["kwargs"]["d"] == 111} == {0, 1}       # seven noise blocks, the last holds 15
    for cid in gc.PHILOX_SHARD_IDS:
        assert gc.PHILOX_BY_ID[cid]["solver"]["K"] == 40 and gc.PHILOX_BY_ID[cid]["it"] == 0
    assert {gc.PHILOX_BY_ID[cid]["route"]["plan"] for cid in gc.PHILOX_SHARD_IDS} == {"gen", "genl"}
    assert gc.CASES == gc._templated() + gc._runtime_shaped()    # the supplied-noise table is what it was: nothing here edits it


# ---- c. planted errors -------------------------------------------------------------------------------------------------------------
def views(g, c):
    """[(W_i with rows = inputs, b_i)] as writable views of the flat gradient g of the case's net."""
    (d, time_input, arch), kw = gc.layout(c)
    dims = [d + (1 if time_input else 0)] + arch + [1]
    out, off = [], 0
    for i in range(1, len(dims)):
        fan, o = sum(dims[:i]), dims[i]
        W = g[off:off + fan * o]
        W = W.view(o, fan).t() if kw["linear"] else W.view(fan, o)
        out.append((W, g[off + fan * o:off + fan * o + o]))
        off += fan * o + o
    return out


def check_planted(what, g, c, where):
    """`where`: the block names the error sits in -- accepted by the flat criterion, rejected per block by a factor >= 10, and in no
    other block."""
    g_ref = gc.runs(c)["ref"]["grad"]
    lay, kw = gc.layout(c)
    names, errs = gc.general_block_errors(g, g_ref, *lay, **kw)
    flat = float((g - g_ref).abs().max()) / float(g_ref.abs().max())
    print("%s [%s]: flat %.2e (<= %.1e passes), blocks %s" % (what, c["id"], flat, FLAT_TOL,
          "  ".join("%s %.2e" % (n, e) for n, e in zip(names, errs) if n in where)))
    assert flat <= FLAT_TOL, (what, flat)
    assert {n for n, e in zip(names, errs) if e > 0.0} == set(where), (what, dict(zip(names, errs)))
    assert all(e >= 10 * BLOCK_TOL for n, e in zip(names, errs) if n in where), (what, dict(zip(names, errs)))
    with pytest.raises(AssertionError):
        gc.assert_general_blocks(g, g_ref, lay, BLOCK_TOL, tag=what, **kw)


def test_what_is_right_passes():
    c = gc.BY_ID["genl-d10-a110x17-relu2"]
    g_ref = gc.runs(c)["ref"]["grad"]
    lay, kw = gc.layout(c)
    gc.assert_general_blocks(g_ref.float(), g_ref, lay, BLOCK_TOL, tag="fp32 rounding of the reference", **kw)


WIDE, RAGGED = gc.PLANTED["plant-d2-a128x128"], gc.PLANTED["plant-d10-a24x24-K257"]


def test_planted_cases_keep_every_block_above_the_floor():
    for c in (WIDE, RAGGED):
        g = gc.runs(c)["ref"]["grad"]
        lay, kw = gc.layout(c)
        names, blocks = gc.general_grad_blocks(g, *lay, **kw)
        share = {n: float(b.abs().max()) / float(g.abs().max()) for n, b in zip(names, blocks)}
        print("%s: %s" % (c["id"], "  ".join("%s %.1e" % kv for kv in share.items())))
        assert min(share.values()) >= gc.BLOCK_FLOOR, share


def test_planted_time_row_scaled():
    """W1's time row x 1.3."""
    g = gc.runs(WIDE)["ref"]["grad"].clone()
    views(g, WIDE)[0][0][WIDE["problem"]["kwargs"]["d"]].mul_(1.3)
    check_planted("W1t x 1.3", g, WIDE, {"W1t"})


def tangent_part(c):
    """What the tangent pass contributes to the gradient: the reference minus the same iteration with grad_x V cut off the
    parameters (ref64_general.iteration(tangent=False)).  On a weight it is the a' zbar'^T outer products, on a hidden bias the
    phi'' term."""
    import ref64_general as r64
    run = gc.runs(c)
    V = gc.orc.general_build(run["oprob"], gc._oracle_config(c), net=c["net"])
    gc.prepare_net(c, V)
    return run["ref"]["grad"] - r64.iteration(c, run["oprob"], r64.net64(V), run["trace"], tangent=False)["grad"]


def test_planted_tangent_term_dropped_from_W2h1():
    g = gc.runs(WIDE)["ref"]["grad"].clone()
    d_in = WIDE["problem"]["kwargs"]["d"] + 1
    views(g, WIDE)[1][0][d_in:] -= views(tangent_part(WIDE), WIDE)[1][0][d_in:]
    check_planted("tangent term dropped from W2h1", g, WIDE, {"W2h1"})


def test_planted_wave_block_zeroed():
    """Hidden units 16 b .. 16 b + 15 of the 128-wide second layer zeroed in W2[h1]: the block of one wave of eight (the wave whose
    loss changes the whole gradient least)."""
    g_ref = gc.runs(WIDE)["ref"]["grad"]
    d_in = WIDE["problem"]["kwargs"]["d"] + 1
    W2_ref = views(g_ref, WIDE)[1][0]
    cols = [float(W2_ref[d_in:, 16 * b:16 * b + 16].abs().max()) for b in range(8)]
    b = cols.index(min(cols))
    g = g_ref.clone()
    views(g, WIDE)[1][0][d_in:, 16 * b:16 * b + 16] = 0.0
    check_planted("wave %d of eight zeroed in W2h1" % b, g, WIDE, {"W2h1"})


def test_planted_phi2_term_dropped_from_a_hidden_bias():
    g = gc.runs(RAGGED)["ref"]["grad"].clone()
    views(g, RAGGED)[0][1].sub_(views(tangent_part(RAGGED), RAGGED)[0][1])
    check_planted("phi'' term dropped from b1", g, RAGGED, {"b1"})


def test_planted_last_ragged_tile_left_out_of_W1x():
    """K = 257: the last tile holds one trajectory.  Its share of W1's x rows is the domain gradient of the same iteration on that
    trajectory alone, weighed 1 / K (the loss is a mean over the trajectories)."""
    import ref64_general as r64
    c = RAGGED
    run = gc.runs(c)
    tr, K = run["trace"], c["solver"]["K"]
    Kf = 16 * (K // 16)
    assert K - Kf == 1
    V = gc.orc.general_build(run["oprob"], gc._oracle_config(c), net=c["net"])
    gc.prepare_net(c, V)
    tail = dict(tr, X0=tr["X0"][Kf:], t0=tr["t0"][Kf:], xi=[x[Kf:] for x in tr["xi"]])
    cs = dict(c, solver=dict(c["solver"], K=K - Kf, K_boundary=1))
    g_tail = r64.iteration(cs, run["oprob"], r64.net64(V), tail)["grad_domain"] * (K - Kf) / K
    g = run["ref"]["grad"].clone()
    d = c["problem"]["kwargs"]["d"]
    views(g, c)[0][0][:d] -= views(g_tail, c)[0][0][:d]
    check_planted("last ragged tile left out of W1x", g, c, {"W1x"})
