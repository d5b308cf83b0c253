"""Per-block gradient tests of the value-net kernels behind GeneralSolver.train / EllipticSolver.train ON THEIR OWN PHILOX NOISE
(noise='philox': production, and every general workload of bench.py) against the float64 reference tests/ref64_general.py.

tests/test_gpu_general_block_gradients.py judges the same two kernel families with noise='reference', where the templated forward is
gen_fwd_kernel<D, H, BF16, /*PHILOX*/false, X3, /*SPECK*/-1> and genl_fwd_kernel reads the noise it is handed.  On Philox noise OTHER
compiled kernels run (csrc/gen_kernels.h GenLaunch::fwd, fwd_x3, fwd_bf16):
  gen_fwd_kernel<D, H, false, true> and <D, H, false, true, true>   the PHILOX instances (fp32 MFMA, split products);
  gen_fwd_kernel<D, H, BF16, true, X3, SPECK>   the specialised instances, SPECK = DRIFT_ZERO | GH_ALLEN_CAHN << 4 or DRIFT_DWELL |
      GH_QUAD << 4, taken under split products and bf16 when the domain is unbounded, the process not adaptive and store_path == 1
      (GenLaunch::spec_kind) -- spec<100, 64> with DWELL|QUAD under split products is what bench.py times at d = 100;
  genl_fwd_kernel   the run-time branch that draws from the counters (lo + k, n, 4 b + q, iter, seed), masks the padded features of
      the last noise block (16 b + 4 r + q >= d) and multiplies by a dense sigma.

How.  Two bound methods of the plan are wrapped with pass-through recorders (record_iterations): _launch_fwd, the one launch point,
keeps X_0, t_0 and the flat parameters of every iteration (and asserts that no noise is handed over); _boundary_terms keeps the
boundary batch and its times.  The stream the kernels draw from is materialised by psp_philox_normal_fill(N, K, d_real, k_offset,
seed, iter) -- its slice n + 1 is the value-net kernels' step n --, and ref64_general.iteration runs on these draws with the float64
net of the recorded parameters.  Every case of general_block_cases.PHILOX_CASES trains L iterations (backend='native', the path store
filled with NaN first) and the LAST is judged with the sibling's bounds, imported from it:
  gradient      every block of plan.grad to BLOCK_TOL = 2e-4 of the block's own maximum;
  end points    YN, VN, XN, tN per trajectory to D_TOL = 2e-5 max(1, max |.|);
  loss          LOSS_TOL = 5e-5 relative;
  discrete      K_log, the run-time-shaped plan's _tile_steps() and the active steps per trajectory exact.
The bf16 cases are judged by the bf16 modes' documented bound (tests/test_gpu_general_variants.py): loss and whole gradient
within 2e-2 -- and XN, tN to D_TOL all the same: without the adaptive shift the state never passes through a bf16 product, so they
pin the noise of the bf16 SPECK instances as tightly as the others'.
The conditions on the reference alone (tests/test_ref64_general.py::test_cases_satisfy_the_conditions: no block under the floor, the
kernels' part of every block at least half of it, exit / time margins 1e-5, relu^2 margin 8 e_fp32) are asserted FIRST, here: X_0
and t_0 come from a device generator in this mode, so no CPU test can evaluate them.  A case that misses them gets another seed,
scale or alpha in the table, never a wider bound.

Routes, asserted on the plan: cfg.noise_mode == NOISE_PHILOX, (d_pad, H_pad), matrix_mode, range_fallbacks() == 0, and for the
templated plan the predicate of GenLaunch::spec_kind read off plan.cfg (domain_kind == DOM_NONE, adaptive == 0, store_path == 1, no
per-step value output, the (drift_kind, h_kind) pair, a split-product or bf16 mode, PSP_NO_SPEC not in the environment): it names
the SPECK kind of a specialised case and is false for every other.  iter = 1 reaches the kernels in the L = 2 cases (a wrong
counter gives unrelated noise there), one per specialised kind and two on the run-time-shaped kernels (four waves; d = 111, seven
noise blocks, the last with 15 features).

test_shard_at_an_offset_that_is_no_multiple_of_16 launches the forward on rows 20 .. 39 of a K = 40 batch alone (cfg.k_offset = 20,
the recorded x0 and t0 of those rows) and compares YN, VN, XN, tN with those rows of the float64 reference -- and with the full
run's rows, which they equal bit for bit on both kernel families.

What the first run found.  Every fp32 and split-product route was at the fp32 floor at once, and every case met its conditions with
the seeds of the supplied-noise table.  The bf16 case on (10, 24) was not: V_N 0.42, loss 0.28, gradient 0.51 off -- with X_N and
t_N at 5e-8, so the noise was right.  The same errors came from the general bf16 instance and on supplied noise: not the SPECK
instance but the bf16 mode on d + 1 <= 12.  There the bf16 image of an input-side weight table (one k-step of 32 = 256 floats per
row block) is larger than its fp32 image (KSI = 2 or 3 k-steps of 64 floats), by which alone GGeo carved the LDS: the table ran 128
(d + 1 = 9 .. 12) or 256 floats (d + 1 <= 8) into the next one, whose staging overwrote them -- hidden units 16 .. of W1 and W2x
read the other table's weights.  GGeo::tbl now sizes a table for the larger image; (10, 24) then gives V_N 5.6e-3, loss 9.1e-4,
gradient 3.1e-3, and with unscaled weights V_N 2.3e-4, which is what bf16 operand rounding of this net predicts in float64 (2.2e-4).
The table carries a third bf16 case for it: (6, 30), the other overrun.  The existing bf16 tests compare losses to 2 % and gradient
directions on the golden cases ((10, 32) among them, which overran as well) and had not noticed.

Measured on an MI355X (37 cases and the two shard runs in under 6 s): end points within 4.6e-7 (YN), 4.6e-7 (VN), 1.3e-7 (XN), 1.3e-8
(tN), loss within 8.2e-7, and the worst block error per route (bound 2e-4; the test prints them with the last case):
  spec<6, 30>/f16x3 ZERO|ALLEN_CAHN   5.9e-7 (W2h1)    spec<10, 24>/f16x3 ZERO|ALLEN_CAHN   6.6e-7 (W1x, iter = 1)
  spec<16, 32>/f16x3 ZERO|ALLEN_CAHN  4.7e-7 (W1t)     spec<48, 48>/f16x3 DWELL|QUAD        5.9e-7 (W1x)
  spec<100, 64>/f16x3 DWELL|QUAD      4.2e-7 (W1x)
  gen<6, 30>/fp32, philox    4.3e-7 (W1x)    gen<10, 24>/fp32, philox    4.2e-6 (W3x)    gen<10, 24>/f16x3, philox   6.0e-7 (W1t)
  gen<16, 32>/f16x3, philox  2.8e-7 (W2h1)   gen<48, 48>/f16x3, philox   1.1e-6 (W1t)    gen<100, 64>/f16x3, philox  3.8e-7 (W1x)
  genl fwd<1> + bwd<1>, philox  2.5e-6 (W1x)    genl fwd<1> + bwd<1> dense sigma, philox  6.2e-6 (W3x)
  genl fwd<4> + bwd<8, 3>, philox  4.9e-7 (W3h1)    genl fwd<8> + bwd<8, 3>, philox  1.2e-5 (b3)    genl fwd<8> + bwd<8, 4>, philox  2.2e-6 (W3x)
The bf16 pair beside them (bound 2e-2 on loss and whole gradient, D_TOL on XN and tN): spec<10, 24>/bf16 ZERO|ALLEN_CAHN loss 9.1e-4,
gradient 3.1e-3, worst block 1.4e-2 (W2h1); spec<100, 64>/bf16 DWELL|QUAD loss 3.6e-5, gradient 2.5e-3, worst block 6.8e-3 (W1x);
spec<6, 30>/bf16 ZERO|ALLEN_CAHN loss 2.2e-3, gradient 8.4e-3, worst block 1.3e-2 (W2h1); XN within 1.3e-7 and tN within 1.3e-8 on
all three.  I.e. on their own noise the kernels are where they are on supplied noise (tests/test_gpu_general_block_gradients.py):
no fp32 or split-product block comes within a factor 16 of the bound.
"""
import copy
import os

import pytest
import torch

import general_block_cases as gc
import ref64_general as r64
from test_general_composite_golden import build as build_pkg
from test_gpu_general_block_gradients import BLOCK_TOL, D_TOL, LOSS_TOL, assert_route, dev
from test_ref64_general import MIN_MARGIN, RELU_MARGIN
from util_cases import psp

pytestmark = pytest.mark.gpu
nat = psp.native

BF16_TOL = 2e-2             # loss and whole gradient of the bf16 modes (tests/test_gpu_general_variants.py)
IDS = [c["id"] for c in gc.PHILOX_CASES]


# ---- the draws of a Philox iteration, recorded ---------------------------------------------------------------------------------------
def record_iterations(plan, monkeypatch):
    """Wraps plan._launch_fwd and plan._boundary_terms (on the instance) with recorders that change nothing they do.  Returns the
    dict they fill: iteration l -> dict(x0 (K, d), t0 (K,), flat (the parameters BEFORE that iteration's Adam step), X_b, t_b)."""
    rec, pending = {}, {}
    launch, boundary = plan._launch_fwd, plan._boundary_terms
    keep = lambda t: None if t is None else t.detach().clone()

    def launch_fwd(flat_k, x0, t0, xi, l, st):
        assert xi is None, "noise='philox' hands no noise to the kernels"
        assert l not in rec
        rec[l] = dict(x0=x0[:, :plan.s.d].clone(), t0=t0.clone(), flat=plan.flat.clone(), X_b=pending.pop("X_b", None),
                      t_b=pending.pop("t_b", None))
        return launch(flat_k, x0, t0, xi, l, st)

    def boundary_terms(X, X_b, t_b):
        pending.update(X_b=keep(X_b), t_b=keep(t_b))
        return boundary(X, X_b, t_b)

    monkeypatch.setattr(plan, "_launch_fwd", launch_fwd)
    monkeypatch.setattr(plan, "_boundary_terms", boundary_terms)
    return rec


def philox_xi(N, K, d, k_offset, seed, it):
    """(N, K, d): the normals of steps 0 .. N - 1 of trajectories k_offset .. k_offset + K - 1 in iteration `it`, as the library
    materialises the kernels' stream.  Slice 0 of the fill is the tanh-net family's unused slot."""
    xi = torch.empty(N + 1, K, d, device=dev())
    nat.check(nat.load().psp_philox_normal_fill(nat.ptr(xi), N, K, d, k_offset, seed, it, None), "psp_philox_normal_fill")
    torch.cuda.synchronize()
    return xi[1:].cpu()


def draws_of(r, plan, model, it):
    """The `draws` of ref64_general.iteration from the record r of iteration `it`.  K is the recorded batch size (the annulus
    problem's rejection step sets it)."""
    K = r["x0"].shape[0]
    cpu = lambda t: None if t is None else t.cpu()
    return dict(X0=r["x0"].cpu(), t0=r["t0"].cpu(), X_boundary=cpu(r["X_b"]), t_b=cpu(r["t_b"]),
                xi=philox_xi(model.N, K, model.d, plan.lo, int(model.seed), it))


# ---- conditions on the reference, route ----------------------------------------------------------------------------------------------
def conditions(c, ref):
    """(one line of figures, the violated conditions) -- what tests/test_ref64_general.py::test_cases_satisfy_the_conditions asserts
    of the supplied-noise table, on the reference of THESE draws."""
    lay, kw = gc.layout(c)
    names, blocks = gc.general_grad_blocks(ref["grad"], *lay, **kw)
    _, dom = gc.general_grad_blocks(ref["grad_domain"], *lay, **kw)
    gmax = float(ref["grad"].abs().max())
    share = {n: float(b.abs().max()) / gmax for n, b in zip(names, blocks)}
    domain = {n: float(q.abs().max()) / max(float(b.abs().max()), 1e-300) for n, b, q in zip(names, blocks, dom)}
    m, ts = ref["margins"], ref["tile_steps"]
    line = ("smallest block %.2e (%s)  smallest domain part %.2f (%s)  margins exit %.1e time %.1e relu %.1e  K_count %d  tile steps "
            "%d..%d  loop %d" % (min(share.values()), min(share, key=share.get), min(domain.values()), min(domain, key=domain.get),
                                 m["exit"], m["time"], m["relu"], ref["K_count"], int(ts.min()), int(ts.max()), ref["n_loop"]))
    bad = []
    if not all(v >= gc.BLOCK_FLOOR for v in share.values()):
        bad.append("a block under the floor: %s" % {n: "%.1e" % v for n, v in share.items() if not v >= gc.BLOCK_FLOOR})
    if not all(v >= 0.5 for v in domain.values()):
        bad.append("the kernels' part under half: %s" % {n: "%.2f" % v for n, v in domain.items() if not v >= 0.5})
    if not (m["exit"] >= MIN_MARGIN and m["time"] >= MIN_MARGIN):
        bad.append("exit / time margin %.1e / %.1e" % (m["exit"], m["time"]))
    if not m["relu"] >= RELU_MARGIN:
        bad.append("relu margin %.1e" % m["relu"])
    if not (ref["K_count"] > 0 and ref["loss"] == ref["loss"] and abs(ref["loss"]) < float("inf")):
        bad.append("no active step, or a non-finite loss")
    if c["early"] and not (int(ts.min()) < int(ts.max()) or ref["n_loop"] < c["solver"]["N"]):
        bad.append("no tile leaves the time loop early")
    if c["solver"]["loss_with_stopped"] and not bool((ref["steps"] < c["solver"]["N"]).any()):
        bad.append("no stopped trajectory")
    return line, bad


def spec_kind(plan):
    """GenLaunch::spec_kind (csrc/gen_kernels.h) read off the plan: the SPECK kind of the specialised forward instance the launch
    takes, or None.  Only fwd_x3 and fwd_bf16 consult it (psp_gen_rollout_fwd: every mlp_dtype but fp32)."""
    cfg = plan.cfg
    if type(plan).__name__ != "GeneralNativePlan" or plan.matrix_mode == "fp32":
        return None
    if os.environ.get("PSP_NO_SPEC", "")[:1] == "1" or cfg.noise_mode != nat.NOISE_PHILOX or cfg.domain_kind != nat.DOM_NONE \
            or cfg.adaptive != 0 or cfg.store_path != 1 or cfg.v_steps_out:
        return None
    return {(nat.DRIFT_DOUBLE_WELL, nat.GH_QUAD): gc.SPEC_DWELL,
            (nat.DRIFT_ZERO, nat.GH_ALLEN_CAHN): gc.SPEC_ALLEN_CAHN}.get((cfg.drift_kind, cfg.h_kind))


def assert_philox_route(c, plan):
    """The sibling's route (plan, instance, matrix mode, no range fall-back; waves, backward instance, sigma kind) on Philox noise,
    and whether the launch takes a specialised instance.  Returns the route's name in the table of worst errors."""
    name = assert_route(c, plan)
    assert plan.cfg.noise_mode == nat.NOISE_PHILOX, plan.cfg.noise_mode
    want = c["route"]["spec"]
    assert want is None or "PSP_NO_SPEC" not in os.environ
    assert spec_kind(plan) == want, (spec_kind(plan), want)
    if want is None:
        return name + ", philox"
    return "spec<%d, %d>/%s %s" % (c["route"]["inst"] + (c["route"]["mode"], want))


# ---- one case ------------------------------------------------------------------------------------------------------------------------
def build_case(c, monkeypatch, **over):
    """(model, plan) of the case on backend='native', noise='philox', the nets prepared as the reference's."""
    if c["nw"] is None:
        monkeypatch.delenv("PSP_GENL_NW", raising=False)
    else:
        monkeypatch.setenv("PSP_GENL_NW", c["nw"])
    over.setdefault("mlp_dtype", c["mode"] if c["mode"] in ("fp32", "bf16") else "auto")
    case = dict(name=c["name"], family=c["family"], problem=c["problem"], solver=c["solver"], net=c["net"])
    if "numpy_seed" in c:
        case["numpy_seed"] = c["numpy_seed"]
    prob, model = build_pkg(case, device=dev(), backend="native", noise="philox", **over)
    gc.prepare_net(c, model.V)
    plan = model._choose_plan()
    assert model.plan_name == "native", getattr(model, "plan_reason", None)
    return model, plan


def run_case(c, monkeypatch):
    """L = it + 1 iterations of the case on the GPU: (model, plan, the record of every iteration, the float64 reference of
    iteration `it` on the recorded draws)."""
    model, plan = build_case(c, monkeypatch)
    rec = record_iterations(plan, monkeypatch)
    plan.path.fill_(float("nan"))                                          # a slot read without having been written fails here
    model.train()
    assert model._gen_plan is plan
    torch.cuda.synchronize()
    it = c["it"]
    assert sorted(rec) == list(range(it + 1)), sorted(rec)
    oprob, net0 = gc.reference_net(c)
    assert torch.equal(rec[0]["flat"].double().cpu(), r64.flat(net0["params"]).detach())        # the same net on both sides
    oprob, net = (oprob, net0) if it == 0 else gc.reference_net(c, rec[it]["flat"])
    ref = r64.iteration(c, oprob, net, draws_of(rec[it], plan, model, it))
    return model, plan, rec, ref


def end_point_errors(got, ref, rows=slice(None)):
    """{quantity: max |kernel - float64| / max(1, max |float64|)} over the trajectories `rows` of the reference."""
    errs = {}
    for name in ("YN", "VN", "XN", "tN"):
        g, want = got[name].double().cpu(), ref[name][rows]
        assert g.shape == want.shape and bool(torch.isfinite(g).all()), name
        errs[name] = float((g - want).abs().max()) / max(1.0, float(want.abs().max()))
    return errs


WORST = {}                   # route -> (largest block error, block, case id): printed by the last case of the module
WORST_PT = dict(YN=0.0, VN=0.0, XN=0.0, tN=0.0, loss=0.0)
WORST_BF16 = dict(YN=0.0, VN=0.0, XN=0.0, tN=0.0, loss=0.0, grad=0.0)


@pytest.mark.parametrize("c", gc.PHILOX_CASES, ids=IDS)
def test_philox_iteration_blocks_match_the_float64_reference(c, monkeypatch):
    model, plan, rec, ref = run_case(c, monkeypatch)
    it = c["it"]
    line, bad = conditions(c, ref)
    print("%s: %s" % (c["id"], line))
    assert not bad, (c["id"], bad)                                         # the case, not the kernel: another seed, scale or alpha
    route = assert_philox_route(c, plan)
    bf16 = c["mode"] == "bf16"
    K = ref["YN"].shape[0]
    assert plan.K_local == K
    # ---- discrete results
    assert model.K_log[it] == ref["K_count"], (model.K_log, ref["K_count"])
    if c["route"]["plan"] == "genl":
        assert torch.equal(plan._tile_steps().cpu().long(), ref["tile_steps"]), (plan._tile_steps().cpu(), ref["tile_steps"])
    t0 = torch.zeros(K, dtype=torch.float64) if c["family"] == "elliptic" else rec[it]["t0"].double().cpu().reshape(K)
    assert torch.equal(torch.round((plan.tN.double().cpu() - t0) / plan.cfg.dt).long(), ref["steps"])
    # ---- per-trajectory end points, loss
    errs = end_point_errors(dict(YN=plan.YN, VN=plan.VN, XN=plan.XN, tN=plan.tN), ref)
    errs["loss"] = abs(model.loss_log[it] - ref["loss"]) / abs(ref["loss"])
    g = plan.grad.cpu()
    assert g.shape == ref["grad"].shape and bool(torch.isfinite(g).all())
    if bf16:
        errs["grad"] = float((g.double() - ref["grad"]).abs().max()) / float(ref["grad"].abs().max())
    print("%s [%s]: %s" % (c["id"], route, "  ".join("%s %.2e" % kv for kv in errs.items())))
    worst_pt = WORST_BF16 if bf16 else WORST_PT
    for k, v in errs.items():
        worst_pt[k] = max(worst_pt[k], v)
    lay, kw = gc.layout(c)
    try:
        names, be = gc.assert_general_blocks(g, ref["grad"], lay, float("inf") if bf16 else BLOCK_TOL, tag=c["id"], **kw)
        worst = max(be)
        if worst > WORST.get(route, (-1.0,))[0]:
            WORST[route] = (worst, names[be.index(worst)], c["id"])
        if bf16:
            assert errs["grad"] <= BF16_TOL and errs["loss"] <= BF16_TOL, errs
            assert errs["XN"] <= D_TOL and errs["tN"] <= D_TOL, errs
        else:
            assert all(errs[k] <= D_TOL for k in ("YN", "VN", "XN", "tN")), errs
            assert errs["loss"] <= LOSS_TOL, (model.loss_log[it], ref["loss"])
    finally:
        if c is gc.PHILOX_CASES[-1]:
            for rt, (e, blk, cid) in sorted(WORST.items()):
                print("worst block per route: %-52s %.2e (%s) %s" % (rt, e, blk, cid))
            print("worst per trajectory / loss: %s" % "  ".join("%s %.2e" % kv for kv in WORST_PT.items()))
            print("worst of the bf16 cases: %s" % "  ".join("%s %.2e" % kv for kv in WORST_BF16.items()))


@pytest.mark.parametrize("cid", gc.PHILOX_SHARD_IDS)
def test_shard_at_an_offset_that_is_no_multiple_of_16(cid, monkeypatch):
    """Rows 20 .. 39 of a K = 40 batch run alone through the C ABI (cfg.k_offset = 20, their recorded x0 and t0) reproduce those rows
    of the float64 reference of the whole batch: the trajectory counter is k_offset + k whatever the tile a row falls into."""
    c = gc.PHILOX_BY_ID[cid]
    lo, K = 20, c["solver"]["K"]
    assert K == 40 and c["it"] == 0
    model, plan, rec, ref = run_case(c, monkeypatch)
    line, bad = conditions(c, ref)
    assert not bad, (cid, bad)
    full = {n: getattr(plan, n).clone() for n in ("YN", "VN", "XN", "tN")}
    half = copy.deepcopy(c)
    half["solver"].update(K=K - lo, K_boundary=min(c["solver"]["K_boundary"], K - lo))
    model2, plan2 = build_case(half, monkeypatch)
    assert type(plan2) is type(plan) and (plan2.d_pad, plan2.H_pad, plan2.matrix_mode) == (plan.d_pad, plan.H_pad, plan.matrix_mode)
    assert spec_kind(plan2) == c["route"]["spec"] and plan2.K_local == K - lo
    r = rec[0]
    plan2.flat.copy_(r["flat"])
    plan2.cfg.k_offset = lo
    plan2.kcount.zero_()
    x0 = plan2.pad.last_dim(r["x0"][lo:].contiguous())
    t0 = r["t0"][lo:].contiguous()
    plan2._launch_fwd(plan2.pad.scatter_params(plan2.flat, plan2.flat_k), x0, t0, None, 0, nat.stream_ptr(dev()))
    torch.cuda.synchronize()
    assert plan2.range_fallbacks() == 0
    got = dict(YN=plan2.YN, VN=plan2.VN, XN=plan2.XN, tN=plan2.tN)
    errs = end_point_errors(got, ref, slice(lo, K))
    same = {n: torch.equal(got[n], full[n][lo:]) for n in got}
    print("%s rows %d..%d alone: %s;  bit for bit the full run's rows: %s" % (cid, lo, K - 1, "  ".join("%s %.2e" % kv for kv in errs.items()),
                                                                            same))
    assert all(v <= D_TOL for v in errs.values()), errs
    assert all(same.values()), same                                        # (measured to hold: a row's results do not depend on its tile)
    assert int(plan2.kcount.item()) == int(ref["steps"][lo:].sum())
