"""Per-block gradient tests of the value-net kernels behind GeneralSolver.train / EllipticSolver.train -- the (d, H)-templated gen_*
kernels (csrc/gen_kernels.h, plan_general_native.py) and the run-time-shaped genl_* kernels (csrc/genl_kernels.h,
plan_general_deep.py) -- against the float64 reference tests/ref64_general.py.

Every other gradient assertion on this family is max |g - g_oracle| <= 5e-4 max |g_oracle| over the whole flat gradient against the
fp32 CPU oracle; the output layer sets that maximum, and a time row that is 30 % off, a hidden block without its tangent term or a
wave of eight that lost its slot pass it (tests/test_ref64_general.py plants five such errors).  Here the first native iteration
(backend='native', noise='reference', the path store filled with NaN first) of every case of tests/general_block_cases.py is
compared with the float64 reference on the same draws:
  gradient      every block of plan.grad (W{i}x, W{i}t, W{i}h{j}, b{i} per layer, the output layer included) to BLOCK_TOL = 2e-4 of
                the block's own maximum (floored at BLOCK_FLOOR = 1e-4 of the whole gradient's);
  end points    plan.YN, plan.VN, plan.XN, plan.tN per trajectory to D_TOL = 2e-5 max(1, max |.|) -- the fp32 oracle on the CPU is
                within 8.3e-7 (YN), 6.7e-7 (VN), 1.3e-7 (XN), 1.3e-8 (tN) of float64 over the cases (tests/test_ref64_general.py
                prints them), so no quantity needs a wider bound;
  loss          5e-5 relative;
  discrete      K_log exact; the run-time-shaped plan's per-tile step counts (_tile_steps) exact; for the templated plan, which keeps
                no per-tile count, the active steps per trajectory round((t_N - t_0) / dt) exact.
The CPU test asserts, on the reference alone, the margins that make the discrete results well defined (exit and time tests 1e-5
away from their thresholds, relu^2 pre-activations 8 e_fp32 of their dot product's absolute terms away from zero) and that the
kernels' part of every block is at least half of it.

Routes (asserted on the plan): the templated instances (6, 30), (10, 24), (100, 64) exact and (16, 32), (48, 48) padded -- one,
two, four and seven input blocks -- each under mlp_dtype 'fp32' and under the split-product forward that 'auto' selects
(range_fallbacks() == 0); K = 1, 16, 40, 257; elliptic with a Neumann boundary, a sphere with early exits, a box with
loss_with_stopped; BSDE and diffusion; adaptive and not.  The run-time-shaped kernels with 1, 4 and 8 forward waves per tile
(PSP_GENL_NW), the backward instances <1>, <8, 3> (HBsum 24) and <8, 4> (HBsum 25 and 32), depths 1 to 4, widths 1 .. 128, d_in 2,
16, 17 and 112, relu^2 / tanh^2 / tanh and the nn.Linear layout, a dense sigma (elliptic box, one-sided parabolic box, the full-Hessian ball), a sphere
whose trajectories all run out of time before step N, the BSDE loss with a Neumann boundary, the annulus and the cut corner; every h of the
native catalogue occurs.
The bf16 modes stay out (tests/general_block_cases.py says why).

d = 7, H = 20 runs on (10, 24), the cheapest instance that covers it, not on (16, 32): the case asserts what the plan takes.

Measured on an MI355X: end points within 1.1e-6 (YN), 9.4e-7 (VN), 1.4e-7 (XN), 1.3e-8 (tN), loss within 8.2e-7, and the worst block
error per route (bound 2e-4; the test prints them with the last case):
  gen<6, 30>/fp32     6.6e-7 (W1x)    gen<6, 30>/f16x3    4.9e-7 (W1t)    gen<10, 24>/fp32   1.8e-6 (W3x)    gen<10, 24>/f16x3  3.1e-6 (W3x)
  gen<16, 32>/fp32    3.5e-7 (W2h1)   gen<16, 32>/f16x3   4.3e-7 (W2h1)   gen<48, 48>/fp32   4.6e-7 (W2x)    gen<48, 48>/f16x3  1.7e-6 (W1t)
  gen<100, 64>/fp32   3.9e-7 (W1x)    gen<100, 64>/f16x3  4.0e-7 (W1x)
  genl fwd<1> + bwd<1>  4.1e-6 (W2x)    genl fwd<1> + bwd<1>, dense sigma  2.0e-6 (W3x)
  genl fwd<4> + bwd<8, 3>  6.7e-7 (W3h1)    genl fwd<8> + bwd<8, 3>  1.5e-6 (W3x)    genl fwd<8> + bwd<8, 4>  2.1e-6 (W4t)
i.e. every route, the split-product forward included, is at the fp32-against-float64 floor (the fp32 oracle itself: up to 5.0e-6,
tests/test_ref64_general.py).  No block comes within a factor 45 of the bound, and the file runs in 6 s.
"""
import pytest
import torch

import general_block_cases as gc
from test_general_composite_golden import build as build_pkg
from test_gpu_genl_fuzz import expected_geometry
from util_cases import flat_params, psp

pytestmark = pytest.mark.gpu
nat = psp.native

BLOCK_TOL = 2e-4            # each gradient block, of that block's own maximum
D_TOL = 2e-5                # per-trajectory end points: |diff| <= D_TOL * max(1, max |.|)
LOSS_TOL = 5e-5


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def run_case(c, monkeypatch):
    """The first iteration of the case on the GPU: (model, plan, float64 reference run)."""
    run = gc.runs(c)                                                       # before the build: both sides seed numpy for the box batches
    if c["nw"] is None:
        monkeypatch.delenv("PSP_GENL_NW", raising=False)
    else:
        monkeypatch.setenv("PSP_GENL_NW", c["nw"])
    over = dict(mlp_dtype="fp32" if c["mode"] == "fp32" else "auto")
    case = dict(name=c["name"], family=c["family"], problem=c["problem"], solver=c["solver"], net=c["net"])
    if "numpy_seed" in c:
        case["numpy_seed"] = c["numpy_seed"]
    prob, model = build_pkg(case, device=dev(), backend="native", noise="reference", **over)
    gc.prepare_net(c, model.V)
    assert torch.equal(flat_params(model.V).double(), torch.cat([p.detach().reshape(-1) for p in run["net"]["params"]]))
    plan = model._choose_plan()
    assert model.plan_name == "native", getattr(model, "plan_reason", None)
    plan.path.fill_(float("nan"))                                          # a slot read without having been written fails here
    model.train()
    assert model._gen_plan is plan
    torch.cuda.synchronize()
    return model, plan, run


def assert_route(c, plan):
    """The route of the case, and its name in the table of worst errors."""
    r = c["route"]
    if r["plan"] == "gen":
        assert type(plan).__name__ == "GeneralNativePlan", type(plan).__name__
        assert (plan.d_pad, plan.H_pad) == r["inst"], (plan.d_pad, plan.H_pad)
        assert plan.matrix_mode == r["mode"], plan.matrix_mode
        assert plan.range_fallbacks() == 0                                 # in range: the split kernels did the work
        return "gen<%d, %d>/%s" % (r["inst"] + (r["mode"],))
    assert type(plan).__name__ == "GeneralDeepPlan", type(plan).__name__
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    d_in = c["problem"]["kwargs"]["d"] + (0 if c["family"] == "elliptic" else 1)
    assert int(plan.sizes.waves_per_tile) == r["fwd"], (int(plan.sizes.waves_per_tile), r)
    assert expected_geometry(d_in, c["net"]["arch"], plan.K_local, c["nw"], cus) == (r["fwd"], r["bwd"])
    dense = c["dense"]
    assert (plan.gcfg.sigma_kind == nat.GENL_SIGMA_DENSE) == dense
    return "genl fwd<%d> + %s%s" % (r["fwd"], r["bwd"][5:], " dense sigma" if dense else "")


WORST = {}                   # route -> (largest block error, block, case id): printed by the last case of the module
WORST_PT = dict(YN=0.0, VN=0.0, XN=0.0, tN=0.0, loss=0.0)


@pytest.mark.parametrize("c", gc.CASES, ids=[c["id"] for c in gc.CASES])
def test_first_iteration_blocks_match_the_float64_reference(c, monkeypatch):
    model, plan, run = run_case(c, monkeypatch)
    route = assert_route(c, plan)
    ref = run["ref"]
    K = ref["YN"].shape[0]
    # ---- discrete results
    assert model.K_log == [ref["K_count"]], (model.K_log, ref["K_count"])
    if c["route"]["plan"] == "genl":
        assert torch.equal(plan._tile_steps().cpu().long(), ref["tile_steps"]), (plan._tile_steps().cpu(), ref["tile_steps"])
    tN = plan.tN.double().cpu()
    t0 = torch.zeros(K, dtype=torch.float64) if c["family"] == "elliptic" else run["trace"]["t0"].double().reshape(K)
    assert torch.equal(torch.round((tN - t0) / plan.cfg.dt).long(), ref["steps"])
    # ---- per-trajectory end points, loss
    errs = {}
    for name, got in (("YN", plan.YN), ("VN", plan.VN), ("XN", plan.XN), ("tN", plan.tN)):
        got, want = got.double().cpu(), ref[name]
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), name
        errs[name] = float((got - want).abs().max()) / max(1.0, float(want.abs().max()))
    errs["loss"] = abs(model.loss_log[0] - ref["loss"]) / abs(ref["loss"])
    print("%s [%s]: %s" % (c["id"], route, "  ".join("%s %.2e" % kv for kv in errs.items())))
    for k, v in errs.items():
        WORST_PT[k] = max(WORST_PT[k], v)
    g = plan.grad.cpu()
    assert g.shape == ref["grad"].shape and bool(torch.isfinite(g).all())
    lay, kw = gc.layout(c)
    try:
        names, be = gc.assert_general_blocks(g, ref["grad"], lay, BLOCK_TOL, tag=c["id"], **kw)
        worst = max(be)
        if worst > WORST.get(route, (-1.0,))[0]:
            WORST[route] = (worst, names[be.index(worst)], c["id"])
        assert all(errs[k] <= D_TOL for k in ("YN", "VN", "XN", "tN")), errs
        assert errs["loss"] <= LOSS_TOL, (model.loss_log[0], ref["loss"])
    finally:
        if c is gc.CASES[-1]:
            for rt, (e, blk, cid) in sorted(WORST.items()):
                print("worst block per route: %-44s %.2e (%s) %s" % (rt, e, blk, cid))
            print("worst per trajectory / loss: %s" % "  ".join("%s %.2e" % kv for kv in WORST_PT.items()))
