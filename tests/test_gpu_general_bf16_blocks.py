"""GeneralSolver(mlp_dtype='bf16_fwd') -- gen_fwd_kernel<D, H, /*BF16*/true, ..> and the fp32 gen_bwd2_kernel behind it -- and
mlp_dtype='bf16' -- the same forward and the bf16 gen_bwd2_kernel -- against a float64 reference that rounds what the kernels round
(tests/ref64_general.py: iteration(..., operands='bf16'[, backward='bf16'])), block by block.

Every judged quantity q (Y_N, V_N, X_N, t_N per trajectory, the loss, every gradient block of general_block_cases) has three values:
q_exact (float64), q_model (float64 on the kernels' three sweeps with both operands of every product rounded to bf16) and q_kernel.
With e_model = |q_model - q_exact| and e_kernel = |q_kernel - q_model| in the normalisation of the fp32 sibling
(tests/test_gpu_general_block_gradients.py),

    e_kernel <= 1/2 e_model + (the sibling's bound: end points 2e-5, loss 5e-5, each block 2e-4);

for the loss e_model is max(e_model(loss), e_model(Y_N)); X_N and t_N keep the plain fp32 bound where no bf16 product reaches the
state (no adaptive shift); K_log and the active steps per trajectory are exact.  1/2 is the reference's figure, not the kernels': the
torch stand-in of tests/test_ref64_general_bf16.py (fp32 arithmetic on bf16-rounded operands) stays within 0.01 e_model on every
case, one product in nine left unrounded misses the bound, and the table overrun that GGeo::tbl ended cost about 100 e_model.

Cases (general_block_cases.BF16_CASES).  Supplied noise, on the fp32 oracle's draws: the exact (6, 30), (10, 24), (10, 32), whose
input-side bf16 tables are larger than the fp32 ones; (16, 16); d = 33, H = 40 on (48, 48).  Philox noise, on the recorded draws
(tests/test_gpu_general_philox_blocks.py): the SPECK instances ZERO|ALLEN_CAHN and DWELL|QUAD at (100, 64); off the specialisation
the adaptive shift at (10, 24) and a sphere with early exits at (48, 48).  The conditions on the exact reference are asserted first.

The full 'bf16' mode (bf16 backward, bf16-pair path store; BF16_FULL_CASES: every case again, and K = 299 over N = 20 steps, a hundred
backward rounds with a ragged last tile) launches the same forward instance with path16 set: its Y_N, V_N, X_N, t_N and loss equal
the 'bf16_fwd' run's bit for bit (asserted on one case per noise mode).  Its gradient is judged by the same criterion against
ref64_general.kernel_backward(rounded=True): gen_bwd2_kernel<D, H, /*BF16*/true> written out with its rounding points -- the stored
images (pk_bf16), both operands of the adjoint products and of the outer products.  DenseNet_tanh and every other net of the
run-time-shaped genl_* kernels decline both bf16 modes (asserted).

Measured on an MI355X (42 tests of the two bf16 files in 6.1 s), worst e_kernel / e_model per route (the test prints them): Y_N, V_N
and the loss below 0.0005 on every route of both modes.  Worst block, 'bf16_fwd': 0.005 (b3, gen<48, 48> on Philox noise with the
sphere), 0.004 (b3, spec<100, 64> DWELL|QUAD), below 0.0005 on gen<6, 30>, gen<10, 24> (both noise modes), gen<10, 32>, gen<16, 16>,
gen<48, 48> on supplied noise and spec<100, 64> ZERO|ALLEN_CAHN.  Worst block, 'bf16': 0.005 (b3, gen<48, 48> sphere), 0.004 (b3,
spec<100, 64> DWELL|QUAD; W1x, spec<100, 64> ZERO|ALLEN_CAHN), 0.001 (W2x, gen<6, 30>; W3t, gen<10, 24> Philox), below 0.0005
elsewhere, the K = 299, N = 20 case included.  The kernels are the model to fp32 rounding, a hundred times inside the bound.
"""
import pytest
import torch

import general_block_cases as gc
import ref64_general as r64
from test_general_composite_golden import build as build_pkg
from test_gpu_general_block_gradients import BLOCK_TOL, D_TOL, LOSS_TOL, assert_route, dev
from test_gpu_general_philox_blocks import assert_philox_route, build_case, conditions, draws_of, record_iterations
from util_cases import flat_params

pytestmark = pytest.mark.gpu
ALL = gc.BF16_CASES + gc.BF16_FULL_CASES
IDS = [c["id"] for c in ALL]


def run_supplied(c, monkeypatch, mode):
    """The first iteration on the fp32 oracle's draws (noise='reference'): (model, plan, draws, float64 net, oracle problem)."""
    run = gc.runs(c)                                                       # before the build: both sides seed numpy
    monkeypatch.delenv("PSP_GENL_NW", raising=False)
    case = dict(name=c["name"], family=c["family"], problem=c["problem"], solver=c["solver"], net=c["net"])
    prob, model = build_pkg(case, device=dev(), backend="native", noise="reference", mlp_dtype=mode)
    gc.prepare_net(c, model.V)
    assert torch.equal(flat_params(model.V).double(), torch.cat([p.detach().reshape(-1) for p in run["net"]["params"]]))
    plan = model._choose_plan()
    assert model.plan_name == "native", getattr(model, "plan_reason", None)
    plan.path.fill_(float("nan"))
    model.train()
    torch.cuda.synchronize()
    return model, plan, run["trace"], run["net"], run["oprob"]


def run_philox(c, monkeypatch, mode):
    model, plan = build_case(c, monkeypatch, mlp_dtype=mode)
    rec = record_iterations(plan, monkeypatch)
    plan.path.fill_(float("nan"))
    model.train()
    torch.cuda.synchronize()
    assert sorted(rec) == [0] and c["it"] == 0
    oprob, net = gc.reference_net(c)
    assert torch.equal(rec[0]["flat"].double().cpu(), r64.flat(net["params"]).detach())
    return model, plan, draws_of(rec[0], plan, model, 0), net, oprob


def run(c, monkeypatch, mode):
    return (run_philox if c["noise"] == "philox" else run_supplied)(c, monkeypatch, mode)


def results(model, plan):
    return dict(YN=plan.YN.clone(), VN=plan.VN.clone(), XN=plan.XN.clone(), tN=plan.tN.clone(), loss=float(model.loss_log[0]),
                grad=plan.grad.cpu())


WORST = {}                   # route -> {quantity: (largest e_kernel / e_model, name)}: printed by the last case of the module


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_bf16_iteration_matches_the_float64_bf16_operand_reference(c, monkeypatch):
    model, plan, draws, net, oprob = run(c, monkeypatch, c["mode"])
    exact = r64.iteration(c, oprob, net, draws)
    line, bad = conditions(c, exact)
    print("%s: %s" % (c["id"], line))
    assert not bad, (c["id"], bad)                                         # the case, not the kernel
    route = assert_philox_route(c, plan) if c["noise"] == "philox" else assert_route(c, plan)
    ref = gc.bf16_reference(c, oprob, net, draws)
    # ---- discrete results: exact
    K = ref["YN"].shape[0]
    assert plan.K_local == K and model.K_log == [ref["K_count"]], (model.K_log, ref["K_count"])
    t0 = draws["t0"].double().cpu().reshape(K)
    assert torch.equal(torch.round((plan.tN.double().cpu() - t0) / plan.cfg.dt).long(), ref["steps"])
    got = results(model, plan)
    assert got["grad"].shape == ref["grad"].shape and bool(torch.isfinite(got["grad"]).all())
    ek, em = gc.bf16_errors(c, got, ref, exact)
    w = WORST.setdefault(route, {})
    rows = [(n, ek[n], em[n]) for n in ("YN", "VN", "loss")] + list(zip(ek["blocks"][0], ek["blocks"][1], em["blocks"][1]))
    for name, a, b in rows:
        key = name if name in ("YN", "VN", "loss") else "block"
        if a / b > w.get(key, (-1.0,))[0]:
            w[key] = (a / b, name)
    try:
        gc.assert_bf16(c, got, ref, exact, gc.BF16_C, D_TOL, LOSS_TOL, BLOCK_TOL, tag=c["id"])
    finally:
        if c is ALL[-1]:
            for rt, q in sorted(WORST.items()):
                print("worst e_kernel / e_model per route: %-40s %s" % (rt, "  ".join("%s %.3f (%s)" % (k, v[0], v[1]) for k, v in sorted(q.items()))))


@pytest.mark.parametrize("cid", ["bf16-gen-10x24-allencahn-K40-bsde", "philox-bf16-gen-100x64-dwell-K40-bsde"])
def test_the_full_bf16_mode_runs_the_same_forward_bit_for_bit(cid, monkeypatch):
    """mlp_dtype='bf16' differs from 'bf16_fwd' in the path store's format (path16) and in the backward kernel only."""
    c = {c["id"]: c for c in gc.BF16_CASES}[cid]
    fwd = results(*run(c, monkeypatch, "bf16_fwd")[:2])
    model, plan = run(c, monkeypatch, "bf16")[:2]
    assert plan.matrix_mode == "bf16" and (plan.d_pad, plan.H_pad) == c["route"]["inst"]
    full = results(model, plan)
    same = {n: torch.equal(full[n], fwd[n]) for n in ("YN", "VN", "XN", "tN")}
    assert all(same.values()) and full["loss"] == fwd["loss"], (same, full["loss"], fwd["loss"])
    assert not torch.equal(full["grad"], fwd["grad"])                      # ... and the backward is another kernel


@pytest.mark.parametrize("mode", ["bf16_fwd", "bf16"])
def test_the_run_time_shaped_kernels_decline_the_bf16_modes(mode):
    """A DenseNet_tanh value net runs on the genl_* kernels, which have no bf16 products: the solver says why instead of running
    them in fp32 under a bf16 name."""
    c = gc.BY_ID["genl-d16-a65x33-linear-nw4"]
    case = dict(name=c["name"], family=c["family"], problem=c["problem"], solver=c["solver"], net=c["net"])
    prob, model = build_pkg(case, device=dev(), backend="native", noise="reference", mlp_dtype=mode)
    with pytest.raises(NotImplementedError, match=r"native plan unavailable: V is not a DenseNet\(17 -> 1\) with two equal hidden widths and relu\^2"):
        model._choose_plan()
