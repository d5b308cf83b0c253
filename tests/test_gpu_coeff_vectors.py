"""The float64 block tests of the control-ansatz Solver kernels on coefficient vectors whose entries DIFFER from coordinate to
coordinate (tests/coeff_cases.py): drift (DIAG a_i, DOUBLE_WELL kappa_i), runcost (p_i), term (alpha_i, r_i, eta_i) and x0.

Each kernel family reads these vectors with index arithmetic of its own -- the permuted T layout 16 b + 4 r + q, block ownership
per wave, a Philox group -- and every stock problem hands it constant vectors, on which term[rowmap(i)], a neighbouring lane's entry
or entry 0 for all give bit-identical results.  tests/test_ref64_coeff.py shows on the CPU that each such mis-read moves D by at least
13 x D_TOL and, attached, a gradient block by at least 16 x BLOCK_TOL on these cases, and that a correct fp32 implementation stays
10 x inside both.  The criterion is that of tests/test_gpu_block_gradients.py and tests/test_gpu_dense_block_gradients.py, with
their bounds (imported): the first iteration through the plan against tests/ref64.py on the noise the kernels used, per trajectory
for D, the loss by the conditioning rule, each of the seven (tanh nets) or 9 / 12 per set (DenseNets) gradient blocks against its
own maximum.  Asserted on the plan besides the route: the four coefficient kinds of the set and sigma_scale = 0.8, the state basis,
the cooperative forward's tiles per workgroup (and that a running cost keeps a launch off that kernel).

Kernels that see a non-constant vector here for the first time: SIGMA_SCALED_IDENTITY in hjb / hjbs / hjbq / hjbw / hjbc / hjba / hjbd
(no stock Solver problem produces it); DRIFT_DIAG with distinct entries (and with a running cost and a quadratic terminal cost) in
all seven; distinct term / runcost / x0 entries in every forward and in hjb_adj, hjbq_adj, hjbw_adj and hjbd_adj; B^T alpha and
B^-1 x0 of a non-constant alpha, x0 under state_basis='sigma'.

Measured on an MI355X (127 cases, 6 s): D within 5.7e-7, loss within 8.0e-7, and the worst block error per route over its sets (bound
2e-4; the test prints one line per route and set):
  narrow-fp32-v1 1.6e-6 (W1t, lqgc_dense d = 100)   narrow-fp32-v2 5.2e-7 (W1t)   narrow-fp32-v3 4.2e-7 (b1)   narrow-f16x3 1.1e-6 (W2, dwell d = 100)
  narrow-philox 6.3e-7 (W3)    narrow-basis 4.6e-7 (W2)    narrow-relent 3.7e-7 (W1x)    narrow-variance 8.2e-7 (W2)
  wide-fp32 3.9e-6 (W1t, dwell d = 250: the fp32 stand-in of tests/test_ref64_coeff.py is 3.1e-6 off on the same block)
  wide-f16x3 3.8e-6 (W1t, the same case)    wide-coop2 = wide-coop4 1.5e-6 (b3, dwell d = 200)    wide-runcost-philox 1.2e-6 (W1t)
  DenseNets: 32x64 7.0e-7 (W1t, fp32 adjoint, lqgc_dense)    112x32 1.1e-6 (W2h1, fp32 adjoint, llgc_diag_sI)
i.e. every route is at the fp32-against-float64 floor on every set, 50 x inside the bound: no mis-indexed read was found.  With one
vector's entries 1 and 2 exchanged on the package side only (nine routes tried once, by hand) the same comparison is off by 17 x
.. 17 000 x D_TOL and 25 x .. 4 600 x BLOCK_TOL.
"""
import pytest
import torch

import block_cases as bc
import coeff_cases as cc
import dense_block_cases as dc
from test_gpu_block_gradients import BLOCK_TOL, D_TOL, SWITCHES, assert_route, dev, philox_noise
from test_gpu_dense_block_gradients import SWITCHES as DENSE_SWITCHES, assert_route as assert_dense_route
from util_cases import BLOCK_NAMES, assert_blocks, assert_dense_blocks, dense_block_names, flat_params, make_pkg_problem, psp

pytestmark = pytest.mark.gpu


def package_problem(c, case):
    prob = make_pkg_problem(case["problem"], dev())
    return cc.apply_to_package(c["cset"], prob, cc.case_vectors(c), dev())       # before the solver is built: it copies X_0


def same_problem(c, prob, model, oprob):
    """The same fp32 numbers on both sides."""
    assert torch.equal(model.X_0.cpu(), oprob.X_0) and torch.equal(prob.B.cpu(), oprob.B)
    for name, t in oprob.extra.items():
        if torch.is_tensor(t) and hasattr(prob, name):
            assert torch.equal(getattr(prob, name).cpu(), t), name


def run_tanh(c, monkeypatch):
    """tests/test_gpu_block_gradients.run_case with the coefficient set on the problem: (model, plan)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    case = cc.golden_style(c, c["K"])
    oprob, _, z = cc.scaled_oracle(c, c["K"])
    prob = package_problem(c, case)
    widths = (c["H"], c["H"])
    kw = dict(case["solver"], L=1, mlp_dtype=c["mode"])
    if c["basis"] is not None:
        kw["state_basis"] = c["basis"]
    model = psp.Solver(name=case["name"], problem=prob, verbose=False, device=dev(), backend="native", noise=c["noise"], widths=widths, **kw)
    model.z_n = psp.MySequential(prob.d + 1, prob.d, kw["lr"], seed=case["net"]["seed"], widths=widths)
    model.update_Phis()
    with torch.no_grad():
        for p in model.z_n.parameters():
            p.mul_(c["scale"])
    assert torch.equal(flat_params(model.z_n), flat_params(z))
    same_problem(c, prob, model, oprob)
    model.train()
    assert model.plan_name == "native" and model.N == c["N"], (model.plan_name, model.N)
    torch.cuda.synchronize()
    return model, model._native_plan


def run_dense(c, monkeypatch):
    """tests/test_gpu_dense_block_gradients.run_case with the coefficient set on the problem: (model, plan)."""
    for k in DENSE_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    case = cc.dense_golden_style(c)
    oprob, _, onets = cc.dense_oracle(c)
    prob = package_problem(c, case)
    model = psp.Solver(name=case["name"], problem=prob, verbose=False, device=dev(), backend="native", noise=c["noise"],
                       mlp_dtype=c["mode"], **case["solver"])
    nets = [psp.DenseNet(d_in=d_in, d_out=c["d"], lr=case["solver"]["lr"], arch=[c["H"], c["H"]], seed=seed).to(dev())
            for d_in, seed in dc.net_specs(c)]
    dc.prepare_nets(c, nets)
    model.z_n = nets if c["tmode"] == "outer" else nets[0]
    model.update_Phis()
    assert torch.equal(torch.cat([flat_params(n) for n in nets]), torch.cat([flat_params(n) for n in onets]))
    same_problem(c, prob, model, oprob)
    model.train()
    assert model.plan_name == "native" and model.N == c["N"], (model.plan_name, model.N)
    torch.cuda.synchronize()
    return model, model._native_plan


def assert_coeff_route(c, model, plan):
    if c["family"] == "dense":
        assert_dense_route(c, plan)
        cc.assert_kinds(c, plan.cfg.base)
        return
    assert_route(c, model, plan)
    cc.assert_kinds(c, plan.cfg)
    if c["basis"] is not None:
        assert plan.state_basis == c["basis"], (plan.state_basis, plan.state_basis_reason)
    else:
        assert plan.state_basis == "x", plan.state_basis_reason      # no set but llgc_dense is eligible for the sigma basis
    if c["coop"] is not None:
        assert int(plan.sizes.fwd_coop_tiles) == c["coop"], int(plan.sizes.fwd_coop_tiles)


WORST = {}                   # route -> (largest block error, block, case id): printed by the last case of the module
WORST_DL = [0.0, 0.0]        # largest D and loss errors


@pytest.mark.parametrize("c", cc.CASES, ids=[c["id"] for c in cc.CASES])
def test_first_iteration_matches_the_float64_reference_on_distinct_coefficients(c, monkeypatch):
    dense = c["family"] == "dense"
    model, plan = (run_dense if dense else run_tanh)(c, monkeypatch)
    assert_coeff_route(c, model, plan)
    draw = philox_noise if c["noise"] == "philox" else bc.host_noise
    ref = cc.reference(c, c["K"], lambda: draw(int(model.seed), c["K"], c["d"], c["N"]), stream="device")
    D, D_ref = plan.D.double().cpu(), ref["D"]
    assert D.shape == D_ref.shape and bool(torch.isfinite(D).all())
    eD = float((D - D_ref).abs().max()) / max(1.0, float(D_ref.abs().max()))
    tol_l = bc.first_loss_tol(bc.loss_values(c["loss"], D_ref), ref["loss"])
    el = abs(model.loss_log[0] - ref["loss"]) / abs(ref["loss"])
    route = "%s/%s" % (c["route"], c["cset"])
    print("%s [%s]: D %.2e (<= %.1e)  loss %.2e (<= %.1e)" % (c["id"], route, eD, D_TOL, el, tol_l))
    g = plan.grad.cpu()
    assert g.shape == ref["grad"].shape and bool(torch.isfinite(g).all())
    WORST_DL[0], WORST_DL[1] = max(WORST_DL[0], eD), max(WORST_DL[1], el)
    try:
        if dense:
            inner = c["tmode"] == "inner"
            errs = assert_dense_blocks(g, ref["grad"], c["d"], c["H"], len(ref["sets"]), inner, BLOCK_TOL, tag=c["id"])
            worst, blk = max((e, "%s of set %d" % (n, s)) for s, es in enumerate(errs) for e, n in zip(es, dense_block_names(inner)))
        else:
            errs = assert_blocks(g, ref["grad"], c["d"], c["H"], BLOCK_TOL, tag=c["id"])
            worst, blk = max(zip(errs, BLOCK_NAMES))
        if worst > WORST.get(route, (-1.0,))[0]:
            WORST[route] = (worst, blk, c["id"])
        assert eD <= D_TOL, eD
        assert el <= tol_l, (model.loss_log[0], ref["loss"])
    finally:
        if c is cc.CASES[-1]:
            for r, (e, b, cid) in sorted(WORST.items()):
                print("worst block per route: %-44s %.2e (%s) %s" % (r, e, b, cid))
            print("worst D %.2e  worst loss %.2e" % tuple(WORST_DL))
