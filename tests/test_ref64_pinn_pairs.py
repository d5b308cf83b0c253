"""The float64 statement of the (K, K) PINN residual (ref64_pinn_pairs.py) against the composite plan and against itself, and
the regime of its test cases.  No GPU."""
import pytest
import torch

import ref64_pinn as r64
import ref64_pinn_pairs as rp
from conftest import load_golden
from pinn_cases import build, ref_case, seed_like_reference_train
from pinn_kernel_cases import REGIME_CAP, assert_rows

NAMES = sorted(rp.CASES)


def first_batch(case, model):
    """The points and times of the first train_PINN() iteration, drawn in its order."""
    seed_like_reference_train(case, model)
    model._sample_boundary()
    X = model.sample_domain()
    return X, torch.rand(model.K, 1) * model.problem.T


def test_statement_is_the_composite_plans_loss_on_the_goldens_first_iteration():
    rec = load_golden("pinn_expsphere_par_d3")
    case, exp = rec["case"], rec["expected"]
    _, model = build(case)
    X, t = first_batch(case, model)
    st = rp.statement(ref_case(model, X, t), alpha0=1.0)
    want = exp["loss_log_domain"][0]                               # fp32, alpha[0] = 1
    assert abs(float(st["loss"]) - want) <= 1e-5 * want
    _, model = build(case, L=1)
    seed_like_reference_train(case, model)
    model.train_PINN()
    assert model.plan_name == "torch"
    assert abs(float(st["loss"]) - model.loss_log_domain[0]) <= 1e-5 * want


def test_matrix_is_the_problems_own_broadcast():
    """problem.h(t (K, 1), x, y, z) of the package, op for op the reference's, against the statement's matrix."""
    rec = load_golden("pinn_expsphere_par_d3")
    prob, model = build(rec["case"])
    X, t = first_batch(rec["case"], model)
    case = ref_case(model, X, t)
    y = torch.randn(model.K, generator=torch.Generator().manual_seed(1)).double()
    R, _ = rp.matrix(case, y, torch.zeros_like(y), torch.float64)
    al, d = case["h_par"][0], case["d"]
    lin = -y * (2.0 * al * (2.0 * al * torch.sum(X.double() ** 2, 1) + d) + 1.0)
    h = prob.h(t.double(), X.double(), y, None)
    assert h.shape == (model.K, model.K)
    assert float((R + lin - h).abs().max()) <= 1e-12 * float(h.abs().max())


@pytest.mark.parametrize("name", NAMES)
def test_factorised_and_broadcast_gradients_agree_in_float64(name):
    f64 = rp.reference(name)["f64"]
    top = float(f64["grad_broadcast"].abs().max())
    assert top > 0.0
    assert float((f64["grad"] - f64["grad_broadcast"]).abs().max()) <= 1e-12 * top
    loss, _ = rp.broadcast(rp.reference(name)["case"])
    assert abs(float(loss) - float(f64["loss"])) <= 1e-14 * float(loss)


@pytest.mark.parametrize("name", NAMES)
def test_transposed_twin_misses_the_bound_by_100x(name):
    """The cases can tell (time i, sample j) from (time j, sample i).  K = 1 has a single pair: the twin is the statement."""
    ref = rp.reference(name)
    twin = rp.statement(ref["case"], transposed=True)
    rows = rp.evaluate(ref, twin)
    if ref["case"]["K"] == 1:
        assert all(torch.equal(twin[k], ref["f64"][k]) for k in ("A", "rho", "nu", "loss", "grad"))
        return
    assert rp.worst_miss(rows) >= 100.0, rp.worst_miss(rows)
    assert rp.worst_miss([r for r in rows if r[0] in ("rho", "nu")]) >= 100.0
    assert rp.worst_miss([r for r in rows if r[0].startswith("grad")]) >= 100.0
    assert abs(float(twin["loss"]) - float(ref["f64"]["loss"])) <= 1e-12 * float(twin["loss"])    # (same mean square)


@pytest.mark.parametrize("name", NAMES)
def test_regime_and_the_statements_pass_their_own_checks(name):
    ref = rp.reference(name)
    case = ref["case"]
    if case["act"] == "relu2":                                     # phi'' jumps at 0: no comparison across a sign flip
        assert r64.preact_margin(case) >= 1e-5
    rows32 = rp.evaluate(ref, ref["f32"])
    rows64 = rp.evaluate(ref, ref["f64"])
    assert_rows(rows32)
    assert_rows(rows64)
    for label, _, e32, bnd, _ in rows32:                           # the yardstick is sharp everywhere: the bound is never vacuous
        assert e32 <= REGIME_CAP and bnd <= 4.1e-5, (label, e32)
    top = float(ref["f64"]["grad_broadcast"].abs().max())
    for blk, v in r64.blocks(case, ref["f64"]["grad_broadcast"]).items():
        assert float(v.abs().max()) >= 1e-6 * top, blk


def test_tau_and_the_sine_are_read():
    """k521_sq_tau has tau = 0.5: a hard-coded 2 t misses by far more than the bound."""
    ref = rp.reference("k521_sq_tau")
    case = dict(ref["case"])
    case["h_par"] = case["h_par"][:3] + (1.0,)
    assert rp.worst_miss(rp.evaluate(ref, rp.statement(case))) >= 100.0
    ref = rp.reference("k257_sin")
    case = dict(ref["case"], h_kind=r64.H_EXP_SQ)
    assert rp.worst_miss(rp.evaluate(ref, rp.statement(case))) >= 100.0
