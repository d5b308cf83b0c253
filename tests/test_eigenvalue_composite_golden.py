"""EigenvalueSolver's composite plan against the reference's three eigenvalue notebooks, run as written
(tests/golden/eig_*.json, tests/golden/make_golden_eigenvalue.py); the problem classes against the coefficient values recorded
there; DenseNet / DenseNet_tanh with default keywords against their committed fingerprints."""
import math

import pytest
import torch

from conftest import load_golden
from eigen_cases import GOLDENS, LOSS_LOGS, build, fingerprint
from util_cases import psp


def close(got, want, exact, rel=1e-5):
    """The bound of tests/test_general_composite_golden.py: the same numbers on the torch that wrote the golden, fp32 rounding on another."""
    return (got == want) if exact else math.isclose(got, want, rel_tol=rel, abs_tol=1e-12)


@pytest.mark.parametrize("name", GOLDENS)
def test_composite_matches_notebook(name):
    torch.set_num_threads(1)
    rec, prob, model = build(name)
    exp = rec["expected"]
    exact = rec["torch"] == torch.__version__
    for a, b in zip(fingerprint(model.V), exp["init_params"]):
        assert a["shape"] == b["shape"] and a["sum"] == b["sum"] and a["abs_sum"] == b["abs_sum"]
    assert model.lambda_.Y_0.item() == exp["lambda_init"]
    model.train()
    assert model.plan_name == "torch"
    assert model.K_log == exp["K_log"]
    for log in LOSS_LOGS + ("V_L2_log", "lambda_log"):
        got, want = getattr(model, log), exp[log]
        assert len(got) == len(want) == rec["case"]["L"]
        for g, w in zip(got, want):
            assert close(g, w, exact), (log, got, want)
    for a, b in zip(fingerprint(model.V), exp["final_params"]):
        assert close(a["sum"], b["sum"], exact, 1e-5) and close(a["abs_sum"], b["abs_sum"], exact, 1e-5)
    assert close(model.lambda_.Y_0.item(), exp["lambda_final"], exact)
    assert len(model.times) == rec["case"]["L"]


@pytest.mark.parametrize("name", ["eig_fp_d5", "eig_fp_d10", "eig_nls5_d5", "eig_nls10_d10", "eig_nls10_d2_exits"])
def test_problem_coefficients_match_notebook(name):
    rec, prob, model = build(name)
    exp, d = rec["expected"], rec["case"]["d"]
    co = exp["coefficients"]
    x, y = torch.tensor(co["x"]).reshape(-1, d), torch.tensor(co["y"])
    assert torch.equal(prob.b(x).reshape(-1), torch.tensor(co["b"]))
    assert torch.allclose(prob.h(x, y, None), torch.tensor(co["h"]), rtol=1e-6, atol=0)
    assert torch.allclose(prob.v_true(x), torch.tensor(co["v_true"]), rtol=1e-6, atol=0)
    if exp["c"] is not None:
        assert prob.c == exp["c"]
    assert prob.boundary == "square" and prob.one_boundary is False
    assert (prob.X_l, prob.X_r) == (0.0, 2 * math.pi) and prob.lambda_ == (0.0 if name.startswith("eig_fp") else -3.0)
    assert torch.equal(prob.X_0, math.pi * torch.ones(d)) or torch.allclose(prob.X_0, torch.tensor(math.pi) * torch.ones(d))
    assert torch.equal(prob.B, torch.sqrt(torch.tensor(2.0)) * torch.eye(d))
    assert torch.equal(prob.sigma(x), prob.B) and torch.equal(prob.g(x), torch.zeros(x.shape[0]))


def test_schroedinger_constant_is_the_notebooks():
    """The constants the two notebooks hard-code for their own d."""
    assert psp.SchroedingerEigenvalue(d=5).c == 1.1040855314961615
    assert psp.SchroedingerEigenvalue(d=10).c == 1.0511402766738196


@pytest.mark.parametrize("name", ["allencahn_d10_arch3_diffusion", "allencahn_d10_densenet_tanh_diffusion"])
def test_default_nets_keep_their_fingerprints(name):
    """DenseNet / DenseNet_tanh with default keywords draw what they drew: the init fingerprints of committed goldens."""
    from test_general_composite_golden import build as build_general
    rec = load_golden(name)
    prob, model = build_general(rec["case"])
    assert getattr(model.V, "output_relu", None) is False
    for (pname, p), want in zip(model.V.named_parameters(), rec["expected"]["init_params"]):
        q = p.detach().double()
        assert list(p.shape) == want["shape"] and float(q.sum()) == want["sum"] and float(q.abs().sum()) == want["abs_sum"]
    with torch.no_grad():
        plain = psp.DenseNet(4, 1, 0.001, arch=[6, 5], seed=3)
        relu = psp.DenseNet(4, 1, 0.001, arch=[6, 5], seed=3, output_relu=True)
        xx = 3 * torch.randn(64, 4)
        assert torch.equal(relu(xx), torch.relu(plain(xx))) and bool((plain(xx) < 0).any())
        pt, rt = psp.DenseNet_tanh(4, 1, 0.001, arch=[6, 5], seed=3), psp.DenseNet_tanh(4, 1, 0.001, arch=[6, 5], seed=3, output_relu=True)
        assert torch.equal(rt(xx), torch.relu(pt(xx))) and bool((pt(xx) < 0).any())
