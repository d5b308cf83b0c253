"""The float64 references of the attached value-function ansatz against each other and against the fp32 CPU oracle, on every
case of value_attached_cases.py (the shapes test_gpu_value_attached.py runs on the GPU):
  * the adjoint recursion the native sweep kernel runs (ref64_value.sweep_iteration) reproduces plain autograd
    (ref64_value.autograd_iteration) to 1e-12 of max|g|: loss, parameter gradient and dLoss/dX_0;
  * the fp32 oracle (oracle.hjb_train, detach_forward=False) is within 5e-6 of max|g| of the float64 gradient (measured on these
    shapes: 7e-8 .. 7e-7), so bounds stated against the oracle and against float64 mean the same;
  * every case is discriminating: the detached gradient differs from the attached one by at least 1e-2 of max|g|."""
import pytest
import torch

import value_attached_cases as vac


@pytest.mark.parametrize("name", vac.NAMES)
def test_sweep_recursion_reproduces_autograd(name):
    sw, ag = vac.ref64(name), vac.ref64_autograd(name)
    gmax = float(ag["grad"].abs().max())
    eg = float((sw["grad"] - ag["grad"]).abs().max()) / gmax
    ex = float((sw["dX0"] - ag["dX0"]).abs().max()) / float(ag["dX0"].abs().max())
    el = abs(sw["loss"] - ag["loss"]) / abs(ag["loss"])
    print("%s: recursion vs autograd: gradient %.1e, dL/dX0 %.1e, loss %.1e" % (name, eg, ex, el))
    assert gmax > 0 and float(ag["dX0"].abs().max()) > 0
    assert eg <= 1e-12 and ex <= 1e-12 and el <= 1e-12


@pytest.mark.parametrize("name", vac.NAMES)
def test_fp32_oracle_is_within_rounding_of_float64(name):
    loss_log, g32 = vac.oracle(name)
    ag = vac.ref64_autograd(name)
    err = float((g32.double() - ag["grad"]).abs().max()) / float(ag["grad"].abs().max())
    print("%s: fp32 oracle vs float64: gradient %.1e, loss %.1e" % (name, err, abs(loss_log[0] - ag["loss"]) / abs(ag["loss"])))
    assert err <= 5e-6
    assert abs(loss_log[0] - ag["loss"]) <= 5e-6 * abs(ag["loss"])


@pytest.mark.parametrize("name", vac.NAMES)
def test_cases_tell_the_attached_from_the_detached_gradient(name):
    _, ga = vac.oracle(name)
    _, gd = vac.oracle(name, detach=True)
    ratio = float((ga - gd)[:-1].abs().max()) / float(ga.abs().max())
    print("%s: |g_attached - g_detached| / max|g| = %.2e" % (name, ratio))
    assert ratio >= 1e-2


def test_state_adjoint_shapes():
    sw = vac.ref64("lqgc_d5")
    N, K, d = 10, 40, 5
    assert sw["U"].shape == (N, K, d) and sw["a"].shape == (N + 1, K) and sw["lam"].shape == (N + 1, K, d)
    assert torch.equal(sw["lam"][0], sw["dX0"]) and float(sw["a"][N].abs().max()) == 0.0
