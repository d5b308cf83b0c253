"""Solver(approx_method='value_function', value_state_path='native') with the state path attached (adaptive_forward_process=True,
detach_forward=False): forward kernel, the adjoint sweep of csrc/genl_adj_kernels.h, the unchanged backward kernel -- against the
CPU oracle (oracle/pathspace_oracle.py hjb_train, detach_forward=False) and the float64 restatement of tests/ref64_value.py
(which test_ref64_value.py pins on plain autograd to 1e-12 and on the oracle to 5e-6).

Bounds of this kernel family (test_gpu_value_function_lq.py): first-iteration loss <= 5e-5 relative, first-iteration gradient
<= 5e-4 max|g| (output bias excluded), whole loss log <= 1e-4 relative.  dLoss/dX_0 (lam0_out) and the rewritten directions U_n
are linear in the state adjoint and the weights mu that the gradient is made of, with the same fp32 products: the same 5e-4, of
max|dLoss/dX_0| and of max|U| over all steps.  Every gradient case is discriminating: the oracle's DETACHED gradient differs from
the attached one by at least 1e-2 max|g| (20 x the bound; test_ref64_value.py checks the same on the CPU)."""
import functools
import math
import types

import pytest
import torch

import value_attached_cases as vac
from conftest import load_golden
from test_gpu_dense_ul2 import _images_X
from util_cases import make_pkg_solver, psp

pytestmark = pytest.mark.gpu
nat = psp.native


def dev():
    return torch.device("cuda:0")


def _run(name, **over):
    model = vac.make_pkg(name, dev(), **over)
    model.train()
    assert model.plan_name == "native", (model.plan_name, getattr(model, "plan_reason", None))
    plan = model._native_plan
    assert isinstance(plan, psp.plan_value_native.ValueNativePlan) and plan.deep is not None
    assert plan.attached and plan.adj is not None
    return model, plan


def _directions(plan, N, K, d):
    """U_n (N, K, d) from the path store: block (n, tile) = the X image, then the U image, each DB0 * 256 floats in the layout
    test_gpu_dense_ul2._images_X decodes (image float ks * 64 + 16 q + j = feature 4 ks + q of sample j)."""
    nt = (K + 15) // 16
    db0 = plan.path.numel() // ((N + 1) * nt * 512)
    store = plan.path.view(N + 1, nt, 2, db0 * 256)
    shim = types.SimpleNamespace(images=store[:, :, 1].contiguous(), d_pad=16 * db0)
    return _images_X(shim, N + 1, K, d)[:N]


@functools.lru_cache(maxsize=None)
def first_iteration(name):
    """One native iteration per case, shared by the tests: loss, gradient, dLoss/dX_0, the rewritten directions."""
    model, plan = _run(name, L=1)
    torch.cuda.synchronize()
    return dict(loss=model.loss_log[0], grad=plan.grad.cpu(), lam0=plan.lam0.cpu(),
                U=_directions(plan, model.N, model.K, model.d).cpu(), coeffs=plan.coeffs is not None,
                waves=int(plan.sizes.waves_per_tile), log=plan.ul2_cfg is not None, ul2=list(model.u_L2_loss))


@pytest.mark.parametrize("name", vac.NAMES)
def test_first_iteration_loss_and_gradient_match_the_oracle(name):
    got = first_iteration(name)
    loss_ref, g_ref = vac.oracle(name)
    _, g_det = vac.oracle(name, detach=True)
    g = got["grad"]
    assert g.shape == g_ref.shape
    err = float((g - g_ref)[:-1].abs().max()) / float(g_ref.abs().max())
    apart = float((g_det - g_ref)[:-1].abs().max()) / float(g_ref.abs().max())
    print("%s: gradient rel err %.1e (detached gradient is %.1e away), loss %.6e vs %.6e (rel %.1e)"
          % (name, err, apart, got["loss"], loss_ref[0], abs(got["loss"] - loss_ref[0]) / abs(loss_ref[0])))
    assert apart >= 1e-2, apart                                      # a plan that ran the detached path could not pass
    assert math.isclose(got["loss"], loss_ref[0], rel_tol=5e-5), (got["loss"], loss_ref)
    assert err <= 5e-4, err


@pytest.mark.parametrize("name", vac.NAMES)
def test_state_adjoint_at_the_initial_point_matches_float64(name):
    got, ref = first_iteration(name), vac.ref64(name)
    want = ref["dX0"]
    err = float((got["lam0"].double() - want).abs().max()) / float(want.abs().max())
    print("%s: dLoss/dX_0 rel err %.1e (max %.2e)" % (name, err, float(want.abs().max())))
    assert float(want.abs().max()) > 0 and err <= 5e-4, err


@pytest.mark.parametrize("name", vac.SHARED)
def test_rewritten_directions_match_float64_per_step(name):
    got, ref = first_iteration(name), vac.ref64(name)
    U, want = got["U"].double(), ref["U"]
    assert U.shape == want.shape
    scale = float(want.abs().max())
    errs = [float((U[n] - want[n]).abs().max()) / scale for n in range(U.shape[0])]
    print("%s: U_n err per step / max|U| %s" % (name, ["%.1e" % e for e in errs]))
    assert max(errs) <= 5e-4, errs


@pytest.mark.parametrize("name", vac.NAMES)
def test_loss_log_matches_the_oracle(name):
    model, plan = _run(name)
    loss_ref, _ = vac.oracle(name)
    errs = [abs(a - b) / abs(b) for a, b in zip(model.loss_log, loss_ref)]
    print("%s: loss rel err per iteration vs the oracle %s" % (name, ["%.1e" % e for e in errs]))
    assert len(model.loss_log) == len(loss_ref) == 3
    for a, b in zip(model.loss_log, loss_ref):
        assert math.isclose(a, b, rel_tol=1e-4), (model.loss_log, loss_ref)


def test_cases_take_the_paths_they_are_meant_to():
    wide, dwell, log = first_iteration("lqgc_d20_wide"), first_iteration("dwell_d10"), first_iteration("lqgc_d5_ul2")
    assert wide["waves"] == 8                                        # nine hidden blocks: the eight-wave instances
    assert first_iteration("lqgc_d5")["waves"] == 1
    assert not dwell["coeffs"] and wide["coeffs"]                    # sigma = s I, element-wise drift: no coefficients struct
    # the log instances of the forward together with the sweep: the first iteration's forward does not depend on the state path
    assert log["log"] and len(log["ul2"]) == 1 and math.isfinite(log["ul2"][0]) and log["ul2"][0] > 0
    model = vac.make_pkg("lqgc_d5_ul2", dev(), L=1, detach_forward=True)
    model.train()
    assert model.plan_name == "native" and not model._native_plan.attached
    assert math.isclose(log["ul2"][0], model.u_L2_loss[0], rel_tol=1e-6), (log["ul2"], model.u_L2_loss)
    assert math.isclose(log["loss"], first_iteration("lqgc_d5")["loss"], rel_tol=1e-6)


def test_four_wave_instance_matches_the_oracle(monkeypatch):
    """The forward takes four waves per tile once the batch fills the chip twice over; PSP_GENL_NW=4 selects that instance of the
    forward and of the sweep at the test's batch size."""
    monkeypatch.setenv("PSP_GENL_NW", "4")
    model, plan = _run("lqgc_d20_wide", L=1)
    assert int(plan.sizes.waves_per_tile) == 4
    loss_ref, g_ref = vac.oracle("lqgc_d20_wide")
    err = float((plan.grad.cpu() - g_ref)[:-1].abs().max()) / float(g_ref.abs().max())
    ex = float((plan.lam0.cpu().double() - vac.ref64("lqgc_d20_wide")["dX0"]).abs().max()) / float(vac.ref64("lqgc_d20_wide")["dX0"].abs().max())
    print("lqgc_d20_wide, four waves: gradient rel err %.1e, dLoss/dX_0 rel err %.1e" % (err, ex))
    assert math.isclose(model.loss_log[0], loss_ref[0], rel_tol=5e-5)
    assert err <= 5e-4 and ex <= 5e-4


def test_reference_golden_runs_native_with_the_keyword():
    rec = load_golden("lqgc_d3_value_function")
    model = make_pkg_solver(rec["case"], dev(), backend="native", value_state_path="native")
    model.train()
    assert model.plan_name == "native" and model._native_plan.attached
    exp = rec["expected"]["loss_log"]
    errs = [abs(a - b) / abs(b) for a, b in zip(model.loss_log, exp)]
    print("lqgc_d3_value_function: loss rel err per iteration vs the reference %s" % ["%.1e" % e for e in errs])
    assert len(model.loss_log) == len(exp)
    for a, b in zip(model.loss_log, exp):
        assert math.isclose(a, b, rel_tol=2e-4), (model.loss_log, exp)


def test_philox_noise_is_finite_and_deterministic():
    runs = []
    for _ in range(2):
        model, plan = _run("lqgc_d5", noise="philox", K=4096, L=2)
        runs.append((model.loss_log, plan.grad.clone(), plan.lam0.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert len(runs[0][0]) == 2 and all(math.isfinite(v) for v in runs[0][0]) and bool(torch.isfinite(runs[0][1]).all())
    assert float(runs[0][1].abs().max()) > 0 and float(runs[0][2].abs().max()) > 0
