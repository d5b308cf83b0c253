"""The forward-Laplacian PINN kernels (csrc/pinn_kernels.h) on the GPU: through the C ABI against the float64 autograd statement
(ref64_pinn.py) with fp32 autograd as the yardstick, and at solver level against the reference's PINN goldens.

Kernel bounds: with e(v) = max|v - v64| / max|v64|, the kernels must stay within 8 e(fp32 torch autograd on CPU, same inputs)
+ 1e-6 -- the factor allows for another summation order over up to K (d + 2) rows, the constant for a yardstick that happens to
be exact.  Solver level: the project's parity contract, 1e-4 relative per iteration of the loss log."""
import functools

import pytest
import torch

import ref64_pinn as r64
from conftest import load_golden
from pinn_cases import COMPOSITE_ONLY, GPU_SHAPES, NATIVE_SCOPE, build, probe_values, seed_like_reference_train
from pinn_kernel_cases import Native

pytestmark = pytest.mark.gpu
ALPHA0 = 1.3


def dev():
    return torch.device("cuda:0")


def rel_err(v, v64):
    return float((v.double().cpu() - v64).abs().max()) / float(v64.abs().max())


@functools.lru_cache(maxsize=None)
def reference(name, log_variance=False):
    """(case, R64, g64, e_R of fp32 autograd, e_g of fp32 autograd): computed once per shape, never modified."""
    case = r64.make_case(**GPU_SHAPES[name])
    R64, _, g64 = r64.loss_and_grad(case, alpha0=ALPHA0, log_variance=log_variance)
    R32, _, g32 = r64.loss_and_grad(case, alpha0=ALPHA0, log_variance=log_variance, dtype=torch.float32)
    return case, R64, g64, rel_err(R32, R64), rel_err(g32, g64)


@pytest.mark.parametrize("name", sorted(GPU_SHAPES))
def test_residual_and_gradient_match_float64(name):
    case, R64, g64, eR32, eg32 = reference(name)
    if case["act"] == "relu2":                                   # phi'' jumps at 0: no comparison across a sign flip
        assert r64.preact_margin(case) >= 1e-5
    run = Native(case)
    R = run.residual()
    eR = rel_err(R, R64)
    g = run.backward((2.0 * ALPHA0 / case["K"]) * R)
    eg = rel_err(g, g64)
    print("%s: residual e_native %.2e e_torch32 %.2e | gradient e_native %.2e e_torch32 %.2e" % (name, eR, eR32, eg, eg32))
    assert eR <= 8.0 * eR32 + 1e-6
    assert eg <= 8.0 * eg32 + 1e-6


@pytest.mark.parametrize("name", ["d16_par_a24_40_8", "d37_a50_30x3_tanh2"])
def test_log_variance_gradient_matches_float64(name):
    case, R64, g64, _, eg32 = reference(name, True)
    run = Native(case)
    R = run.residual()
    g = run.backward((2.0 * ALPHA0 / (case["K"] - 1)) * (R - R.mean()))
    eg = rel_err(g, g64)
    print("%s (variance): gradient e_native %.2e e_torch32 %.2e" % (name, eg, eg32))
    assert eg <= 8.0 * eg32 + 1e-6


def test_backward_is_deterministic_and_leaves_its_inputs():
    case = reference("d16_par_a24_40_8")[0]
    run = Native(case)
    R = run.residual().clone()
    rbar = (2.0 / case["K"]) * R
    g1 = run.backward(rbar).clone()
    g2 = run.backward(rbar)
    assert torch.equal(g1, g2) and torch.equal(run.residual(), R)


@pytest.mark.parametrize("name", NATIVE_SCOPE)
def test_solver_matches_the_reference_golden(name):
    rec = load_golden(name)
    case, exp = rec["case"], rec["expected"]
    prob, model = build(case, device=dev())
    seed_like_reference_train(case, model)
    model.train_PINN()
    assert model.plan_name == "native", model.plan_reason
    errs = [abs(a - b) / abs(b) for a, b in zip(model.loss_log, exp["loss_log"])]
    print("%s: loss rel err per iteration %s" % (name, ["%.1e" % e for e in errs]))
    assert len(model.loss_log) == len(exp["loss_log"]) and max(errs) <= 1e-4, (model.loss_log, exp["loss_log"])
    assert model.K == exp["K"] and model.K_log == []
    for key in ("V_L2_log", "loss_log_domain", "loss_log_boundary", "V_test_L2"):
        got = getattr(model, key)
        assert len(got) == len(exp[key])
        for a, b in zip(got, exp[key]):
            assert abs(a - b) <= 1e-4 * abs(b) + 1e-12, (key, got, exp[key])
    v, want = probe_values(case, exp, prob, model), torch.tensor(exp["probe_V"])
    assert float((v - want).abs().max()) <= 1e-4 * max(1e-2, float(want.abs().max()))


@pytest.mark.parametrize("name", sorted(COMPOSITE_ONLY))
def test_composite_only_goldens_plan_torch_on_the_gpu(name):
    rec = load_golden(name)
    case, exp = rec["case"], rec["expected"]
    prob, model = build(case, device=dev())
    seed_like_reference_train(case, model)
    with pytest.warns(UserWarning, match="composite torch plan"):
        model.train_PINN()
    assert model.plan_name == "torch" and COMPOSITE_ONLY[name] in model.plan_reason
    errs = [abs(a - b) / abs(b) for a, b in zip(model.loss_log, exp["loss_log"])]
    assert max(errs) <= 1e-4, (model.loss_log, exp["loss_log"])
    _, model = build(case, device=dev(), backend="native")
    with pytest.raises(NotImplementedError, match="native plan unavailable"):
        model.train_PINN()


def test_device_test_log_runs_behind_the_native_plan():
    """test_log='device': the K_test_log diagnostic on the plan's stream; its points come from the device generator, so only the
    first loss (drawn before any test point) is the golden's."""
    import math
    rec = load_golden("pinn_heat_d6")
    prob, model = build(rec["case"], device=dev(), test_log="device")
    seed_like_reference_train(rec["case"], model)
    model.train_PINN()
    assert model.plan_name == "native"
    assert abs(model.loss_log[0] - rec["expected"]["loss_log"][0]) <= 1e-4 * rec["expected"]["loss_log"][0]
    for log in (model.V_test_L2, model.V_test_abs, model.V_test_rel_abs):
        assert len(log) == 3 and all(math.isfinite(v) and v > 0.0 for v in log)
    want = rec["expected"]["V_test_L2"]                          # other points, same error: a Monte-Carlo estimate on 16 points
    assert 0.2 * want[0] <= model.V_test_L2[0] <= 5.0 * want[0]


def test_train_and_train_pinn_on_one_model_each_train_the_live_parameters():
    """Both plans make the net's tensors views of their own flat buffer: the one built last owns them, the other is rebuilt
    instead of stepping a stale copy."""
    from test_general_composite_golden import build as build_general
    _, model = build_general(load_golden("allencahn_d10_arch3_diffusion")["case"], device=dev(), backend="native", L=1)
    model.problem.B = model.problem.B_pt
    first = next(iter(model.V.parameters()))
    for step in (model.train, model.train_PINN, model.train, model.train_PINN):
        before = first.detach().clone()
        step()
        assert model.plan_name == "native"
        plan = model._pinn_plan if step == model.train_PINN else model._gen_plan
        assert first.data_ptr() == plan.flat.data_ptr()
        assert not torch.equal(first.detach(), before)


def test_train_still_refuses_pinn_on_the_gpu():
    _, model = build(load_golden("pinn_heat_d6")["case"], device=dev())
    with pytest.raises(NotImplementedError, match="train_PINN"):
        model.train()


def test_diffusion_loss_is_unchanged():
    """The diffusion-loss kernels and their plan are untouched: this golden's loss log, bit for bit as before the PINN plan."""
    from test_general_composite_golden import build as build_general
    rec = load_golden("allencahn_d10_arch3_diffusion")
    want = load_golden("pinn_unchanged_allencahn_d10_arch3_gpu")["loss_log"]
    _, model = build_general(rec["case"], device=dev(), backend="native")
    model.train()
    assert model.plan_name == "native"
    assert model.loss_log == want, (model.loss_log, want)
