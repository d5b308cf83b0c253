"""The float64 statement of the PINN residual (ref64_pinn.py) against the fp32 composite plan of train_PINN() on CPU: same
points, same parameters -- the problems' Python coefficients on one side, the catalogue description the kernels are configured
from (general_native_spec) on the other."""
import pytest
import torch

import ref64_pinn as r64
from conftest import load_golden
from pinn_cases import NATIVE_SCOPE, build, ref_case, seed_like_reference_train


@pytest.mark.parametrize("name", NATIVE_SCOPE)
def test_ref64_matches_the_composite_plan(name):
    torch.set_num_threads(1)
    case = load_golden(name)["case"]
    prob, model = build(case, L=1, boundary_loss=False, log_loss_parts=True, K_test_log=None)
    logvar = bool(model.PINN_log_variance)
    # the points train_PINN() is about to draw: same seeding, same draw order, then rewind
    seed_like_reference_train(case, model)
    if model.bounded:
        model._sample_boundary()
    X = model.sample_domain()
    t = None if model.elliptic else torch.rand(model.K, 1) * prob.T
    ref = ref_case(model, X, t)
    R64, loss64, g64 = r64.loss_and_grad(ref, alpha0=model.alpha[0], log_variance=logvar)
    seed_like_reference_train(case, model)
    model.train_PINN()
    assert model.plan_name == "torch"
    # fp32 against float64: the project's parity bound (1e-4 relative), far above fp32 rounding of these small nets
    assert model.loss_log_domain[0] == pytest.approx(float(loss64) / model.alpha[0], rel=1e-4)
    from path_space_pde_solver_amd.plan_general_deep import value_net_spec
    # the parameter tensors in registration order: their .grad is the gradient of the step just taken
    params = value_net_spec(model.V, model.d + (0 if model.elliptic else 1))["params"]
    g32 = torch.cat([(torch.zeros_like(p) if p.grad is None else p.grad).reshape(-1) for p in params]).double()
    assert g32.shape == g64.shape
    assert float((g32 - g64).abs().max()) <= 1e-4 * float(g64.abs().max())


def test_log_variance_gradient_is_the_centred_form():
    """d var(R) / d theta = sum_k 2 (R_k - mean R) / (K - 1) dR_k / d theta: what the native plan hands psp_pinn_backward."""
    case = r64.make_case(d=4, parabolic=False, arch=[9, 7], K=11, act="tanh2", seed=3, h_kind=r64.H_EXP_SIN, h_par=(0.3, 4.0, 0.0, 0.0))
    R, _, g = r64.loss_and_grad(case, alpha0=1.7, log_variance=True)
    params = [p.clone().requires_grad_(True) for p in case["params"]]
    Rg = r64.residual(case, params)
    rbar = 2.0 * 1.7 * (R - R.mean()) / (case["K"] - 1)
    gs = torch.autograd.grad(torch.sum(rbar * Rg), params)
    assert torch.allclose(torch.cat([v.reshape(-1) for v in gs]), g, rtol=1e-12, atol=1e-14)


def test_relu2_margins_of_the_kernel_shapes():
    from pinn_cases import GPU_SHAPES
    for name, kw in GPU_SHAPES.items():
        if kw["act"] == "relu2":
            assert r64.preact_margin(r64.make_case(**kw)) >= 1e-5, name
