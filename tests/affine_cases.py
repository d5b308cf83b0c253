"""Helpers of the linear / affine / constant control tests (plan_affine_native.py, csrc/aff_kernels.h)."""
import math

import torch

from util_cases import make_oracle, make_pkg_solver, orc, psp

GOLDEN = ["lqgc_d10_linear_outer_logvar", "lqgc_d10_linear_outer_moment_learn_y0", "lqgc_d10_linear_outer_cross_entropy",
          "lqgc_d10_linear_outer_relative_entropy_attached", "lqgc_d5_linear_outer_relative_entropy_randx0",
          "llgc_d20_affine_outer_attached_logvar", "llgc_d3_constant_outer_nonadaptive"]


def gain_matrices(d, seed=3):
    """Random well-conditioned B, Q (cond < 4) for a Linear control with G = Q^-1 B^T != I."""
    g = torch.Generator().manual_seed(seed)
    B = torch.eye(d) + 0.2 * torch.randn(d, d, generator=g) / math.sqrt(d)
    S = 0.2 * torch.randn(d, d, generator=g) / math.sqrt(d)
    Q = torch.eye(d) + 0.5 * (S + S.t())
    return B, Q


def build_modules(control, d, N, lr, seed, device=None):
    """The list a notebook assigns to model.z_n -- the recipe of tests/golden/make_golden_affine.py with this package's
    function_space; control['gains'] = seed adds B, Q != I to a Linear list (no golden has it)."""
    kind = control["kind"]
    mods = []
    for n in range(N):
        if kind == "Linear":
            if control.get("gains") is not None:
                B, Q = gain_matrices(d, control["gains"])
            else:
                B, Q = torch.eye(d), torch.eye(d)
            if device is not None:
                B, Q = B.to(device), Q.to(device)
            m = psp.Linear(d=d, B=B, Q=Q, lr=lr, seed=seed)
        elif kind == "Affine":
            m = psp.Affine(d=d, lr=lr, seed=seed)
        else:
            m = psp.Constant(d=d, lr=lr, seed=seed)
        init = control.get("init")
        if init is not None:
            g = torch.Generator().manual_seed(init["seed0"] + n)
            with torch.no_grad():
                for p in m.parameters():
                    p.copy_(init["scale"] * torch.randn(p.shape, generator=g))
        if device is not None:
            m.to(device)
        mods.append(m)
    return mods


def make_affine_solver(case, device, backend="auto", noise="reference", **over):
    model = make_pkg_solver(case, device, backend=backend, noise=noise, **over)
    model.z_n = build_modules(case["control"], model.d, model.N, model.lr, case["solver"]["seed"], device)
    model.update_Phis()
    return model


def make_affine_oracle(case, L=None):
    prob, cfg, models = make_oracle(case, L=L)
    z = build_modules(case["control"], prob.d, models[2], cfg.lr, case["solver"]["seed"])
    return prob, cfg, (z, models[1], models[2])


def assert_first_iteration(model, case, tag=""):
    """One native iteration against the oracle's autograd with the bounds of tests/test_gpu_dense_control.py: D within
    2e-5 max(1, |D|), the gradient within 2e-4 of its maximum overall and per parameter set (time step), the loss with that
    file's conditioning formula.  Prints every figure before it asserts."""
    oprob, ocfg, omodels = make_affine_oracle(case, L=1)
    model.train()
    plan = model._native_plan
    assert model.plan_name == "native" and isinstance(plan, psp.plan_affine_native.AffineNativePlan)
    ref = orc.hjb_train(oprob, ocfg, step_models=omodels, trace=True)
    tr = ref["traces"][0]
    relent = case["solver"]["loss_method"] == "relative_entropy"
    D, D_ref = plan.D.cpu(), (-tr["Zsum_g"] if relent else tr["D"])
    g, g_ref = plan.grad.cpu(), torch.cat([x.reshape(-1) for x in tr["grads"]])
    assert D.shape == D_ref.shape and g.shape == g_ref.shape
    errD = float((D - D_ref).abs().max()) / max(1.0, float(D_ref.abs().max()))
    gmax = float(g_ref.abs().max())
    errg = float((g - g_ref).abs().max()) / gmax
    N = model.N
    gs, gs_ref = g.view(N, -1), g_ref.view(N, -1)
    per = [float((gs[n] - gs_ref[n]).abs().max()) / max(float(gs_ref[n].abs().max()), 1e-30) for n in range(N)]
    cond = float((D_ref.double() ** 2).mean()) / max(abs(ref["loss_log"][0]), 1e-30)
    tol = min(1e-4, max(2e-5, 4 * 6e-8 * cond))
    print("%s: D err %.2e  grad err %.2e  worst step %.2e  loss %r vs %r (tol %.1e)"
          % (tag or case["name"], errD, errg, max(per), model.loss_log[0], ref["loss_log"][0], tol))
    assert gmax > 0.0
    assert errD <= 2e-5, errD
    assert errg <= 2e-4, errg
    assert max(per) <= 2e-4, per
    assert math.isclose(model.loss_log[0], ref["loss_log"][0], rel_tol=tol), (model.loss_log[0], ref["loss_log"][0])
    return plan, ref
