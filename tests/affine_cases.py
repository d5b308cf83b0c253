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


def cus():
    """The CU count make_aff_plan plans with: the device's, or 256 (the library's own fallback) without one."""
    return int(torch.cuda.get_device_properties(0).multi_processor_count) if torch.cuda.is_available() else 256


def k_big():
    """The first trajectory count with 256-thread workgroups (make_aff_plan: K > 64 CUs) and 17 valid lanes in the last one."""
    return 64 * cus() + 17


K_BIG = k_big()


def _sweep_case(kind, d, K, dt, T, control, loss="log-variance", detach=True, adaptive=True, random_x0=False, off_diag=None,
                u_l2=False):
    if kind == "DoubleWell_multidim":
        kwargs = dict(d=d, d_1=d // 2, d_2=d - d // 2, T=T, eta=0.05, kappa=1.0)
    elif kind == "LQGC":
        kwargs = dict(d=d, off_diag=0.05 if off_diag is None else off_diag, T=T, seed=42, delta_t=dt)
    else:
        kwargs = dict(d=d, off_diag=0.3 / d ** 0.5 if off_diag is None else off_diag, T=T, seed=42)
    solver = dict(loss_method=loss, time_approx="outer", adaptive_forward_process=adaptive, detach_forward=detach,
                  early_stopping_time=None, L=1, lr=0.1, seed=42, delta_t=dt, K=K, u_l2_error_flag=u_l2, random_X_0=random_x0)
    return dict(name="affsweep", family="solver", problem=dict(kind=kind, kwargs=kwargs), solver=solver, control=control)


LIN, AFF, CON = dict(kind="Linear"), dict(kind="Affine", init=dict(scale=0.1, seed0=50)), dict(kind="Constant")
SWEEP = {
    # ragged K, bucket 16
    "d5_K37": _sweep_case("LQGC", 5, 37, 0.05, 0.2, LIN),
    "d5_K37_attached": _sweep_case("LQGC", 5, 37, 0.05, 0.2, LIN, detach=False),
    # a single step: with X_0 = 0 a Linear control has an identically zero gradient there, hence random_X_0
    "d20_K16_N1_randx0": _sweep_case("LQGC", 20, 16, 0.05, 0.05, LIN, random_x0=True),
    "d20_K16_N1_randx0_attached": _sweep_case("LQGC", 20, 16, 0.05, 0.05, LIN, loss="moment", detach=False, random_x0=True),
    # exact bucket 64, dense A and B
    "d64_K50_N10": _sweep_case("LLGC", 64, 50, 0.02, 0.2, AFF),
    "d64_K50_N10_attached": _sweep_case("LLGC", 64, 50, 0.02, 0.2, AFF, detach=False),
    # bucket 64 with padding; running and terminal quadratic costs
    "d33": _sweep_case("LQGC", 33, 40, 0.05, 0.15, LIN),
    "d33_attached_cross_entropy": _sweep_case("LQGC", 33, 40, 0.05, 0.15, LIN, loss="cross_entropy", detach=False),
    # element-wise drift and its Jacobian, SHIFTED_QUAD
    "dw_d6_affine": _sweep_case("DoubleWell_multidim", 6, 48, 0.05, 0.2, AFF),
    "dw_d6_affine_attached": _sweep_case("DoubleWell_multidim", 6, 48, 0.05, 0.2, AFF, detach=False),
    "dw_d6_affine_nonadaptive": _sweep_case("DoubleWell_multidim", 6, 48, 0.05, 0.2, AFF, adaptive=False),
    # many workgroups and slices
    "K5000_d20": _sweep_case("LLGC", 20, 5000, 0.05, 0.15, LIN),
    "K5000_d20_relative_entropy": _sweep_case("LLGC", 20, 5000, 0.05, 0.15, LIN, loss="relative_entropy", detach=False),
    # chain rule with G = Q^-1 B^T != I
    "d7_gains": _sweep_case("LQGC", 7, 40, 0.05, 0.2, dict(kind="Linear", gains=3)),
    "d7_gains_attached": _sweep_case("LQGC", 7, 40, 0.05, 0.2, dict(kind="Linear", gains=3), detach=False),
    "d12_constant_variance": _sweep_case("LLGC", 12, 40, 0.05, 0.2, CON, loss="variance"),
    # 256-thread workgroups with a ragged last one, slices of several LDS stages
    "Kbig_d20_N3": _sweep_case("LLGC", 20, K_BIG, 0.05, 0.15, AFF),
    "Kbig_d20_N3_attached": _sweep_case("LLGC", 20, K_BIG, 0.05, 0.15, AFF, detach=False),
    # off_diag = 0, the constructors' default: diagonal drift, identity sigma
    "d12_llgc_diag": _sweep_case("LLGC", 12, 40, 0.05, 0.2, AFF, off_diag=0.0),
    "d12_llgc_diag_attached": _sweep_case("LLGC", 12, 40, 0.05, 0.2, AFF, detach=False, off_diag=0.0),
    "d12_lqgc_diag": _sweep_case("LQGC", 12, 40, 0.05, 0.2, LIN, off_diag=0.0),
    "d12_lqgc_diag_attached": _sweep_case("LQGC", 12, 40, 0.05, 0.2, LIN, detach=False, off_diag=0.0),
}
BIG_K = ("Kbig_d20_N3", "Kbig_d20_N3_attached")
DIAGONAL = ("d12_llgc_diag", "d12_llgc_diag_attached", "d12_lqgc_diag", "d12_lqgc_diag_attached")
# the u_L2 log next to a bucket-64 LINEAR reference: only the log entry and the plan are asserted at solver level, the values are
# compared at kernel level (tests/test_gpu_affine_kernels.py)
UL2_D33 = _sweep_case("LQGC", 33, 40, 0.05, 0.15, LIN, u_l2=True)
