"""The PINN goldens (tests/golden/pinn_*.json, made by make_golden_pinn.py) and how a test turns one into a package solver."""
import numpy as np
import torch

from util_cases import make_pkg_value_net, psp

# in the native scope of plan_pinn_native.py (they run on the composite plan on a CPU)
NATIVE_SCOPE = ["pinn_allencahn_d5", "pinn_heat_d6", "pinn_dwgen_d4", "pinn_expball_sin_d5_elliptic",
                "pinn_expball_sin_d5_elliptic_logvar", "pinn_committor_d3_tanh2", "pinn_box_d4_elliptic"]
# composite on every device, with the reason plan_pinn_native.pinn_eligibility gives (a substring of it)
COMPOSITE_ONLY = {"pinn_expsphere_par_d3": "reads t", "pinn_expsphere_par_d3_neumann": "reads t",
                  "pinn_expball_hess_d4_full": "full_hessian"}
ALL = NATIVE_SCOPE + list(COMPOSITE_ONLY)


def build(case, device="cpu", backend="auto", **over):
    prob = getattr(psp, case["problem"]["kind"])(device=device, **case["problem"]["kwargs"])
    for k, v in case["problem"].get("attrs", {}).items():
        setattr(prob, k, v)
    for dst, src in case["problem"].get("attr_copies", {}).items():
        setattr(prob, dst, getattr(prob, src))
    elliptic = case["family"] == "elliptic"
    cls = psp.EllipticSolver if elliptic else psp.GeneralSolver
    kw = dict(case["solver"])
    kw.update(over)
    model = cls(problem=prob, name=case["name"], verbose=False, device=device, backend=backend, **kw)
    if "net" in case:
        model.V = make_pkg_value_net(case["net"], prob.d + (0 if elliptic else 1), case["solver"]["lr"], device)
    return prob, model


def seed_like_reference_train(case, model):
    """What the reference's train() does before it calls train_PINN(): manual_seed, and np.random.seed for the elliptic class
    (the parabolic class leaves numpy to the caller)."""
    if "numpy_seed" in case:
        np.random.seed(case["numpy_seed"])
    torch.manual_seed(model.seed)
    if case["family"] == "elliptic":
        np.random.seed(model.seed)


def probe_values(case, exp, prob, model):
    xp = torch.tensor(exp["probe_x"]).reshape(-1, prob.d)
    if case["family"] != "elliptic":
        xp = torch.cat([xp, torch.full((xp.shape[0], 1), exp["probe_t"])], 1)
    with torch.no_grad():
        return model.V(xp.to(model.device)).squeeze().cpu()


def ref_case(model, X, t):
    """The float64 statement's inputs (ref64_pinn.make_case's dict) for a package solver in the native scope: its net through
    value_net_spec, its coefficients through general_native_spec() -- the description the kernels are configured from."""
    from path_space_pde_solver_amd.plan_general_deep import value_net_spec
    elliptic = model.elliptic
    net = value_net_spec(model.V, model.d + (0 if elliptic else 1))
    assert not isinstance(net, str), net
    spec = model.problem.general_native_spec()
    vec = spec["drift"][1]
    return dict(d=model.d, parabolic=not elliptic, arch=net["dims"][1:-1], K=X.shape[0], act=net["act"], linear=net["linear"],
                params=[p.detach().cpu().double().clone() for p in net["params"]], x=X.detach().cpu().double(),
                t=None if t is None else t.detach().cpu().double().reshape(-1), s=float(spec["sigma_scale"]),
                drift_kind=spec["drift"][0], drift=None if vec is None else vec.detach().cpu().double(),
                h_kind=spec["h"], h_par=tuple(float(v) for v in spec.get("h_par", (0.0, 0.0, 0.0, 0.0))))


# Shapes of the kernel tests (tests/test_gpu_pinn.py): the smallest at which padding, block boundaries and depth can go wrong.
# A tile carries 14 input columns: 16 inputs = 2 blocks, 17 inputs = 2 blocks with the time column in the second, 37 = 3, 101 = 8.
# relu^2 seeds are chosen such that no float64 pre-activation lies within 1e-5 max|z| of the kink (the tests assert it).
import ref64_pinn as r64  # noqa: E402

GPU_SHAPES = {
    "d3_a20": dict(d=3, parabolic=False, arch=[20], K=5, act="relu2", seed=0, h_kind=r64.H_ALLEN_CAHN),
    "d15_par_a16x2": dict(d=15, parabolic=True, arch=[16, 16], K=33, act="relu2", seed=0, h_kind=r64.H_QUAD,
                          drift_kind=r64.DRIFT_DWELL, s=1.0),
    "d16_par_a24_40_8": dict(d=16, parabolic=True, arch=[24, 40, 8], K=17, act="relu2", seed=0, h_kind=r64.H_ALLEN_CAHN,
                             drift_kind=r64.DRIFT_DIAG),
    "d37_a50_30x3_relu2": dict(d=37, parabolic=False, arch=[50, 30, 30, 30], K=40, act="relu2", seed=16, h_kind=r64.H_EXP_SIN,
                               h_par=(0.05, 37.0, 0.0, 0.0)),
    "d37_a50_30x3_tanh": dict(d=37, parabolic=False, arch=[50, 30, 30, 30], K=40, act="tanh", seed=0, linear=True,
                              h_kind=r64.H_EXP_SQ, h_par=(0.05, 37.0, 0.0, 0.0)),
    "d37_a50_30x3_tanh2": dict(d=37, parabolic=False, arch=[50, 30, 30, 30], K=40, act="tanh2", seed=0, h_kind=r64.H_ZERO, s=1.0),
    "d100_par_notebook": dict(d=100, parabolic=True, arch=[110, 110, 50], K=32, act="relu2", seed=15, h_kind=r64.H_ALLEN_CAHN),
}
