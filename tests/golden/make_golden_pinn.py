"""Goldens of the PINN baseline: the reference's own GeneralSolver / EllipticSolver ``train()`` with ``loss_method='PINN'``
(which seeds and then calls its ``train_PINN()``), on CPU through make_golden's proxy.  A separate script so that make_golden.py,
index.json and the fixtures it writes stay as they are.  Data only: the case, the logs, ``K``, probe values, fingerprints.

    python tests/golden/make_golden_pinn.py [case names]
"""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402

S = dict(seed=42, delta_t=0.01, N=10, lr=0.001, L=3, K=24, K_boundary=8, loss_method="PINN")
EXPSPHERE = dict(kind="ExponentialOnSphereNonlinearParabolic", kwargs=dict(d=3, T=0.5, alpha=0.7))

CASES = [
    # the notebook's configuration in small: uniform_square, problem.B = problem.B_pt, a three-layer net
    dict(name="pinn_allencahn_d5", family="general",
         problem=dict(kind="AllenCahn", kwargs=dict(d=5, T=0.3, seed=42, modus="pt"), attr_copies=dict(B="B_pt")),
         solver=dict(S, alpha=[1.0, 1.0, 1.0], uniform_square=True), net=dict(arch=[20, 20, 12], seed=42)),
    # one hidden layer, K = 2 * 16 + 1, the test log after every step
    dict(name="pinn_heat_d6", family="general",
         problem=dict(kind="HeatEquation", kwargs=dict(d=6, T=0.5, seed=42)),
         solver=dict(S, K=33, alpha=[1.0, 1.0, 1.0], K_test_log=16), net=dict(arch=[16], seed=42)),
    # a z-dependent h and a drift
    dict(name="pinn_dwgen_d4", family="general",
         problem=dict(kind="DoubleWell_multidim_for_general_solver", kwargs=dict(d=4, d_1=2, d_2=2, T=0.3, eta=1, kappa=1, modus="HJB")),
         solver=dict(S, alpha=[1.0, 1.0, 1.0])),
    # a time-dependent h: it receives t_n as (K, 1) and the residual broadcasts to (K, K)
    dict(name="pinn_expsphere_par_d3", family="general", problem=EXPSPHERE,
         solver=dict(S, alpha=[1.0, 0.5, 2.0], log_loss_parts=True)),
    dict(name="pinn_expsphere_par_d3_neumann", family="general",
         problem=dict(EXPSPHERE, attrs=dict(boundary_type="Neumann")), solver=dict(S, alpha=[1.0, 0.5, 2.0])),
    dict(name="pinn_expball_sin_d5_elliptic", family="elliptic",
         problem=dict(kind="ExponentialOnBallNonlinearSin", kwargs=dict(d=5, alpha=0.5)),
         solver=dict(S, alpha=[1.0, 2.0], log_loss_parts=True)),
    dict(name="pinn_expball_sin_d5_elliptic_logvar", family="elliptic",
         problem=dict(kind="ExponentialOnBallNonlinearSin", kwargs=dict(d=5, alpha=0.5)),
         solver=dict(S, alpha=[1.0, 2.0], PINN_log_variance=True)),
    dict(name="pinn_expball_hess_d4_full", family="elliptic",
         problem=dict(kind="ExponentialOnBallNonlinearSinHessian", kwargs=dict(d=4, alpha=0.5)),
         solver=dict(S, alpha=[1.0, 1.0], full_hessian=True)),
    # 'two_spheres': the rejection step changes K; the notebook's tanh^2 net [d + 10, d, d, d].  Without the boundary term: the
    # committor's data [|x| > a] is evaluated exactly ON the sampled inner sphere, where the last bit of a host-side norm decides
    # between 0 and 1 -- two CPUs disagreed on one of these twelve points, which moves the loss by (1 - 2 V) / K_boundary.  A
    # fixture must not hang on that bit; the data terms are pinned by the sphere and box cases.
    dict(name="pinn_committor_d3_tanh2", family="elliptic",
         problem=dict(kind="Committor", kwargs=dict(d=3)),
         solver=dict(S, alpha=[10.0, 1.0], boundary_loss=False), net=dict(kind="user_tanh2", arch=[13, 3, 3, 3], seed=42)),
    # the numpy shuffle of the square's boundary batch
    dict(name="pinn_box_d4_elliptic", family="elliptic", numpy_seed=3,
         problem=dict(kind="QuadraticOnBox", kwargs=dict(d=4, X_l=-1.0, X_r=1.0, parabolic=False)),
         solver=dict(S, alpha=[1.0, 1.0])),
]


def run_case(case):
    problem = mg.make_problem(case["problem"])
    for dst, src in case["problem"].get("attr_copies", {}).items():     # what the notebooks assign: problem.B = problem.B_pt
        setattr(problem, dst, getattr(problem, src))
    elliptic = case["family"] == "elliptic"
    cls = mg.ref_sv.EllipticSolver if elliptic else mg.ref_sv.GeneralSolver
    skw = dict(case["solver"])
    model = cls(problem=problem, name=case["name"], verbose=False, **skw)
    if "net" in case:
        model.V = mg.make_value_net(case["net"], problem.d + (0 if elliptic else 1), skw["lr"])
    if "numpy_seed" in case:
        np.random.seed(case["numpy_seed"])
    init_fp = mg.param_fingerprint(model.V)
    model.train()
    xp = (0.4 if elliptic else 1.0) * mg.probe_points(problem.d)
    res = {"probe_x": mg.f32list(xp)}
    if not elliptic:
        res["probe_t"] = 0.5 * problem.T
        xp = torch.cat([xp, torch.full((xp.shape[0], 1), 0.5 * problem.T)], 1)
    with torch.no_grad():
        v = model.V(xp).squeeze()
    res.update({
        "loss_log": [float(v_) for v_ in model.loss_log], "V_L2_log": [float(v_) for v_ in model.V_L2_log],
        "K": int(model.K), "K_log": [int(v_) for v_ in model.K_log],
        "loss_log_domain": [float(v_) for v_ in model.loss_log_domain],
        "loss_log_boundary": [float(v_) for v_ in model.loss_log_boundary],
        "V_test_L2": [float(v_) for v_ in model.V_test_L2], "V_test_abs": [float(v_) for v_ in model.V_test_abs],
        "init_params": init_fp, "final_params": mg.param_fingerprint(model.V), "probe_V": mg.f32list(v),
    })
    return res


def main():
    torch.set_num_threads(1)
    warnings.filterwarnings("ignore")
    only = set(sys.argv[1:])
    for case in CASES:
        if only and case["name"] not in only:
            continue
        print("running", case["name"], flush=True)
        res = run_case(case)
        with open(os.path.join(HERE, case["name"] + ".json"), "w") as fh:
            json.dump({"case": case, "expected": res, "torch": torch.__version__}, fh, indent=1)
        print("   loss_log", res["loss_log"], "K", res["K"], flush=True)


if __name__ == "__main__":
    main()
