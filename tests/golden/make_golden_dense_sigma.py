"""Goldens of the elliptic problem with a full Hessian (`Nonlinear toy problem - elliptic with full Hessian.ipynb`): the
reference's own EllipticSolver on its ExponentialOnBallNonlinearSinHessian, whose diffusion matrix is the dense
sqrt(2 / d) ones(d, d).  A separate script so that make_golden.py, index.json and the fixtures it writes stay as they are;
the records have the layout of make_golden's elliptic cases plus ``min_exit_margin``.

Exit-margin condition: with a dense sigma a GPU rollout forms X_n by fp32 MFMA products where the reference calls torch.mm, so
X_n differs in its last bits, and the sphere test |X_n| < 1 decides K_log.  The script records
min | |X_n| - 1 | over every (k, n >= 1) the reference tests (a wrapper around the problem's h sees each X; a stopped trajectory
keeps the X it stopped with, which was counted while it was active) and refuses to write a fixture whose margin is below
1e-5 -- about a hundred fp32 ulps at 1: then take the next seed.

    python tests/golden/make_golden_dense_sigma.py [case names]
"""
import contextlib
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as mg  # noqa: E402

MIN_MARGIN = 1e-5

CASES = [
    # the notebook's diffusion configuration (cell 2: d = 20, K = 200, N = 20, delta_t = 0.001, alpha = [0.1, 1.0]), K_test_log
    # scaled down
    dict(name="expball_hess_d20_elliptic_diffusion", family="elliptic",
         problem=dict(kind="ExponentialOnBallNonlinearSinHessian", kwargs=dict(d=20)),
         solver=dict(seed=42, delta_t=0.001, N=20, lr=0.001, L=3, K=200, K_boundary=50, alpha=[0.1, 1.0],
                     loss_method="diffusion", K_test_log=500)),
    # BSDE loss: N large enough that every trajectory leaves the ball
    dict(name="expball_hess_d5_elliptic_bsde", family="elliptic",
         problem=dict(kind="ExponentialOnBallNonlinearSinHessian", kwargs=dict(d=5, alpha=0.5)),
         solver=dict(seed=42, delta_t=0.01, N=400, lr=0.001, L=3, K=64, K_boundary=20, loss_method="BSDE")),
    dict(name="expball_hess_d4_elliptic_neumann", family="elliptic",
         problem=dict(kind="ExponentialOnBallNonlinearSinHessian", kwargs=dict(d=4, alpha=0.5, boundary_type="Neumann")),
         solver=dict(seed=42, delta_t=0.01, N=15, lr=0.001, L=3, K=64, K_boundary=20, loss_method="diffusion",
                     boundary_type="Neumann", alpha=[1.0, 0.5], adaptive_forward_process=True)),
]


def run_case(case):
    """make_golden.run_elliptic_case with the margin recorder around problem.h."""
    problem = mg.make_problem(case["problem"])
    model = mg.ref_sv.EllipticSolver(problem=problem, name=case["name"], verbose=False, **case["solver"])
    state = dict(iteration=-1, n=0, margin=float("inf"))
    h_ref = problem.h

    def h(x, y, z):
        it = len(model.loss_log)
        if it != state["iteration"]:
            state["iteration"], state["n"] = it, 0
        if state["n"] >= 1:
            r = torch.sqrt(torch.sum(x.detach().double() ** 2, 1))
            state["margin"] = min(state["margin"], float(torch.min(torch.abs(r - problem.boundary_distance))))
        state["n"] += 1
        return h_ref(x, y, z)

    problem.h = h
    init_fp = mg.param_fingerprint(model.V)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model.train()
    if "Not all trajectories stopped" in buf.getvalue():
        raise RuntimeError("%s: N is too small, not every trajectory left the ball" % case["name"])
    xp = 0.4 * mg.probe_points(problem.d)
    with torch.no_grad():
        v = model.V(xp).squeeze()
    return {
        "loss_log": [float(v_) for v_ in model.loss_log],
        "K_log": [int(v_) for v_ in model.K_log],
        "V_L2_log": [float(v_) for v_ in model.V_L2_log],
        "V_test_L2": [float(v_) for v_ in model.V_test_L2], "V_test_abs": [float(v_) for v_ in model.V_test_abs],
        "init_params": init_fp, "final_params": mg.param_fingerprint(model.V),
        "probe_x": mg.f32list(xp), "probe_V": mg.f32list(v),
        "min_exit_margin": state["margin"],
    }


def main():
    torch.set_num_threads(1)
    only = set(sys.argv[1:])
    for case in CASES:
        if only and case["name"] not in only:
            continue
        print("running", case["name"], flush=True)
        res = run_case(case)
        print("  K_log", res["K_log"], "min_exit_margin %.3e" % res["min_exit_margin"], flush=True)
        if not res["min_exit_margin"] >= MIN_MARGIN:
            raise RuntimeError("%s: exit margin %.3e below %.0e -- take the next seed" % (case["name"], res["min_exit_margin"], MIN_MARGIN))
        with open(os.path.join(HERE, case["name"] + ".json"), "w") as fh:
            json.dump({"case": case, "expected": res, "torch": torch.__version__}, fh, indent=1)


if __name__ == "__main__":
    main()
