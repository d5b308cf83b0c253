"""Goldens of the remaining double-well problems (DoubleWell_OU, DoubleWell_multidim_2, DoubleWell_multidim_3) and of
LLGC_general_f: the reference's own Solver with its constructor defaults (time_approx='outer', one DenseNet per step) on its own
classes, on CPU through make_golden's proxy.  A separate script so that make_golden.py, index.json and the fixtures they write
stay as they are; the records have the layout of make_golden's solver cases, plus ``probes`` of the problem's own functions
(b, g, h and, where it evaluates, u_true on make_golden.probe_points).

Every class at K = 37, N = 4 (T = 0.2, dt = 0.05), L = 3, in four flag combinations: the constructor defaults (attached forward
process, log-variance), detach_forward=True, the moment loss on a non-adaptive process, and the relative entropy.  u_L2 is logged
for OU and _3 (after their reference-solution calls) and off for _2, whose u_true cannot be broadcast by the reference's own log
line.  LLGC_general_f is NaN from its second iteration on (|z|^1.25 has no gradient at the initial z = 0): one iteration only.

    python tests/golden/make_golden_wells.py [case names]
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

BASE = dict(L=3, K=37, delta_t=0.05, seed=42, lr=0.005)
FLAGS = dict(
    default=dict(),
    detached=dict(detach_forward=True),
    moment_nonadaptive=dict(loss_method="moment", adaptive_forward_process=False),
    relent=dict(loss_method="relative_entropy"),
)
PROBLEMS = dict(
    ou_d3=dict(kind="DoubleWell_OU", kwargs=dict(d=3, T=0.2, alpha=1.0, kappa=2.0),
               calls=[["compute_reference_solution_x_1", dict(nx=400)]]),
    ou_d20=dict(kind="DoubleWell_OU", kwargs=dict(d=20, T=0.2, alpha=0.5, kappa=1.0),
                calls=[["compute_reference_solution_x_1", dict(nx=400)]]),
    dw3_d5=dict(kind="DoubleWell_multidim_3", kwargs=dict(d=5, T=0.2, eta=0.5, kappa=2.0),
                calls=[["compute_reference_solution", dict(nx=400)]]),
    radial_d4=dict(kind="DoubleWell_multidim_2", kwargs=dict(d=4, T=0.2, alpha=1.0, kappa=1.0)),
    radial_d20=dict(kind="DoubleWell_multidim_2", kwargs=dict(d=20, T=0.2, alpha=0.5, kappa=0.5)),
)

CASES = [dict(name="wells_%s_%s" % (p, f), family="solver", problem=PROBLEMS[p],
              solver=dict(BASE, u_l2_error_flag=not p.startswith("radial"), **FLAGS[f]))
         for p in PROBLEMS for f in FLAGS]
CASES.append(dict(name="wells_llgc_general_f_d3", family="solver",
                  problem=dict(kind="LLGC_general_f", kwargs=dict(d=3, off_diag=0.1, T=0.2, seed=42)),
                  solver=dict(BASE, L=1, u_l2_error_flag=False)))


def problem_probes(problem):
    """The problem's own coefficient functions on fixed points: what a port has to reproduce."""
    x = mg.probe_points(problem.d, n=6, seed=11)
    x[-1] = 3.0 * x[-1]                                   # one point well outside the unit ball / beyond the wells
    z = mg.probe_points(problem.d, n=6, seed=12)
    t = torch.tensor(0.1)
    out = {"x": mg.f32list(x), "z": mg.f32list(z), "t": 0.1, "X_0": mg.f32list(problem.X_0),
           "b": mg.f32list(problem.b(x)), "g": mg.f32list(problem.g(x)),
           "h": mg.f32list(problem.h(t, x, torch.zeros(6), z)), "f": mg.f32list(problem.f(x, t))}
    try:
        u = np.asarray(problem.u_true(x, 0.1), dtype=np.float64)
        out["u_true"], out["u_true_shape"] = [float(v) for v in u.reshape(-1)], list(u.shape)
    except Exception as e:                                # (a class whose tables were not computed)
        out["u_true"], out["u_true_error"] = None, type(e).__name__
    return out


def main():
    torch.set_num_threads(1)
    warnings.filterwarnings("ignore")
    only = set(sys.argv[1:])
    for case in CASES:
        if only and case["name"] not in only:
            continue
        print("running", case["name"], flush=True)
        res = mg.run_solver_case(case)
        res["problem_probes"] = problem_probes(mg.make_problem(case["problem"]))
        print("   loss_log", res["loss_log"], "u_L2", res["u_L2_loss"], flush=True)
        with open(os.path.join(HERE, case["name"] + ".json"), "w") as fh:
            json.dump({"case": case, "expected": res, "torch": torch.__version__}, fh, indent=1)


if __name__ == "__main__":
    main()
