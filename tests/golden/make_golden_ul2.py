"""Goldens of the u_L2 log with a DenseNet control (time_approx='outer', and a DenseNet swapped into z_n): the reference's
own Solver runs, made with make_golden.run_solver_case.  A separate script so that make_golden.py, index.json and the
fixtures it writes stay as they are.

    python tests/golden/make_golden_ul2.py [case names]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as mg  # noqa: E402

DW1 = dict(loss_method="log-variance", time_approx="inner", adaptive_forward_process=True, detach_forward=True,
           early_stopping_time=None)

CASES = [
    # the literal constructor defaults (outer, attached, log-variance, u_L2 on); K not a multiple of 16
    dict(name="llgc_d12_outer_ul2", family="solver",
         problem=dict(kind="LLGC", kwargs=dict(d=12, off_diag=0.05, T=0.2, seed=42)),
         solver=dict(L=4, lr=0.003, K=90, delta_t=0.02, seed=42)),
    # the first cell of the LQGC notebook with L reduced: the gain row is ceil(t / 0.005) with solver dt 0.01; dense B
    dict(name="lqgc_d10_outer_ul2", family="solver",
         problem=dict(kind="LQGC", kwargs=dict(d=10, off_diag=0.1, T=0.5, seed=42, delta_t=0.005)),
         solver=dict(loss_method="moment", learn_Y_0=True, detach_forward=True, L=3, lr=0.003, K=100, delta_t=0.01, seed=42)),
    # two grid tables and a coordinate map; relative entropy
    dict(name="dw_d6_mixed_outer_ul2", family="solver",
         problem=dict(kind="DoubleWell_multidim", kwargs=dict(d=6, d_1=2, d_2=4, T=0.3, eta=0.5, kappa=2.0),
                      calls=[["compute_reference_solution", dict(nx=500)], ["compute_reference_solution_2", dict(nx=500)]]),
         solver=dict(loss_method="relative_entropy", L=3, lr=0.005, K=96, delta_t=0.01, seed=42)),
    # a DenseNet(d+1 -> d) in z_n at d = 1: the last trajectory's cell shift is the whole state
    dict(name="dw1d_densenet_inner_ul2", family="solver",
         problem=dict(kind="DoubleWell", kwargs=dict(d=1, T=0.4, eta=3.0, kappa=5.0),
                      calls=[["compute_reference_solution", dict(nx=400)]]),
         solver=dict(DW1, L=4, lr=0.005, K=112, delta_t=0.01, seed=42),
         net=dict(kind="densenet", arch=[20, 20], seed=7), probe_times=[0.0, 0.2]),
    # d = 100 with the default [30, 30] nets: the padded (112, 32) instance
    dict(name="llgc_d100_outer_ul2", family="solver",
         problem=dict(kind="LLGC", kwargs=dict(d=100, off_diag=0.01, T=0.1, seed=42)),
         solver=dict(L=2, lr=0.001, K=48, delta_t=0.01, seed=42)),
]


def main():
    torch.set_num_threads(1)
    only = set(sys.argv[1:])
    for case in CASES:
        if only and case["name"] not in only:
            continue
        print("running", case["name"], flush=True)
        res = mg.run_solver_case(case)
        with open(os.path.join(HERE, case["name"] + ".json"), "w") as fh:
            json.dump({"case": case, "expected": res, "torch": torch.__version__}, fh, indent=1)
        print("   loss_log", res["loss_log"], "u_L2", res["u_L2_loss"], flush=True)


if __name__ == "__main__":
    main()
