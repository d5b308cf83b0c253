"""Goldens of the u_L2 log with the value-function ansatz (approx_method='value_function', time_approx='inner', the u_L2 flag
left at its default: on): the reference's own Solver runs, made with make_golden.run_solver_case.  A separate script so that
make_golden.py, index.json and the fixtures it writes stay as they are.

    python tests/golden/make_golden_value_ul2.py [case names]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as mg  # noqa: E402

VF = dict(approx_method="value_function", time_approx="inner", early_stopping_time=None, seed=42)

CASES = [
    # a table of u*(t_n) on the linear-quadratic instance (dense A and B); ragged last tile (8 live rows)
    dict(name="llgc_d8_off_value_ul2", family="solver",
         problem=dict(kind="LLGC", kwargs=dict(d=8, off_diag=0.1, T=0.4, seed=42)),
         solver=dict(VF, loss_method="log-variance", adaptive_forward_process=True, detach_forward=True, L=3, lr=0.005, K=40,
                     delta_t=0.02)),
    # the gains of a u* linear in x: the gain row ceil(t / 0.005) differs from the step index; the running cost
    dict(name="lqgc_d5_value_ul2", family="solver",
         problem=dict(kind="LQGC", kwargs=dict(d=5, off_diag=0.1, T=0.5, seed=42, delta_t=0.005)),
         solver=dict(VF, loss_method="moment", adaptive_forward_process=True, detach_forward=True, L=3, lr=0.005, K=40,
                     delta_t=0.01)),
    # the gain product across two 16-blocks (the time row must not enter it); a three-layer value net
    dict(name="lqgc_d17_arch3_value_ul2", family="solver",
         problem=dict(kind="LQGC", kwargs=dict(d=17, off_diag=0.05, T=0.3, seed=42, delta_t=0.05)),
         solver=dict(VF, loss_method="log-variance", adaptive_forward_process=True, detach_forward=True, L=2, lr=0.005, K=24,
                     delta_t=0.05),
         net=dict(kind="value_densenet", arch=[20, 16, 12], seed=7)),
    # two grid tables and a coordinate map on the sigma = s I instance; the last global trajectory in a ragged tile
    dict(name="dw_d6_mixed_value_ul2", family="solver",
         problem=dict(kind="DoubleWell_multidim", kwargs=dict(d=6, d_1=2, d_2=4, T=0.3, eta=0.5, kappa=2.0),
                      calls=[["compute_reference_solution", dict(nx=500)], ["compute_reference_solution_2", dict(nx=500)]]),
         solver=dict(VF, loss_method="log-variance", adaptive_forward_process=True, detach_forward=True, L=3, lr=0.005, K=90,
                     delta_t=0.01)),
    # d = 1: the last trajectory's cell shift is the whole state
    dict(name="dw1d_value_ul2", family="solver",
         problem=dict(kind="DoubleWell", kwargs=dict(d=1, T=0.4, eta=3.0, kappa=5.0),
                      calls=[["compute_reference_solution", dict(nx=400)]]),
         solver=dict(VF, loss_method="log-variance", adaptive_forward_process=True, detach_forward=True, L=3, lr=0.005, K=112,
                     delta_t=0.01)),
    # a table of u*(t_n) on the sigma = s I instance, c = 0; the default [30, 30] net (the templated family with the log off)
    dict(name="llgc_d8_diag_value_ul2", family="solver",
         problem=dict(kind="LLGC", kwargs=dict(d=8, off_diag=0.0, T=0.4, seed=42)),
         solver=dict(VF, loss_method="moment", adaptive_forward_process=False, detach_forward=False, L=3, lr=0.003, K=80,
                     delta_t=0.02)),
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
