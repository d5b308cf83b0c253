"""Goldens of the naive and reference-control importance-sampling estimators: the reference's own
utilities.do_importance_sampling_me with simulate_naive=True, verbose=True and a cross_statistics threshold, made with
make_golden's problems and solvers.  A separate script so that make_golden.py, index.json and the fixtures it writes stay as
they are.  The crossing counts are parsed from the printed lines.

    python tests/golden/make_golden_is_naive.py [case names]
"""
import contextlib
import io
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as mg  # noqa: E402

NOTRAIN = dict(L=0, lr=0.001, K=16, loss_method="log-variance", time_approx="inner", adaptive_forward_process=True,
               detach_forward=True, early_stopping_time=None)

CASES = [
    # a: the paper notebook's call (Double well - 1d - high metastability.ipynb, cell 3), K scaled down
    dict(name="is_naive_dw1d_true", problem=dict(kind="DoubleWell", kwargs=dict(d=1, T=1, eta=3.0, kappa=5.0),
                                                 calls=[["compute_reference_solution", {}]]),
         solver=dict(NOTRAIN, delta_t=0.01, seed=42), is_K=2048, is_delta_t=0.01, control="true", cross=[[0.0]], is_seed=3),
    # b: two grid tables
    dict(name="is_naive_dw4_true", problem=dict(kind="DoubleWell_multidim", kwargs=dict(d=4, d_1=2, d_2=2, T=0.5, eta=2.0, kappa=3.0),
                                                calls=[["compute_reference_solution", {}], ["compute_reference_solution_2", {}]]),
         solver=dict(NOTRAIN, delta_t=0.01, seed=42), is_K=2048, is_delta_t=0.01, control="true", cross=[[0.0]], is_seed=4),
    # c: u* independent of x, dense A and B
    dict(name="is_naive_llgc6_true", problem=dict(kind="LLGC", kwargs=dict(d=6, off_diag=0.1, T=0.5, seed=42)),
         solver=dict(NOTRAIN, delta_t=0.01, seed=42), is_K=2048, is_delta_t=0.01, control="true", cross=[[0.0]], is_seed=5),
    # d: u* = M_n x with gain row ceil(t / 0.005), a running cost
    dict(name="is_naive_lqgc3_true", problem=dict(kind="LQGC", kwargs=dict(d=3, off_diag=0.1, T=0.5, seed=42, delta_t=0.005)),
         solver=dict(NOTRAIN, delta_t=0.01, seed=42), is_K=2048, is_delta_t=0.01, control="true", cross=[[0.0]], is_seed=6),
    # e: the learned control after three iterations, naive next to IS
    dict(name="is_naive_llgc20_approx", problem=dict(kind="LLGC", kwargs=dict(d=20, off_diag=0.1, T=0.3, seed=42)),
         solver=dict(NOTRAIN, L=3, lr=0.003, K=64, delta_t=0.01, seed=42), is_K=2048, is_delta_t=0.01, control="approx",
         cross=[[0.0]], is_seed=7),
]


def run_case(case):
    problem = mg.make_problem(case["problem"])
    model = mg.ref_sv.Solver(name=case["name"], problem=problem, verbose=False, **case["solver"])
    model.train()
    torch.manual_seed(case["is_seed"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = mg.ref_ut.do_importance_sampling_me(problem, model, case["is_K"], control=case["control"], simulate_naive=True,
                                                  verbose=True, delta_t=case["is_delta_t"],
                                                  cross_statistics=torch.tensor(case["cross"]))
    text = buf.getvalue()
    crossed = [int(m) for m in re.findall(r"crossed: (\d+)/", text)]
    keys = ["mean_naive", "variance_naive", "rel_error_naive", "mean_IS", "variance_IS", "rel_error_IS"]
    return dict({k: float(v) for k, v in zip(keys, res)}, crossed_naive=crossed[0], crossed_IS=crossed[1], printed=text)


def main():
    torch.set_num_threads(1)
    only = set(sys.argv[1:])
    for case in CASES:
        if only and case["name"] not in only:
            continue
        print("running", case["name"], flush=True)
        res = run_case(case)
        with open(os.path.join(HERE, case["name"] + ".json"), "w") as fh:
            json.dump({"case": case, "expected": res, "torch": torch.__version__}, fh, indent=1)
        print(res["printed"], flush=True)


if __name__ == "__main__":
    main()
