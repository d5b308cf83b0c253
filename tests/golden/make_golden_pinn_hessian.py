"""Golden of the full-Hessian PINN with a full-rank diffusion matrix: the reference's own EllipticSolver ``train()`` with
``loss_method='PINN'`` and ``full_hessian=True`` (one autograd.functional.hessian call per sample), on CPU through make_golden's
proxy.  The problem is ExponentialOnBallNonlinearSinHessian with its ``B`` replaced by a seeded full-rank matrix (the reference's h
does not read B), so trace(B B^T Hess V) needs d = 15 second-order directions: two blocks of the native kernels.  A separate
script so that make_golden_pinn.py and the fixtures it writes stay as they are.  Data only: the case with B, the logs, probe
values, fingerprints.

    python tests/golden/make_golden_pinn_hessian.py
"""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as mg  # noqa: E402
import make_golden_pinn as mgp  # noqa: E402

D, B_SEED = 15, 15


def seeded_B(d=D, seed=B_SEED):
    g = torch.Generator().manual_seed(seed)
    return ((2.0 / d) ** 0.5 * torch.randn(d, d, generator=g)).float()


CASE = dict(name="pinn_expball_hess_d15_dense", family="elliptic",
            problem=dict(kind="ExponentialOnBallNonlinearSinHessian", kwargs=dict(d=D, alpha=0.5), B=seeded_B().tolist()),
            solver=dict(mgp.S, alpha=[1.0, 1.0], full_hessian=True))


def main():
    torch.set_num_threads(1)
    warnings.filterwarnings("ignore")
    B = torch.tensor(CASE["problem"]["B"])
    assert int(torch.linalg.matrix_rank(B.double())) == D
    make_problem = mg.make_problem

    def with_B(spec):                                             # run_case builds the problem itself: hand it this B
        pb = make_problem(spec)
        pb.B = torch.tensor(spec["B"])
        return pb

    mg.make_problem = with_B
    try:
        res = mgp.run_case(CASE)
    finally:
        mg.make_problem = make_problem
    with open(os.path.join(HERE, CASE["name"] + ".json"), "w") as fh:
        json.dump({"case": CASE, "expected": res, "torch": torch.__version__}, fh, indent=1)
    print("   loss_log", res["loss_log"], "K", res["K"], flush=True)


if __name__ == "__main__":
    main()
