"""The full-Hessian PINN goldens and how a test turns one into a package solver: pinn_cases.build, plus the diffusion matrix a
fixture carries as data (tests/golden/make_golden_pinn_hessian.py)."""
import torch

import pinn_cases

# EllipticSolver(full_hessian=True) on a dense sigma: the ones matrix of the notebook (rank 1) and a seeded full-rank B (d = 15)
GOLDENS = ["pinn_expball_hess_d4_full", "pinn_expball_hess_d15_dense"]


def build(case, device="cpu", backend="auto", hessian="directions", **over):
    """``hessian='directions'``: the switch that lets full_hessian=True onto the native plan (the default keeps the reference's
    sample-by-sample Hessian, which tests/test_gpu_pinn.py pins)."""
    if case["family"] == "elliptic":
        over["hessian"] = hessian
    prob, model = pinn_cases.build(case, device=device, backend=backend, **over)
    if "B" in case["problem"]:
        prob.B = torch.tensor(case["problem"]["B"]).to(prob.device)
    return prob, model
