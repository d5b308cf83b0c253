"""The direction-table statement (ref64_pinn_dense.py) against what it must agree with: ref64_pinn's scaled statement for
u_j = s e_j, trace(B B^T Hess V) by torch.autograd.functional.hessian, and the plan's eigh factor.  No GPU."""
import pytest
import torch

import ref64_pinn as r64
import ref64_pinn_dense as r64d
from pinn_hessian_kernel_cases import full_rank_B, ones_B


@pytest.mark.parametrize("kw", [
    dict(d=5, parabolic=False, arch=[8, 6], K=7, act="tanh", seed=1, h_kind=r64.H_ALLEN_CAHN, drift_kind=r64.DRIFT_DWELL, s=1.25),
    dict(d=4, parabolic=True, arch=[9], K=6, act="tanh2", seed=2, linear=True, h_kind=r64.H_EXP_SIN, h_par=(0.3, 4.0, 0.5, 0.0),
         drift_kind=r64.DRIFT_DIAG),
], ids=["elliptic", "parabolic"])
def test_scaled_unit_directions_give_the_scaled_statement(kw):
    case = r64.make_case(**kw)
    dense = dict(case, dirs=case["s"] * torch.eye(case["d"], dtype=torch.float64))
    V, g, lap, R = r64.parts(case)
    Vd, gd, second, Rd = r64d.parts(dense)
    assert torch.equal(V, Vd) and torch.equal(g, gd)
    tol = 64 * torch.finfo(torch.float64).eps
    assert float((second - case["s"] ** 2 * lap).abs().max()) <= tol * float(second.abs().max())
    assert float((R - Rd).abs().max()) <= tol * float(R.abs().max())
    w = torch.linspace(-1.0, 1.0, case["K"], dtype=torch.float64)
    ga, gb = r64.weighted_grad(case, w), r64d.weighted_grads(dense, [w])[0]
    assert float((ga - gb).abs().max()) <= tol * float(ga.abs().max())


@pytest.mark.parametrize("B", [ones_B(4), full_rank_B(4, 11)], ids=["ones", "full rank"])
def test_directions_give_the_trace_of_the_hessian_form(B):
    case = r64d.make_case(r64d.eigh_factor(B), d=4, parabolic=False, arch=[10, 7], K=6, act="tanh", seed=3)
    case["dirs"] = r64d.eigh_factor(B)                              # unrounded: float64 against float64
    second = r64d.parts(case)[2]
    want = r64d.trace_form(case, B)
    assert float((0.5 * second - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("d", [4, 20])
def test_eigh_factor_of_the_ones_matrix_is_one_direction(d):
    U = r64d.eigh_factor(ones_B(d))
    assert U.shape == (1, d)
    U = U * torch.sign(U[0, 0])
    assert float((U - 2.0 ** 0.5).abs().max()) <= 1e-14
    B = full_rank_B(5, 7)
    U = r64d.eigh_factor(B)
    assert U.shape == (5, 5) and float((U.t() @ U - B @ B.t()).abs().max()) <= 1e-14
