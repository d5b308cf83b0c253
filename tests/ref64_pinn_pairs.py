"""Float64 (or any dtype) torch-autograd statement of the PINN loss with an h that reads t -- what the pair kernels
(csrc/pinn_kernels.h, psp_pinn_pairs_*) are tested against.

The reference hands h the times as a (K, 1) column (solver.py:1284-1285), so with i over the times and j over the samples

    R[i, j] = A_j + nl(exp(2 al |x_j|^2 + 2 tau t_i) - y_j^2)        nl = identity (H_EXP_SQ) or sin (H_EXP_SIN)
    y_j = V(x_j, t_j),   A_j = dV/dt_j + s^2/2 Lap V_j + b . grad V_j - y_j (2 al (2 al |x_j|^2 + dd) + e)
    loss = alpha0 mean_ij R[i, j]^2

``broadcast`` states exactly that, by nested autograd as ref64_pinn does.  ``statement`` adds the factorisation the kernels use:
rho_j = 2 alpha0 / K^2 sum_i R[i, j], nu_j = 2 alpha0 / K^2 sum_i R[i, j] nl'(arg_ij) (-2 y_j) and the gradient
sum_j (rho_j dA_j/dtheta + nu_j dy_j/dtheta).  ``transposed=True`` is a deliberately wrong twin: it pairs t_j with sample i
(R'[i, j] = A_i + nl(exp(2 al |x_i|^2 + 2 tau t_j) - y_i^2) = R[j, i]) and reduces over i all the same -- what a kernel
computes that mixes up which index is staged per workgroup and which per wave.  Its loss is the true one (a transposed matrix
has the same mean square) and at K = 1 it is the true statement altogether; rho, nu and the gradient are wrong from K = 2 on.
"""
import functools

import torch

import ref64_pinn as r64
from pinn_kernel_cases import row

ALPHA0 = 1.3

# name -> make_case arguments (h_par = (al, dd, e, tau)); al = 0.05 keeps the sine's argument O(1) on (-1, 1)^d.
# golden_shape has the golden's al = 0.7 and T = 0.5: the exponential reaches 11, and what fp32 does to nu (a sum of R cos(arg)
# with cancellation) varies from 4e-7 to 3e-5 with the seed; its seed is one whose fp32 statement keeps the regime cap
# (pinn_kernel_cases.REGIME_CAP, asserted in test_ref64_pinn_pairs.py), chosen on the statements alone.
CASES = {
    "k1": dict(d=2, arch=[5], K=1, act="tanh", seed=0, h_kind=r64.H_EXP_SIN, h_par=(0.05, 2.0, 1.0, 1.0)),
    "k63": dict(d=3, arch=[8], K=63, act="tanh", seed=0, h_kind=r64.H_EXP_SIN, h_par=(0.05, 3.0, 1.0, 1.0)),
    "k64": dict(d=3, arch=[8], K=64, act="tanh", seed=0, h_kind=r64.H_EXP_SQ, h_par=(0.05, 3.0, 1.0, 1.0)),
    "k65": dict(d=3, arch=[8], K=65, act="relu2", seed=0, h_kind=r64.H_EXP_SIN, h_par=(0.05, 3.0, 1.0, 1.0)),
    "k257_sin": dict(d=3, arch=[8], K=257, act="tanh", seed=0, h_kind=r64.H_EXP_SIN, h_par=(0.05, 3.0, 1.0, 1.0)),
    "k521_sq_tau": dict(d=15, arch=[16], K=521, act="tanh", seed=0, linear=True, h_kind=r64.H_EXP_SQ,
                        h_par=(0.05, 15.0, -0.5, 0.5)),
    "k33_tanh2": dict(d=15, arch=[16, 16], K=33, act="tanh2", seed=0, h_kind=r64.H_EXP_SIN, h_par=(0.05, 15.0, 1.0, 1.0)),
    "golden_shape": dict(d=3, arch=[30, 30], K=24, act="relu2", seed=7, h_kind=r64.H_EXP_SIN, h_par=(0.7, 3.0, 1.0, 1.0),
                         T=0.5),
}


def make(name):
    kw = dict(CASES[name])
    T = kw.pop("T", 1.0)
    case = r64.make_case(parabolic=True, **kw)
    case["t"] = (case["t"].float() * T).double()                   # fp32-representable times in (0, T)
    return case


def _nl(case, arg):
    return (arg, torch.ones_like(arg)) if case["h_kind"] == r64.H_EXP_SQ else (torch.sin(arg), torch.cos(arg))


def per_sample(case, params, dtype):
    """(y (K,), A (K,)) on the graph of ``params``: the residual of ref64_pinn with the linear part of h only."""
    assert case["parabolic"] and case["h_kind"] in (r64.H_EXP_SQ, r64.H_EXP_SIN)
    V, _, _, A = r64.terms(dict(case, h_kind=r64.H_EXP_LIN), params, dtype)
    return V, A


def matrix(case, V, A, dtype, transposed=False):
    """(R (K, K), nl' (K, K)) with [i, j] = (time i, sample j), written as the broadcast the reference's h performs on
    t (K, 1) against x (K, d) and y (K,); ``transposed``: the wrong twin, sample i with time j."""
    al, tau = case["h_par"][0], case["h_par"][3]
    rr = torch.sum(case["x"].to(dtype) ** 2, 1)
    t = case["t"].to(dtype).reshape(-1, 1)
    if transposed:
        arg = torch.exp(2 * al * rr.reshape(-1, 1) + 2 * tau * t.reshape(1, -1)) - V.reshape(-1, 1) ** 2
        val, der = _nl(case, arg)
        return A.reshape(-1, 1) + val, der
    arg = torch.exp(2 * al * rr + 2 * tau * t) - V ** 2             # (K,) + (K, 1) -> (K, K)
    val, der = _nl(case, arg)
    return A + val, der


def broadcast(case, alpha0=ALPHA0, dtype=torch.float64):
    """(loss, flat gradient) of alpha0 mean(R^2) over the (K, K) matrix, by autograd through the broadcast."""
    params = [p.to(dtype).clone().requires_grad_(True) for p in case["params"]]
    V, A = per_sample(case, params, dtype)
    loss = alpha0 * torch.mean(matrix(case, V, A, dtype)[0] ** 2)
    return loss.detach(), r64.flat_grad(torch.autograd.grad(loss, params, allow_unused=True), params)


def statement(case, alpha0=ALPHA0, dtype=torch.float64, transposed=False):
    """dict(A, V, rho, nu (K,), loss (1,), grad (P,) factorised, grad_broadcast (P,)), detached, as float64 tensors of numbers
    computed in ``dtype``."""
    params = [p.to(dtype).clone().requires_grad_(True) for p in case["params"]]
    V, A = per_sample(case, params, dtype)
    K = case["K"]
    R, der = matrix(case, V.detach(), A.detach(), dtype, transposed)
    c = 2.0 * alpha0 / (K * K)
    rho = c * R.sum(0)
    nu = c * (R * der).sum(0) * (-2.0 * V.detach())
    loss = alpha0 * torch.mean(R ** 2)
    grad = r64.flat_grad(torch.autograd.grad(torch.sum(rho * A) + torch.sum(nu * V), params, allow_unused=True), params)
    out = dict(A=A, V=V, rho=rho, nu=nu, loss=loss.reshape(1), grad=grad, grad_broadcast=broadcast(case, alpha0, dtype)[1])
    return {k: v.detach().double() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(case, f64, f32): computed once per case, never modified."""
    case = make(name)
    return dict(name=name, case=case, f64=statement(case), f32=statement(case, dtype=torch.float32))


def evaluate(ref, got):
    """Rows (label, e_native, e_fp32, bound, ok) of pinn_kernel_cases.row for A, rho, nu, the loss and every named block of the
    gradient.  ``got``: A, rho, nu (K,), loss (1,), grad (P,).  The fp32 yardstick of the gradient is autograd through the
    broadcast; a single-entry block takes the worse of that and the factorised fp32 gradient (pinn_kernel_cases.row)."""
    case, f64, f32 = ref["case"], ref["f64"], ref["f32"]
    rows = [row(k, got[k], f64[k], f32[k]) for k in ("A", "rho", "nu", "loss")]
    g, g32, other = (r64.blocks(case, v) for v in (got["grad"], f32["grad_broadcast"], f32["grad"]))
    for blk, v64 in r64.blocks(case, f64["grad_broadcast"]).items():
        rows.append(row("grad " + blk, g[blk], v64, g32[blk], other[blk]))
    return rows


def worst_miss(rows):
    """max over the rows of e_native / bound: <= 1 passes."""
    return max((r[1] / r[3]) if r[3] > 0.0 else (0.0 if r[4] else float("inf")) for r in rows)

