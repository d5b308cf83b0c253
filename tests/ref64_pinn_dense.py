"""Float64 (or any dtype) torch-autograd statement of the PINN residual with second-order DIRECTIONS, and of the parameter gradient
of its loss -- what the direction-table route of the forward-Laplacian kernels (csrc/pinn_kernels.h) is tested against.

    R_k = [dV/dt] + 1/2 sum_j u_j^T (Hess_x V) u_j + b(x) . grad_x V + h(x, V)

A case is ref64_pinn.make_case's dict plus ``dirs`` (n_hess, d), float64.  With sum_j u_j u_j^T = B B^T the second-order term is
1/2 trace(B B^T Hess_x V), a dense sigma B.  Nested autograd: one directional second derivative u . grad(u . grad V) per row of
``dirs``.  Gradients are weighted by rbar as ref64_pinn does; blocks / one_hot / the rbar forms are ref64_pinn's own.
"""
import torch

import ref64_pinn as r64

H_EXP_SIN_FULL = 6              # PSP_GH_EXPBALL_SIN_FULL: (sum_i x_i)^2 in the linear part of h, |x|^2 kept in the exponent


def h_pde(kind, par, x, y):
    if kind == H_EXP_SIN_FULL:
        al, dd, e = par[0], par[1], par[2]
        lin = 2.0 * al * (2.0 * al * torch.sum(x, 1) ** 2 + dd) + e
        return torch.sin(torch.exp(2.0 * al * torch.sum(x ** 2, 1)) - y ** 2) - y * lin
    assert kind != r64.H_QUAD, "an h that reads z is outside the direction-table route"
    return r64.h_pde(kind, par, x, y, None)


def terms(case, params=None, dtype=torch.float64, create_graph=True, preacts=None):
    """(V (K,), grad V (K, n_in), sum_j u_j^T Hess_x V u_j (K,), R (K,)) of ``case`` in ``dtype``, on the graph of ``params``."""
    if params is None:
        params = [p.to(dtype) for p in case["params"]]
    d = case["d"]
    x = case["x"].to(dtype)
    cols = [x] + ([case["t"].to(dtype).reshape(-1, 1)] if case["parabolic"] else [])
    inp = torch.cat(cols, 1).requires_grad_(True)
    V = r64.net(params, case["act"], inp, case["linear"], preacts)
    g, = torch.autograd.grad(V.sum(), inp, create_graph=True)
    second = torch.zeros_like(V)
    for u in case["dirs"].to(dtype):
        gu = torch.sum(g[:, :d] * u, 1)
        second = second + torch.sum(torch.autograd.grad(gu.sum(), inp, create_graph=create_graph, retain_graph=True)[0][:, :d] * u, 1)
    xs = inp[:, :d].detach()
    vec = None if case["drift"] is None else case["drift"].to(dtype)
    R = 0.5 * second + torch.sum(r64.drift(case["drift_kind"], vec, xs) * g[:, :d], 1) + h_pde(case["h_kind"], case["h_par"], xs, V)
    if case["parabolic"]:
        R = R + g[:, d]
    return V, g, second, R


def parts(case, dtype=torch.float64):
    return tuple(v.detach() for v in terms(case, None, dtype, create_graph=False))


def weighted_grads(case, rbars, dtype=torch.float64):
    """[d(sum_k rbar_k R_k)/dtheta for rbar in rbars], flat in registration order, in ``dtype``: one residual graph for all."""
    params = [p.to(dtype).clone().requires_grad_(True) for p in case["params"]]
    R = terms(case, params, dtype)[3]
    return [r64.flat_grad(torch.autograd.grad(torch.sum(rbar.to(dtype) * R), params, allow_unused=True, retain_graph=True), params)
            for rbar in rbars]


def trace_form(case, B, dtype=torch.float64):
    """1/2 trace(B B^T Hess_x V) per sample with torch.autograd.functional.hessian, as the solvers' composite plan takes it
    (elliptic cases: the net input is x)."""
    assert not case["parabolic"]
    params = [p.to(dtype) for p in case["params"]]
    A = (B @ B.t()).to(dtype)
    out = []
    for x in case["x"].to(dtype):
        hess = torch.autograd.functional.hessian(lambda p: r64.net(params, case["act"], p, case["linear"]).squeeze(), x.unsqueeze(0))
        out.append(0.5 * torch.sum(torch.diagonal(A @ hess.squeeze())))
    return torch.stack(out)


def eigh_factor(B):
    """The plan's own factor of B B^T (plan_pinn_native.direction_table): (rank, d) float64."""
    from util_cases import psp
    return psp.plan_pinn_native.direction_table(B)


def make_case(dirs, **kw):
    """ref64_pinn.make_case plus the direction table, rounded to fp32 (the kernels read fp32)."""
    case = r64.make_case(**kw)
    case["dirs"] = torch.as_tensor(dirs).float().double().reshape(-1, case["d"])
    return case
