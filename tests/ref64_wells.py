"""float64 reference of ONE iteration of `Solver` with DenseNet controls on a problem given by its ``native_spec()`` -- CPU only.

tests/ref64.py::iteration_dense restated for the coefficient kinds of the remaining double wells (DoubleWell_OU,
DoubleWell_multidim_2, DoubleWell_multidim_3), which the fp32 oracle does not know: the drift and the terminal cost are closures over
the spec's own fp32 numbers cast to double, the nets are the package's DenseNets (weights (in, out), relu(.)**2, dense-concat), the
step is the fp32 delta_t and its fp32 root.  Nothing is drawn here.

  drift   DRIFT_DOUBLE_WELL   b_i = -4 kappa_i x_i (x_i^2 - 1)
          DRIFT_WELL_DIAG     the same for i < split, b_i = a_i x_i from split on
          DRIFT_RADIAL_WELL   b = -phi(r) x / r,  r = |x|,  phi = 4 kappa (r - r0) ((r - r0)^2 - w)
  term    TERM_SHIFTED_QUAD   g = sum_i eta_i (x_i - 1)^2
          TERM_QUAD_LINEAR    the same for i < split, alpha_i x_i from split on
          TERM_RADIAL_QUAD    g = alpha (r - rho)^2

``jacobian=False`` drops the drift Jacobian from the backward pass (b sees a detached state): the regime check of the GPU cases --
an attached case whose gradient does not move when b' is dropped proves nothing about b'.
"""
import numpy as np
import torch

import ref64
from util_cases import psp

nat = psp.native
F64 = torch.float64


def coefficients(spec, d, jacobian=True):
    kd, dv = spec["drift"]
    kt, tv = spec["term"]
    split = int(spec.get("split", 0))
    dv, tv = dv.detach().cpu().to(F64), tv.detach().cpu().to(F64)
    assert spec["sigma"][0] == nat.SIGMA_IDENTITY and spec["runcost"][0] == nat.RUNCOST_ZERO

    def well(x, kappa):
        return -4.0 * kappa * (x * (x ** 2 - 1.0))

    def b(x):
        x = x if jacobian else x.detach()
        if kd == nat.DRIFT_DOUBLE_WELL:
            return well(x, dv)
        if kd == nat.DRIFT_WELL_DIAG:
            return torch.cat([well(x[:, :split], dv[:split]), dv[split:] * x[:, split:]], 1)
        if kd == nat.DRIFT_RADIAL_WELL:
            r = torch.sqrt(torch.sum(x ** 2, 1, keepdim=True))
            s = r - dv[1]
            return -(4.0 * dv[0] * s * (s ** 2 - dv[2])) * x / r
        raise NotImplementedError(kd)

    def g(x):
        if kt == nat.TERM_SHIFTED_QUAD:
            return torch.sum(tv * (x - 1.0) ** 2, 1)
        if kt == nat.TERM_QUAD_LINEAR:
            return torch.sum(tv[:split] * (x[:, :split] - 1.0) ** 2, 1) + torch.sum(tv[split:] * x[:, split:], 1)
        if kt == nat.TERM_RADIAL_QUAD:
            return tv[0] * (torch.sqrt(torch.sum(x ** 2, 1)) - tv[1]) ** 2
        raise NotImplementedError(kt)

    return b, g


def iteration(spec, X_0, N, delta_t, nets, noise, loss="log-variance", adaptive=True, detach=False, jacobian=True):
    """time_approx='outer': `nets` the N per-step DenseNet(d -> d); noise (K, d, N + 1) as the reference draws it.  Returns
    dict(D, Y, XN, loss, sets=[[dW1, db1, dW2, db2, dW3, db3] per step], grad (flat), Z (N, K, d), X (N + 1, K, d), r (N + 1, K))."""
    d = X_0.numel()
    xi = noise.detach().cpu().to(F64)
    K = xi.shape[0]
    assert xi.shape == (K, d, N + 1) and len(nets) == N
    dt32 = torch.tensor(delta_t)
    dt, sq = float(dt32), float(torch.sqrt(dt32))
    b, g = coefficients(spec, d, jacobian)
    sets = [[p.detach().cpu().to(F64).clone().requires_grad_(True) for p in net.W] for net in nets]

    def net(n, X):
        W1, b1, W2, b2, W3, b3 = sets[n]
        u = torch.cat([X, torch.relu(X @ W1 + b1) ** 2], 1)
        u = torch.cat([u, torch.relu(u @ W2 + b2) ** 2], 1)
        return u @ W3 + b3

    X = X_0.detach().cpu().to(F64).repeat(K, 1)
    Y = torch.zeros(K, dtype=F64)
    Z_sum = torch.zeros(K, dtype=F64)
    Zs, Xs = [], [X.detach().clone()]
    for n in range(N):
        Z = net(n, X)
        c = -Z if adaptive else torch.zeros_like(Z)
        if detach:
            c = c.detach()
        dW = xi[:, :, n + 1]
        X = X + (b(X) + c) * dt + dW * sq
        Y = Y + (0.5 * torch.sum(Z ** 2, 1) + torch.sum(Z * c, 1)) * dt + torch.sum(Z * dW, 1) * sq
        if loss == "relative_entropy":
            Z_sum = Z_sum + 0.5 * torch.sum(Z ** 2, 1) * dt
        Zs.append(Z.detach().clone())
        Xs.append(X.detach().clone())
    gX = g(X)
    D = Y - gX
    L = ref64._loss(loss, D, Y, gX, Z_sum, adaptive)
    flat = [p for s in sets for p in s]
    grads = torch.autograd.grad(L, flat, allow_unused=True)
    grads = [torch.zeros_like(p) if q is None else q.detach() for p, q in zip(flat, grads)]
    D_out = -(Z_sum + gX) if loss == "relative_entropy" else D
    Xs = torch.stack(Xs)
    return dict(D=D_out.detach(), Y=(-Z_sum if loss == "relative_entropy" else Y).detach(), XN=X.detach(), loss=float(L.detach()),
                sets=[grads[6 * i:6 * i + 6] for i in range(N)], grad=torch.cat([q.reshape(-1) for q in grads]),
                Z=torch.stack(Zs), X=Xs, r=torch.sqrt(torch.sum(Xs ** 2, 2)))


def grid_control(ref, X, n):
    """u*(X, t_n) (K, d_pad-wide columns cut to X's) read from plan_common.ul2_reference's kind-2 description with the kernel's
    cell arithmetic (csrc/ugrid.h): fp32 clamp and division, the globally last trajectory lowered by two, numpy wrap-around."""
    X32 = X.detach().cpu().float()
    K, d = X32.shape
    xb, dx, xhi = (torch.tensor(ref[k], dtype=torch.float32) for k in ("xb", "dx", "xhi"))
    cell = torch.floor((torch.clamp(X32, -xb, xhi) + xb) / dx).long()
    last = ref["K_global"] - 1 - ref["k_offset"]
    if 0 <= last < K:
        cell[last] -= 2
    cell = torch.where(cell < 0, cell + ref["ncols"], cell).clamp(0, ref["ncols"] - 1)
    row = int(ref["row"][n])
    grp = ref["group"][:d].long()
    return ref["tables"][grp.unsqueeze(0).expand(K, d), row, cell].to(F64)


def ul2_per_trajectory(ref, out, delta_t):
    """sum_n |-Z_n - u*(X_{n+1}, t_n)|^2 dt per trajectory (solver.py:491-494) from an `iteration` result, in float64."""
    dt = float(torch.tensor(delta_t))
    N = out["Z"].shape[0]
    acc = torch.zeros(out["Z"].shape[1], dtype=F64)
    for n in range(N):
        acc += torch.sum((-out["Z"][n] - grid_control(ref, out["X"][n + 1], n)) ** 2, 1) * dt
    return acc
