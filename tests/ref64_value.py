"""Float64 references for Solver(approx_method='value_function') with the state path ATTACHED (adaptive_forward_process=True,
detach_forward=False; reference solver.py:326-339, 438-440, 449-478):

  autograd_iteration   one training iteration restated in float64 and differentiated by plain autograd (create_graph=True), the
                       judge of everything else;
  sweep_iteration      the same gradient by the adjoint recursion the native sweep kernel runs (csrc/genl_adj_kernels.h), written
                       with torch ops: forward with detached states, the weights mu, the reverse recursion for the state adjoint
                       lambda, the rewritten tangent directions U_n and coefficients a_n, and per sample the parameter gradient of
                       a_n V(X_n, n) + grad_x V(X_n, n) . U_n at fixed X_n.

Both take the coefficients of an oracle problem in float64 (coeffs64), a dense-concat value net as a list of float64 parameters
(net64) and the reference-order noise xi (K, d, N + 1), slot n = xi[:, :, n + 1].  The step size is the fp32 value the solver
uses (torch.tensor(delta_t)), so that the fp32 oracle differs from these by rounding alone."""
import torch

F64 = torch.float64


def coeffs64(oprob):
    """dict(B, A | None, kappa | None, p | None, g, x0) of an oracle problem of kind LLGC, LQGC or DoubleWell_multidim."""
    ex, d = oprob.extra, oprob.d
    co = dict(d=d, B=oprob.B.to(F64), A=None, kappa=None, p=None, x0=oprob.X_0.to(F64))
    if oprob.kind == "LLGC":
        alpha = ex["alpha"].to(F64)
        co["A"] = ex["A"].to(F64)
        co["g"] = lambda x: (x @ alpha)[:, 0]
    elif oprob.kind == "LQGC":
        R, P = ex["R"].to(F64), ex["P"].to(F64)
        assert torch.equal(P, torch.diag(torch.diagonal(P)))
        co["A"], co["p"] = ex["A"].to(F64), torch.diagonal(P).clone()
        co["g"] = lambda x: ((x @ R.t()) * x).sum(1)
    elif oprob.kind == "DoubleWell_multidim":
        eta, co["kappa"] = ex["eta_"].to(F64), ex["kappa_"].to(F64)
        co["g"] = lambda x: (eta * (x - 1.0) ** 2).sum(1)
    else:
        raise ValueError(oprob.kind)
    return co


def net64(net, scale=1.0):
    """(parameters as float64 leaves in registration order W_1, b_1, .., W_out, b_out, activation) of a dense-concat value net
    (weights (in, out): the oracle's DenseNetOracle, the package's DenseNet)."""
    params = [(scale * p.detach().cpu().to(F64)).clone().requires_grad_(True) for p in net.parameters()]
    act = getattr(net, "activation", "relu2") or "relu2"
    return params, act


def value(params, act, x, n):
    """V([n, x]): the time input comes first and is the STEP INDEX (solver.py:336-339, 439)."""
    a = torch.cat([torch.full((x.shape[0], 1), float(n), dtype=F64), x], 1)
    nl = len(params) // 2
    for i in range(nl):
        z = a @ params[2 * i] + params[2 * i + 1]
        if i == nl - 1:
            return z[:, 0]
        r = torch.tanh(z) if act in ("tanh", "tanh2") else torch.relu(z)
        a = torch.cat([a, r if act == "tanh" else r ** 2], 1)


def _drift(co, x):
    if co["A"] is not None:
        return x @ co["A"].t()
    return -4.0 * co["kappa"] * (x * (x ** 2 - 1.0))


def _runcost(co, x):
    return (co["p"] * x * x).sum(1) if co["p"] is not None else torch.zeros(x.shape[0], dtype=F64)


def _steps(delta_t):
    dt32 = torch.tensor(delta_t)
    return float(dt32), float(torch.sqrt(dt32))


def _loss_and_weights(D, add, K, loss_method):
    if loss_method == "moment":
        return (D ** 2).mean() + add.mean(), (2.0 / K) * D
    assert loss_method == "log-variance", loss_method
    return (D ** 2).mean() - D.mean() ** 2 + add.mean(), (2.0 / K) * (D - D.mean())


def flat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def autograd_iteration(co, params, act, xi, delta_t, N, loss_method):
    """One iteration by autograd.  Returns dict(loss, grad (flat), dX0 (K, d) = dLoss / dX_0 per trajectory)."""
    dt, sq = _steps(delta_t)
    K, B = xi.shape[0], co["B"]
    xi = xi.to(F64)
    X0 = co["x0"].repeat(K, 1).clone().requires_grad_(True)
    X, Y = X0, value(params, act, X0, 0)
    add = torch.zeros(K, dtype=F64)
    for n in range(N):
        Vn = value(params, act, X, n)
        if n > 0:
            add = add + (Vn - Y) ** 2
        g, = torch.autograd.grad(Vn.sum(), X, create_graph=True)
        Z = g @ B.t()                                                # Z_k = B grad_x V (solver.py:330)
        c = -Z
        w = xi[:, :, n + 1]
        X = X + (_drift(co, X) + c @ B.t()) * dt + (w @ B.t()) * sq
        Y = Y + (0.5 * (Z ** 2).sum(1) + _runcost(co, X) + (Z * c).sum(1)) * dt + (Z * w).sum(1) * sq
    D = Y - co["g"](X)
    loss, _ = _loss_and_weights(D, add, K, loss_method)
    grads = torch.autograd.grad(loss, [X0] + list(params))
    return dict(loss=float(loss.detach()), grad=flat(grads[1:]), dX0=grads[0])


def sweep_iteration(co, params, act, xi, delta_t, N, loss_method):
    """The same iteration by the adjoint recursion of the native sweep (Z = B g orientation).  Returns dict(loss, grad (flat),
    dX0 (K, d), U (N, K, d) rewritten directions, a (N + 1, K) coefficients, lam (N + 1, K, d) state adjoints (lam[n] = adjoint of
    X_n), mu (N + 1, K), X (N + 1, K, d))."""
    dt, sq = _steps(delta_t)
    K, d, B = xi.shape[0], co["d"], co["B"]
    xi = xi.to(F64)
    with torch.enable_grad():
        # ---- forward, states detached: X_n, Z_n, the stored direction U_fwd = B^T xi sqrt(dt), V(X_n, n), Y_n
        X = co["x0"].repeat(K, 1).clone()
        Xs, Zs, Uf, Vs, Ys = [X], [], [], [], []
        Y = None
        for n in range(N):
            x = X.clone().requires_grad_(True)
            Vn = value(params, act, x, n)
            g, = torch.autograd.grad(Vn.sum(), x)
            Vn = Vn.detach()
            if n == 0:
                Y = Vn.clone()
            Vs.append(Vn)
            Ys.append(Y)
            Z = g @ B.t()
            w = xi[:, :, n + 1]
            X = X + (_drift(co, X) - Z @ B.t()) * dt + (w @ B.t()) * sq
            Y = Y + (-0.5 * (Z ** 2).sum(1) + _runcost(co, X)) * dt + (Z * w).sum(1) * sq
            Xs.append(X)
            Zs.append(Z)
            Uf.append((w * sq) @ B)
        xN = X.clone().requires_grad_(True)
        gN = co["g"](xN)
        dg, = torch.autograd.grad(gN.sum(), xN)
        D = Y - gN.detach()
        r = [torch.zeros(K, dtype=F64)] + [Vs[n] - Ys[n] for n in range(1, N)]
        add = sum(rn ** 2 for rn in r)
        loss, wD = _loss_and_weights(D, add, K, loss_method)
        # ---- weights: mu_N = w^D, mu_n = mu_{n+1} - (2/K) r_n
        mu = [None] * (N + 1)
        mu[N] = wD
        for n in range(N - 1, 0, -1):
            mu[n] = mu[n + 1] - (2.0 / K) * r[n]
        mu[0] = torch.zeros(K, dtype=F64)
        a = [mu[1]] + [(2.0 / K) * r[n] for n in range(1, N)] + [torch.zeros(K, dtype=F64)]
        lam = -wD[:, None] * dg
        lams = [None] * (N + 1)
        lams[N] = lam
        U = [None] * N
        grad = [torch.zeros_like(p) for p in params]
        for n in range(N - 1, -1, -1):
            m = mu[n + 1][:, None]
            Lam = lam
            if co["p"] is not None:
                Lam = Lam + m * dt * (2.0 * co["p"] * Xs[n + 1])     # f sits in Y_{n+1} at the MOVED state
            U[n] = m * Uf[n] - dt * ((m * Zs[n] + Lam @ B) @ B)      # B^T v = v @ B in row form
            x = Xs[n].clone().requires_grad_(True)
            Vn = value(params, act, x, n)
            g, = torch.autograd.grad(Vn.sum(), x, create_graph=True)
            S = (a[n] * Vn).sum() + (g * U[n]).sum()
            gs = torch.autograd.grad(S, [x] + list(params))
            for acc, gp in zip(grad, gs[1:]):
                acc += gp
            if co["A"] is not None:
                Jt = Lam @ co["A"]                                   # A^T Lam
            else:
                Jt = -4.0 * co["kappa"] * (3.0 * Xs[n] ** 2 - 1.0) * Lam
            lam = Lam + dt * Jt + gs[0]
            lams[n] = lam
    return dict(loss=float(loss), grad=flat(grad), dX0=lam, U=torch.stack(U), a=torch.stack(a), lam=torch.stack(lams),
                mu=torch.stack(mu), X=torch.stack(Xs))
