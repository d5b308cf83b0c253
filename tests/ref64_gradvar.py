"""float64 reference of the gradient-variance diagnostic (Solver.get_gradient_variances, reference solver.py:234-281) for DenseNet
controls with time_approx='outer' -- CPU only.  Conventions of ref64.iteration_dense: every input is the fp32 oracle's own number
cast to double, the noise is given, nothing is drawn here.

Pre-activation-gradient form: trajectories are independent and net n is evaluated at one input per trajectory, so ONE backward of
sum_k Y_N[k] with respect to the pre-activations (z1, z2, Z) of step n yields the per-trajectory deltas, and the per-trajectory
gradient of Y_N[k] with respect to the set n is the list of rank-one products
    G_k = [x (x) d1, d1, [x | h1] (x) d2, d2, [x | h1 | h2] (x) d3, d3]      (registration order W1, b1, W2, b2, W3, b3; weights (in, out)).
Everything is streamed per step and per chunk of trajectories: no (N, K, p) tensor exists, and the moments of f are taken in two
passes (mean first, then centred squares), not from raw moments.

    f_k = 2 r_k (G_k - Gg)                                              'moment'
    f_k = 2 (r_k - mean r) ((G_k - Gg) - mean_j (G_j - Gg))             'log-variance'
with r = Y_N - g(X_N) and Gg the gradient of g(X_N[0]) (ROW 0 for every k, the reference's quirk; 0 when the forward process is not
adaptive).  `literal` computes the same from K separate autograd.grad calls per step, as the reference does.
"""
import numpy as np
import torch

import ref64

F64 = torch.float64
CHUNK = 2048


def rollout(prob, cfg, nets, noise, y0=0.0):
    """The forward pass of ref64.iteration_dense ('outer') with the pre-activations of every step kept as graph nodes."""
    assert cfg.time_approx == "outer" and cfg.approx_method == "control" and not cfg.random_X_0
    assert prob.kind in ref64.KINDS
    nets = list(nets)
    d = prob.d
    xi = noise.detach().to(F64)
    K = xi.shape[0]
    N = int(np.floor(prob.T / cfg.delta_t))
    assert xi.shape == (K, d, N + 1) and len(nets) == N
    dt32 = torch.tensor(cfg.delta_t)
    dt, sq = float(dt32), float(torch.sqrt(dt32))
    B = prob.B.to(F64)
    b, f, g = ref64._coefficients(prob)
    sets = [[p.detach().to(F64).clone().requires_grad_(True) for p in net.parameters()] for net in nets]
    X = prob.X_0.to(F64).repeat(K, 1)
    Y = torch.full((K,), float(y0), dtype=F64)
    steps = []
    for n in range(N):
        W1, b1, W2, b2, W3, b3 = sets[n]
        z1 = X @ W1 + b1
        h1 = torch.relu(z1) ** 2
        z2 = torch.cat([X, h1], 1) @ W2 + b2
        h2 = torch.relu(z2) ** 2
        Z = torch.cat([X, h1, h2], 1) @ W3 + b3
        steps.append(dict(x=X.detach(), h1=h1.detach(), h2=h2.detach(), z1=z1, z2=z2, Z=Z))
        c = -Z if cfg.adaptive_forward_process else torch.zeros_like(Z)
        if cfg.detach_forward:
            c = c.detach()
        dW = xi[:, :, n + 1]
        X = X + (b(X) + c @ B.t()) * dt + (dW @ B.t()) * sq
        Y = Y + (0.5 * torch.sum(Z ** 2, 1) + f(X) + torch.sum(Z * c, 1)) * dt + torch.sum(Z * dW, 1) * sq
    gX = g(X)
    return dict(sets=sets, steps=steps, Y=Y, gX=gX, K=K, N=N, p=sum(q.numel() for q in sets[0]))


def _deltas(out, ro):
    """Per step (d1, d2, d3): d out[k] / d (z1, z2, Z)[k] for a per-trajectory quantity `out` (K,) -- one backward of its sum."""
    nodes = [t for st in ro["steps"] for t in (st["z1"], st["z2"], st["Z"])]
    if not out.requires_grad:
        return [tuple(torch.zeros_like(t) for t in nodes[3 * n:3 * n + 3]) for n in range(ro["N"])]
    gr = torch.autograd.grad(out.sum(), nodes, retain_graph=True, allow_unused=True)
    gr = [torch.zeros_like(t) if q is None else q.detach() for t, q in zip(nodes, gr)]
    return [tuple(gr[3 * n:3 * n + 3]) for n in range(ro["N"])]


def _rows(st, dl, k0, k1):
    """(k1 - k0, p): the per-trajectory gradients of trajectories k0 .. k1 - 1 with respect to the step's parameter set."""
    x, h1, h2 = st["x"][k0:k1], st["h1"][k0:k1], st["h2"][k0:k1]
    d1, d2, d3 = (t[k0:k1] for t in dl)
    m = k1 - k0
    op = lambda a, dd: (a.unsqueeze(2) * dd.unsqueeze(1)).reshape(m, -1)
    return torch.cat([op(x, d1), d1, op(torch.cat([x, h1], 1), d2), d2, op(torch.cat([x, h1, h2], 1), d3), d3], 1)


def moments(prob, cfg, nets, noise, weights=(), y0=0.0, loss=None):
    """dict(r (K,), Gg (N, p), grads_mean, grads_var (N, p) of `loss` (default cfg.loss_method: 'moment' | 'log-variance'; unbiased
    variance), S, Q: lists over `weights` (each (K,)) of (N, p)  S[c] = sum_k c_k G_k,  Q[c] = sum_k c_k^2 G_k o G_k)."""
    loss = loss or cfg.loss_method
    assert loss in ("moment", "log-variance")
    ro = rollout(prob, cfg, nets, noise, y0)
    K, N, p = ro["K"], ro["N"], ro["p"]
    r = (ro["Y"] - ro["gX"]).detach()
    dY = _deltas(ro["Y"], ro)
    adaptive = bool(cfg.adaptive_forward_process)
    assert not (adaptive and cfg.detach_forward), "g(X_N) does not depend on the parameters: the reference raises here"
    dg = _deltas(ro["gX"][0:1], ro) if adaptive else None              # row 0 only: the deltas of the other rows are zero
    ws = [w.detach().to(F64).cpu() for w in weights]
    Gg = torch.zeros(N, p, dtype=F64)
    mean, var = torch.zeros(N, p, dtype=F64), torch.zeros(N, p, dtype=F64)
    S = [torch.zeros(N, p, dtype=F64) for _ in ws]
    Q = [torch.zeros(N, p, dtype=F64) for _ in ws]
    c = r if loss == "moment" else r - r.mean()
    for n, st in enumerate(ro["steps"]):
        if adaptive:
            Gg[n] = _rows(st, dg[n], 0, 1)[0]
        chunks = [(k0, min(K, k0 + CHUNK)) for k0 in range(0, K, CHUNK)]
        Gbar = torch.zeros(p, dtype=F64)
        for k0, k1 in chunks:
            G = _rows(st, dY[n], k0, k1)
            Gbar += G.sum(0)
            for i, w in enumerate(ws):
                S[i][n] += (w[k0:k1, None] * G).sum(0)
                Q[i][n] += ((w[k0:k1, None] * G) ** 2).sum(0)
        Gbar /= K
        shift = Gg[n] if loss == "moment" else Gbar                     # (log-variance: Gg cancels against its own mean)
        fsum = torch.zeros(p, dtype=F64)
        for k0, k1 in chunks:
            fsum += (2 * c[k0:k1, None] * (_rows(st, dY[n], k0, k1) - shift)).sum(0)
        mean[n] = fsum / K
        sq = torch.zeros(p, dtype=F64)
        for k0, k1 in chunks:
            sq += ((2 * c[k0:k1, None] * (_rows(st, dY[n], k0, k1) - shift) - mean[n]) ** 2).sum(0)
        var[n] = sq / (K - 1)
    return dict(r=r, Gg=Gg, grads_mean=mean, grads_var=var, S=S, Q=Q, N=N, p=p)


def literal(prob, cfg, nets, noise, y0=0.0, loss=None):
    """The literal definition in float64: K separate autograd.grad calls per step, row-0 Gg.  dict(grads_mean, grads_var, Gg)."""
    loss = loss or cfg.loss_method
    ro = rollout(prob, cfg, nets, noise, y0)
    K, N, p = ro["K"], ro["N"], ro["p"]
    r = (ro["Y"] - ro["gX"]).detach().unsqueeze(1)
    mean, var, Ggs = torch.zeros(N, p, dtype=F64), torch.zeros(N, p, dtype=F64), torch.zeros(N, p, dtype=F64)
    for n in range(N):
        theta = ro["sets"][n]
        flat = lambda gs: torch.cat([torch.zeros_like(q).reshape(-1) if g_ is None else g_.reshape(-1) for q, g_ in zip(theta, gs)])
        G = torch.stack([flat(torch.autograd.grad(ro["Y"][k], theta, retain_graph=True, allow_unused=True)) for k in range(K)])
        if cfg.adaptive_forward_process:
            Ggs[n] = flat(torch.autograd.grad(ro["gX"][0], theta, retain_graph=True, allow_unused=True))
        A = G - Ggs[n]
        f = 2 * r * A if loss == "moment" else 2 * (r - r.mean()) * (A - A.mean(0, keepdim=True))
        mean[n], var[n] = f.mean(0), f.var(0)
    return dict(grads_mean=mean, grads_var=var, Gg=Ggs)
