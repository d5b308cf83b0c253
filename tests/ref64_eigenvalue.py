"""Float64 restatement of one iteration of EigenvalueSolver (eigenvalue_solver.py; the reference's `Eigenvalue - *.ipynb` notebooks),
written with torch ops in float64 and differentiated by plain autograd -- the judge of the EIG instances of the value-net forward
kernel (csrc/genl_kernels.h) in tests/test_gpu_eigenvalue_blocks.py, itself compared with the fp32 composite plan in
tests/test_ref64_eigenvalue.py.

  coefficients   b, h, v_true of the two problems in float64 from (kind, d, c);
  value          o (the net's linear output) and V = relu(o) | o, for the dense-concat layout and the nn.Linear layout;
  iteration      the iteration on given draws (X_2 | None, the boundary pair, X_0, xi per step), cast to double: the loss parts, the
                 flat parameter gradient of the domain part (what the kernels differentiate) and of the whole loss, dLoss/dlambda,
                 S_k = sum_n act_n V(X_n) dt, the end points, the discrete results (active steps, K_count, the step count of every
                 16-trajectory tile) and the margins that make them well defined.
The step sizes are the fp32 values the solver uses (torch.tensor(delta_t) and its root); the box is [float32(X_l), float32(X_r)] as
the kernels compare.  ``plant='open_tangent_gate'`` plants the error the per-block test must catch: Z = s grad o where it should
be s 1[o > 0] grad o, with V = relu(o) kept."""
import math

import torch

F64 = torch.float64


def steps(delta_t):
    dt32 = torch.tensor(delta_t)
    return float(dt32), float(torch.sqrt(dt32))


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def coefficients(kind, d, c):
    """dict(b(x), h(x, y), v_true(x)): kind 'fp' (c: (d,) vector) or 'nls' (c: the normalising constant)."""
    if kind == "fp":
        cv = torch.as_tensor(c, dtype=F64).reshape(1, d)
        S = lambda x: (cv * torch.cos(x)).sum(1)                                                 # noqa: E731
        return dict(b=lambda x: -torch.cos(S(x)).unsqueeze(1) * cv * torch.sin(x),
                    h=lambda x, y: y * (-(cv ** 2 * torch.sin(x) ** 2).sum(1) * torch.sin(S(x)) - torch.cos(S(x)) * S(x)),
                    v_true=lambda x: torch.exp(-torch.sin(S(x))))
    assert kind == "nls"
    c = float(c)
    return dict(b=lambda x: torch.zeros_like(x),
                h=lambda x, y: -y ** 3 - y * (-1 / c ** 2 * torch.exp(2 / d * torch.cos(x).sum(1))
                                              + (torch.sin(x) ** 2 / d ** 2 - torch.cos(x) / d).sum(1) - 3),
                v_true=lambda x: 1 / c * torch.exp(1 / d * torch.cos(x).sum(1)))


def net64(params, act, linear, relu):
    """The parameters as float64 leaves, in the flat order of the native plan."""
    return dict(params=[p.detach().cpu().to(F64).clone().requires_grad_(True) for p in params], act=act, linear=linear, relu=relu)


def linear_output(net, a):
    params, act, linear = net["params"], net["act"], net["linear"]
    nl = len(params) // 2
    for i in range(nl):
        W = params[2 * i].t() if linear else params[2 * i]
        z = a @ W + params[2 * i + 1]
        if i == nl - 1:
            return z[:, 0]
        r = torch.relu(z) if act == "relu2" else torch.tanh(z)
        a = torch.cat([a, r if act == "tanh" else r ** 2], 1)


class Gate:
    """Every o the iteration evaluates: the gate margin min |o| and the share of closed gates."""

    def __init__(self):
        self.min_abs, self.n, self.neg = float("inf"), 0, 0

    def see(self, o):
        with torch.no_grad():
            self.min_abs = min(self.min_abs, float(o.abs().min()))
            self.n += o.numel()
            self.neg += int((o < 0).sum())


def value(net, a, gate=None):
    o = linear_output(net, a)
    if gate is not None:
        gate.see(o)
    return torch.relu(o) if net["relu"] else o


def flat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def _grad(loss, params):
    gs = torch.autograd.grad(loss, params, allow_unused=True, retain_graph=True)
    return flat([g if g is not None else torch.zeros_like(p) for g, p in zip(gs, params)])


def hat(x):
    return torch.exp(-200 * x ** 2) * ((x > -0.2) & (x < 0.2))


def iteration(kind, d, c, net, lam, draws, delta_t, N, alpha, X_l=0.0, X_r=2 * math.pi, sigma=math.sqrt(2.0), normalisation=None,
              X_center=None, plant=None):
    """draws: dict(X0 (K, d), xi (N, K, d)[, X2 (K, d), Xb, Xr (Kb, d)]) fp32 tensors.  lam: python float or float64 leaf.
    The boundary / normalisation parts are formed only where their draws are given."""
    co = coefficients(kind, d, c)
    params = net["params"]
    dt, sq = steps(delta_t)
    sig = f32(sigma)
    lo, hi = f32(X_l), f32(X_r)
    lam = lam if torch.is_tensor(lam) else torch.tensor(float(lam), dtype=F64, requires_grad=True)
    gate = Gate()
    X = draws["X0"].to(F64)
    K = X.shape[0]
    parts = {}
    loss_rest = torch.zeros((), dtype=F64)
    if normalisation == "center":
        Xc = X_center.to(F64).reshape(1, d)
        parts["center"] = ((value(net, Xc, gate) - co["v_true"](Xc)) ** 2).mean()
        loss_rest = loss_rest + parts["center"]
    elif normalisation == "l2":
        m = (value(net, draws["X2"].to(F64), gate) ** 2).mean()
        parts["center"] = (m - 1) ** 2
        loss_rest = loss_rest + hat(m) + 0.01 * (m - 1) ** 2
    if "Xb" in draws:
        Xb = draws["Xb"].to(F64).clone().requires_grad_(True)
        Xr = draws["Xr"].to(F64).clone().requires_grad_(True)
        Vb, Vr = value(net, Xb, gate), value(net, Xr, gate)
        gb, = torch.autograd.grad(Vb.sum(), Xb, create_graph=True)
        gr, = torch.autograd.grad(Vr.sum(), Xr, create_graph=True)
        parts["boundary"] = ((Vb - Vr) ** 2).mean()
        parts["derivative_boundary"] = ((gb - gr) ** 2).mean()
        loss_rest = loss_rest + alpha[1] * parts["boundary"] + alpha[1] * parts["derivative_boundary"]
    # ---- the rollout: the state path carries no parameter
    Y = torch.zeros(K, dtype=F64)
    S = torch.zeros(K, dtype=F64)
    stopped = torch.zeros(K, dtype=torch.bool)
    steps_k = torch.zeros(K, dtype=torch.long)
    V_L2 = torch.zeros(K, dtype=F64)
    exit_margin, K_count, n_loop = float("inf"), 0, N
    V0 = None
    for n in range(N):
        if not bool((~stopped).any()):
            n_loop = n
            break
        Xg = X.detach().clone().requires_grad_(True)
        o = linear_output(net, Xg)
        gate.see(o)
        Vn = torch.relu(o) if net["relu"] else o
        if V0 is None:
            V0 = Vn
        src = o if plant == "open_tangent_gate" else Vn
        g, = torch.autograd.grad(src.sum(), Xg, create_graph=True)
        Z = sig * g
        xi = draws["xi"][n].to(F64)
        with torch.no_grad():
            alive = (~stopped).to(F64).unsqueeze(1)
            V_L2 = V_L2 + (~stopped).to(F64) * (Vn.detach() - co["v_true"](X)) ** 2 * dt
            Xp = X + (co["b"](X) * dt + sig * xi * sq) * alive
            inside = ((Xp >= lo) & (Xp <= hi)).all(1)
            dist = torch.minimum((Xp - lo).abs(), (Xp - hi).abs()).min(1).values
            if bool((~stopped).any()):
                exit_margin = min(exit_margin, float(dist[~stopped].min()))
            act = inside & ~stopped
            actf = act.to(F64)
        Y = Y + ((-co["h"](X, Vn) - lam * Vn) * dt + (Z * xi).sum(1) * sq) * actf
        S = S + actf * Vn.detach() * dt
        with torch.no_grad():
            X = torch.where(act.unsqueeze(1), Xp, X)
            steps_k += act.long()
            K_count += int(act.sum())
            stopped = stopped | ~inside
    VN = value(net, X, gate)
    D = VN - V0 - Y
    parts["domain"] = (D ** 2).mean()
    loss_dom = alpha[0] * parts["domain"]
    loss = loss_rest + loss_dom
    grad_domain = _grad(loss_dom, params)
    grad = grad_domain + (_grad(loss_rest, params) if loss_rest.requires_grad else 0.0)
    dlam, = torch.autograd.grad(loss_dom, lam, retain_graph=True, allow_unused=True)
    w = (2.0 * alpha[0] / K) * D.detach()
    nt = (K + 15) // 16
    m = torch.cat([steps_k, torch.zeros(16 * nt - K, dtype=torch.long) - 1]).reshape(nt, 16)    # (padding lanes start stopped)
    tile_steps = torch.clamp(m.max(1).values + 1, max=N)
    return dict(loss=float(loss.detach()), loss_domain=float(loss_dom.detach()), parts={k: float(v.detach()) for k, v in parts.items()}, grad=grad.detach(),
                grad_domain=grad_domain.detach(), dlam=float(dlam) if dlam is not None else 0.0, dlam_scale=float((w * S).abs().sum()),
                S=S.detach(), YN=(V0 + Y).detach(), VN=VN.detach(), XN=X.detach(), D=D.detach(), steps=steps_k, K_count=K_count,
                n_loop=n_loop, tile_steps=tile_steps, V_L2=float(V_L2.mean()),
                margins=dict(exit=exit_margin, gate=gate.min_abs), closed_share=gate.neg / max(1, gate.n),
                stopped_share=float(stopped.double().mean()))
