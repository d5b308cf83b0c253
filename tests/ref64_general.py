"""Float64 reference of one training iteration of GeneralSolver.train / EllipticSolver.train (reference solver.py:1001-1206, :628-826;
oracle/pathspace_oracle.py general_train / elliptic_train), restated with torch ops in float64 and differentiated by plain autograd
(create_graph=True for grad_x V) -- the judge of the value-net kernels (csrc/gen_kernels.h, csrc/genl_kernels.h) in
tests/test_gpu_general_block_gradients.py, itself checked against the fp32 oracle in tests/test_ref64_general.py.

  coeffs64    the coefficients of every problem kind the native plans take (problems.py general_native_spec), in float64, from the
              fp32 numbers the oracle problem holds (B, kappa_, eta_) and the case's keywords;
  net64       the value net as float64 leaves in the package's flat order, for the dense-concat layout (weights (in, out): relu^2,
              tanh^2, tanh) and DenseNet_tanh's nn.Linear layout (weights (out, in));
  iteration   the iteration on the DRAWS of the fp32 oracle's trace (X0, t0, xi per step, the boundary batch and its times), cast to
              double: diffusion and BSDE loss; unbounded, sphere (Dirichlet / Neumann), box, one-sided box, cut corner, annulus;
              adaptive_forward_process with the detached control; loss_with_stopped; a dense constant sigma; the early break.

The input order is [x, t] (time last); EllipticSolver's net has no time input.  The step sizes are the fp32 values the solvers use
(torch.tensor(delta_t) and its root), T is the fp32 value the kernels compare with, so that the fp32 sides differ from this by
rounding alone.  The state path carries no parameter gradient: the control is detached (the native plans take nothing else)."""
import torch

F64 = torch.float64
E32 = 2.0 ** -23


def _steps(delta_t):
    dt32 = torch.tensor(delta_t)
    return float(dt32), float(torch.sqrt(dt32))


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


HESS = "ExponentialOnBallNonlinearSinHessian"
KINDS = ("DoubleWell_multidim_for_general_solver", "AllenCahn", "HeatEquation", "ExponentialOnSphere", "ExponentialOnBallNonlinear",
         "ExponentialOnBallNonlinearSin", HESS, "ExponentialOnSphereNonlinearParabolic", "Committor", "QuadraticOnBox")


def coeffs64(case, oprob):
    """dict(d, B, drift | None, h(t, x, y, z), f(x), g(x, t) | None) of an oracle problem, float64.  h takes the general solver's
    four arguments for every kind (the elliptic kinds ignore t)."""
    kind, kw, ex, d = oprob.kind, case["problem"]["kwargs"], oprob.extra, oprob.d
    assert kind in KINDS, kind
    r2 = lambda x: (x ** 2).sum(1)
    zero = lambda x: torch.zeros(x.shape[0], dtype=F64)
    quad = lambda t, x, y, z: -0.5 * (z ** 2).sum(1)
    co = dict(d=d, B=oprob.B.to(F64), drift=None, g=None)
    if kind == "DoubleWell_multidim_for_general_solver":
        kappa, eta = ex["kappa_"].to(F64), ex["eta_"].to(F64)
        cost = lambda x: (eta * (x - 1.0) ** 2).sum(1)
        linear = kw.get("modus", "HJB") == "linear"
        co["drift"] = lambda x: -4.0 * kappa * (x * (x ** 2 - 1.0))
        co["h"] = (lambda t, x, y, z: zero(x)) if linear else quad
        co["f"] = (lambda x: torch.exp(-cost(x))) if linear else cost
    elif kind == "AllenCahn":
        co["h"] = lambda t, x, y, z: y - y ** 3
        co["f"] = lambda x: 1.0 / (2.0 + 0.4 * r2(x))
    elif kind == "HeatEquation":
        co["h"], co["f"] = (lambda t, x, y, z: zero(x)), r2
    elif kind == "Committor":
        a = float(ex["boundary_distance_1"])
        co["h"], co["f"] = (lambda t, x, y, z: zero(x)), zero
        co["g"] = lambda x, t=None: (torch.sqrt(r2(x)) > a).to(F64)
    elif kind == "QuadraticOnBox":
        T, parabolic = oprob.T, kw.get("parabolic", True)
        co["h"] = quad if kw.get("quad_h", True) else (lambda t, x, y, z: zero(x))
        co["f"] = r2 if parabolic else zero
        co["g"] = (lambda x, t: r2(x) + (T - t)) if parabolic else (lambda x, t=None: r2(x))
    else:                                                        # the exponential-on-the-ball family
        al = float(kw.get("alpha", 1.0))
        neumann = ex.get("boundary_type") == "Neumann"
        if kind == "ExponentialOnSphereNonlinearParabolic":
            T = oprob.T
            co["h"] = lambda t, x, y, z: (-2 * al * y * (al * 2 * r2(x) + d) - y
                                          + torch.sin(torch.exp(2 * al * r2(x) + 2 * t) - y ** 2))
            co["f"] = lambda x: torch.exp(al * r2(x) + T)
            co["g"] = (lambda x, t: 2 * al * x * torch.exp(al * r2(x) + t).unsqueeze(1)) if neumann else \
                (lambda x, t: torch.exp(al * r2(x) + t))
        else:
            if kind == "ExponentialOnSphere":
                co["h"] = lambda t, x, y, z: -al * y * (al * 4 * r2(x) + 2 * d)
            elif kind == "ExponentialOnBallNonlinear":
                co["h"] = lambda t, x, y, z: -2 * al * y * (al * 2 * r2(x) + d) + torch.exp(2 * al * r2(x)) - y ** 2
            elif kind == "ExponentialOnBallNonlinearSin":
                co["h"] = lambda t, x, y, z: -2 * al * y * (al * 2 * r2(x) + d) + torch.sin(torch.exp(2 * al * r2(x)) - y ** 2)
            else:                                                # the full Hessian: (sum_i x_i)^2 in the linear part
                co["h"] = lambda t, x, y, z: (-2 * al * y * (2 * al * x.sum(1) ** 2 + d)
                                              + torch.sin(torch.exp(2 * al * r2(x)) - y ** 2))
            co["f"] = zero
            co["g"] = (lambda x, t=None: 2 * al * x * torch.exp(al * r2(x)).unsqueeze(1)) if neumann else \
                (lambda x, t=None: torch.exp(al * r2(x)))
    return co


def net64(V):
    """dict(params, act, linear): the parameters as float64 leaves in registration order -- the order of the native plans' flat
    vector -- of an oracle value net (DenseNetOracle: act relu2 / tanh2 / tanh, weights (in, out); DenseNetTanhOracle: nn.Linear)."""
    params = [p.detach().cpu().to(F64).clone().requires_grad_(True) for p in V.parameters()]
    linear = hasattr(V, "layers")
    return dict(params=params, act="tanh" if linear else (getattr(V, "activation", "relu2") or "relu2"), linear=linear)


class _Margin:
    """Smallest relative distance of a relu^2 pre-activation from zero: |z| / (sum_j |a_j W_ji| + |b_i|)."""

    def __init__(self):
        self.relu = float("inf")

    def see(self, a, W, b, z):
        with torch.no_grad():
            s = a.abs() @ W.abs() + b.abs()
            self.relu = min(self.relu, float((z.abs() / s.clamp_min(1e-300)).min()))


def value(net, a, margin=None):
    """V(a) (K,): a = [x, t] (time LAST), or [x] for the elliptic solver."""
    params, act, linear = net["params"], net["act"], net["linear"]
    nl = len(params) // 2
    for i in range(nl):
        W = params[2 * i].t() if linear else params[2 * i]
        z = a @ W + params[2 * i + 1]
        if i == nl - 1:
            return z[:, 0]
        if act == "relu2" and margin is not None:
            margin.see(a, W, params[2 * i + 1], z)
        r = torch.relu(z) if act == "relu2" else torch.tanh(z)
        a = torch.cat([a, r if act == "tanh" else r ** 2], 1)


def _inputs(x, t):
    return x if t is None else torch.cat([x, t.reshape(-1, 1)], 1)


def _rel(q, thr):
    return (q - thr).abs() / max(abs(thr), 1e-300)


def exit_test64(ex, X, X_prop, elliptic):
    """(inside (K,) bool, relative distance (K,) of the tested quantities from their thresholds): new_selection of
    solver.py:1119-1129 / :758-767.  Sphere and annulus test the state BEFORE the move, the boxes the proposal.  The distance of
    the one-sided boxes is the smallest over ALL coordinates -- more than their any / all needs, never less."""
    bnd = ex["boundary"]
    if bnd == "sphere":
        r = torch.sqrt((X ** 2).sum(1))
        return r < ex["boundary_distance"], _rel(r, ex["boundary_distance"])
    if bnd == "two_spheres":
        r = torch.sqrt((X ** 2).sum(1))
        a, c = ex["boundary_distance_1"], ex["boundary_distance_2"]
        return (r > a) & (r < c), torch.minimum(_rel(r, a), _rel(r, c))
    if bnd == "square":
        hi = _rel(X_prop, ex["X_r"]).min(1).values
        if ex["one_boundary"]:
            le = X_prop <= ex["X_r"]
            return (le.all(1) if elliptic else le.any(1)), hi
        return ((X_prop >= ex["X_l"]) & (X_prop <= ex["X_r"])).all(1), torch.minimum(hi, _rel(X_prop, ex["X_l"]).min(1).values)
    if bnd == "square-corner":
        return (X_prop <= ex["X_r"]).any(1), _rel(X_prop, ex["X_r"]).min(1).values
    return torch.ones(X.shape[0], dtype=torch.bool), torch.full((X.shape[0],), float("inf"), dtype=F64)


def _neumann(net, pts, gx, d):
    """mean((grad_x V . x - g . x)^2) at the points pts = [x (, t)] (solver.py:1069-1074, :688-693)."""
    pts = pts.detach().clone().requires_grad_(True)
    gV, = torch.autograd.grad(value(net, pts).sum(), pts, create_graph=True)
    return ((gV[:, :d] * pts[:, :d]).sum(1) - (gx * pts[:, :d]).sum(1)).pow(2).mean()


def flat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def _grad(loss, params):
    if not torch.is_tensor(loss) or not loss.requires_grad:
        return torch.zeros(sum(p.numel() for p in params), dtype=F64)
    gs = torch.autograd.grad(loss, params, allow_unused=True, retain_graph=True)
    return flat([g if g is not None else torch.zeros_like(p) for g, p in zip(gs, params)])


def iteration(case, oprob, net, draws, tangent=True):
    """One iteration of the case (the layout of the golden cases: family, problem, solver) on the net `net64` returned and the
    draws of the fp32 oracle's trace.  Returns dict(loss, grad, grad_domain, grad_boundary (flat; domain = the terms the kernels
    differentiate, boundary = the K_boundary-sized terms and the BSDE loss's Neumann residual, which the plans leave to torch
    autograd), YN, VN, XN, tN, steps (active steps per trajectory), K_count, n_loop, tile_steps, margins = dict(exit, time, relu))."""
    s, ex, d = case["solver"], oprob.extra, oprob.d
    elliptic = case["family"] == "elliptic"
    assert not s.get("sample_center", False) and not s.get("uniform_square", False)
    co = coeffs64(case, oprob)
    B, params = co["B"], net["params"]
    dt, sq = _steps(s["delta_t"])
    N, Kb, alpha = s["N"], s["K_boundary"], s["alpha"]
    adaptive, diffusion = s.get("adaptive_forward_process", False), s["loss_method"] == "diffusion"
    bounded = "unbounded" not in ex["boundary"]
    btype = s.get("boundary_type", "Dirichlet") if elliptic else ex.get("boundary_type")
    T = None if elliptic else _f32(oprob.T)
    mg = _Margin()
    X = draws["X0"].to(F64)
    K = X.shape[0]
    t = None if elliptic else draws["t0"].to(F64).reshape(K)
    zeros = torch.zeros(K, dtype=F64)
    # ---- the K_boundary-sized terms
    loss_b = 0.0
    Xb = draws["X_boundary"].to(F64) if bounded else None
    tb = draws["t_b"].to(F64).reshape(-1) if bounded and not elliptic else None
    if diffusion:
        if not elliptic:
            loss_b = loss_b + alpha[1] * (value(net, _inputs(X[:Kb], torch.full((Kb,), T, dtype=F64)), mg) - co["f"](X[:Kb])).pow(2).mean()
        if bounded:
            a_b = alpha[1] if elliptic else alpha[2]
            if btype == "Dirichlet":
                loss_b = loss_b + a_b * (value(net, _inputs(Xb, tb), mg) - co["g"](Xb, tb)).pow(2).mean()
            else:
                loss_b = loss_b + a_b * _neumann(net, _inputs(Xb, tb), co["g"](Xb, tb), d)
    # ---- the rollout
    Y = value(net, _inputs(X, t), mg)
    stopped = torch.zeros(K, dtype=torch.bool)
    steps = torch.zeros(K, dtype=torch.int64)
    m_exit, m_time, n_loop, gV = float("inf"), float("inf"), 0, None
    for n in range(N):
        if not bool((~stopped).any()):                           # solver.py:1093-1097 / :742-744
            break
        assert n < len(draws["xi"]), "the float64 replay runs longer than the oracle's loop: a discrete decision differs"
        x = X.clone().requires_grad_(True)
        Vn = value(net, _inputs(x, t), mg)
        gV, = torch.autograd.grad(Vn.sum(), x, create_graph=True)
        Z = (gV if tangent else gV.detach()) @ B                 # sigma^T grad_x V, row form
        xi = draws["xi"][n].to(F64)
        c = -Z.detach() if adaptive else torch.zeros(K, d, dtype=F64)
        alive = (~stopped).to(F64).unsqueeze(1)
        drift = co["drift"](X) if co["drift"] is not None else 0.0
        X_prop = X + ((drift + c @ B.t()) * dt + (xi @ B.t()) * sq) * alive
        new_sel, dist = exit_test64(ex, X, X_prop, elliptic)
        if bool((~stopped).any()):
            m_exit = min(m_exit, float(dist[~stopped].min()))
        if not elliptic:
            new_sel = new_sel & ((t + dt) <= T)
            m_time = min(m_time, float(_rel(t + dt, T)[~stopped].min()))
        act = new_sel & ~stopped
        actf = act.to(F64)
        Y = Y + ((-co["h"](n * dt, X, Vn, Z) + (Z * c).sum(1)) * dt + (Z * xi).sum(1) * sq) * actf
        X = torch.where(act.unsqueeze(1), X_prop, X).detach()
        if not elliptic:
            t = t + dt * actf
        steps += act.long()
        stopped = stopped | ~new_sel
        n_loop = n + 1
    VN = value(net, _inputs(X, t), mg)
    loss_d = 0.0
    if diffusion:
        loss_d = loss_d + alpha[0] * (VN - Y).pow(2).mean()
    elif elliptic:
        loss_d = loss_d + (co["g"](X) - Y).pow(2).mean()
    elif not bounded:
        loss_d = loss_d + (Y - co["f"](X)).pow(2).mean()
    elif btype == "Dirichlet":
        loss_d = loss_d + (Y - co["g"](X, t)).pow(2).mean()
    else:                                                        # BSDE with a Neumann boundary, solver.py:1177-1183
        late = t > (T - dt)
        m_time = min(m_time, float(_rel(t + dt, T).min()))
        if bool(late.any()):
            loss_d = loss_d + (Y[late] - co["f"](X[late])).pow(2).mean()
        if int(late.sum()) < K:                                  # grad_x V of the LAST executed step against the final X
            loss_b = loss_b + ((gV * X).sum(1) - (co["g"](X, t) * X).sum(1)).pow(2).mean()
    if s.get("loss_with_stopped", False):
        target = co["g"](X) if elliptic else co["f"](X)
        loss_d = loss_d + (Y[stopped] - target[stopped]).pow(2).mean()
    g_d, g_b = _grad(loss_d, params), _grad(loss_b, params)
    tile = steps.clone()
    pad = (-K) % 16
    tile = torch.cat([tile, torch.full((pad,), -1, dtype=torch.int64)]).view(-1, 16).max(1).values
    return dict(loss=float((loss_d + loss_b).detach()), grad=g_d + g_b, grad_domain=g_d, grad_boundary=g_b, YN=Y.detach(), VN=VN.detach(),
                XN=X, tN=(steps.to(F64) * dt if elliptic else t), steps=steps, K_count=int(steps.sum()), n_loop=n_loop,
                tile_steps=torch.clamp(tile + 1, max=N), margins=dict(exit=m_exit, time=m_time, relu=mg.relu))
