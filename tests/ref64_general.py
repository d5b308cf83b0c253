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

from ref64 import product

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


# ---- the kernels' own sweeps of the two-hidden-layer relu^2 net, for the bf16 modes ----------------------------------------------------
def _relu2_parts(net, DI):
    assert net["act"] == "relu2" and not net["linear"] and len(net["params"]) == 6, "the templated kernels' net: DenseNet [H, H], relu^2"
    W1, b1, W2, b2, W3, b3 = net["params"]
    H = W1.shape[1]
    assert W1.shape == (DI, H) and W2.shape == (DI + H, H) and W3.shape == (DI + 2 * H, 1)
    w3 = W3[:, 0]
    return W1, b1, W2[:DI], W2[DI:], b2, w3[:DI], w3[DI:DI + H], w3[DI + H:], b3[0]


def up_sweep(net, a, operands):
    """(V (K,), r1, r2 = relu(z1), relu(z2)) as net_value of gen_fwd_kernel forms them: the three products through `product` (weights
    are stored (in, out): a W = product(a, W^T)), the output layer as fp32 dot products (dot4: exact here)."""
    W1, b1, W2x, W2h, b2, w3x, w3h1, w3h2, b3 = _relu2_parts(net, a.shape[1])
    r1 = torch.relu(product(a, W1.t(), operands) + b1)
    h1 = r1 ** 2
    r2 = torch.relu(product(a, W2x.t(), operands) + product(h1, W2h.t(), operands) + b2)
    return a @ w3x + h1 @ w3h1 + (r2 ** 2) @ w3h2 + b3, r1, r2


def reverse_sweep(net, r1, r2, operands):
    """grad_a V (K, DI) by the kernel's reverse sweep over the stored relu(z1), relu(z2): g_z2 = w3h2 2 r2, g_z1 = (w3h1 + W2h g_z2) 2 r1,
    g_a = w3x + W2x g_z2 + W1 g_z1 -- three more products."""
    W1, b1, W2x, W2h, b2, w3x, w3h1, w3h2, b3 = _relu2_parts(net, net["params"][0].shape[0])
    gz2 = w3h2 * (2.0 * r2)
    gz1 = (w3h1 + product(gz2, W2h, operands)) * (2.0 * r1)
    return w3x + product(gz2, W2x, operands) + product(gz1, W1, operands)


def tangent_images(net, r1, r2, U, operands):
    """(z1^, z2^) (K, H): the tangent pre-activations gen_fwd_kernel stores, z1^ = W1^T U and z2^ = W2x^T U + W2h^T (2 r1 z1^)."""
    W1, b1, W2x, W2h, b2, w3x, w3h1, w3h2, b3 = _relu2_parts(net, U.shape[1])
    z1t = product(U, W1.t(), operands)
    return z1t, product(U, W2x.t(), operands) + product((2.0 * r1) * z1t, W2h.t(), operands)


def tangent_sweep(net, r1, r2, U, operands):
    """U . grad_a V (K,) in forward mode, as the kernel forms the images its backward differentiates, and the output layer's dot
    products."""
    W1, b1, W2x, W2h, b2, w3x, w3h1, w3h2, b3 = _relu2_parts(net, U.shape[1])
    z1t, z2t = tangent_images(net, r1, r2, U, operands)
    return U @ w3x + ((2.0 * r1) * z1t) @ w3h1 + ((2.0 * r2) * z2t) @ w3h2


def kernel_backward(net, samples, wY, wV, rounded):
    """The flat gradient gen_bwd2_kernel forms from the path store: grad_theta sum_samples [a V + w U . grad_x V] over the sample blocks
    (step n < N: a = wY (dY / dV_n), w = wY; the end point: a = wV, no tangent), statement by statement as in its header comment.
    samples: per step dict(a0 (K, DI) = [x, t], U, r1, r2, z1t, z2t, coef = dY / dV_n; fin) of detached tensors.

    rounded=True is gen_bwd2_kernel<D, H, /*BF16*/true> (mlp_dtype='bf16'), whose rounding points are: the stored images, which
    pk_bf16 rounds in the forward kernel before the backward uses them anywhere -- X, U, 2 r1, 2 r2, z1^, z2^; both operands of the
    adjoint products on the bf16 table gW2hr (`gen_gemm<1, ..>(gz1t, lds + G::gW2hr, gz2t, ..)` and `(gz1, .., gz2, ..)`); both
    operands of the outer products (`pack2`: the row items x, w U, h1 = (d1 / 2)^2, h1' = d1 w z1^ and the adjoint panels gz2,
    gz2', gz1, gz1' read back from the exchange tiles).  The bias sums and the rows of dW3 are fp32 sums of unrounded registers.
    rounded=False is the fp32 kernel, i.e. the autograd gradient to float64 rounding (tests/test_ref64_general_bf16.py)."""
    R = (lambda v: v.to(torch.bfloat16).to(v.dtype)) if rounded else (lambda v: v)
    W1, b1, W2x, W2h, b2, w3x, w3h1, w3h2, b3 = [p.detach() for p in _relu2_parts(net, net["params"][0].shape[0])]
    DI, H = W1.shape
    gW1, gW2x, gW2h = torch.zeros_like(W1), torch.zeros_like(W2x), torch.zeros_like(W2h)
    gb1, gb2, gb3 = torch.zeros_like(b1), torch.zeros_like(b2), torch.zeros((), dtype=F64)
    gw3x, gw3h1, gw3h2 = torch.zeros_like(w3x), torch.zeros_like(w3h1), torch.zeros_like(w3h2)
    step2 = lambda dd: 2.0 * (dd > 0).to(F64)
    adj = lambda g, W: R(g) @ R(W).t()                           # W g over the output side, both operands of the MFMA rounded
    outer = lambda A, G: R(A).t() @ R(G)
    for sm in samples:
        X_, d1, d2 = R(sm["a0"]), R(2.0 * sm["r1"]), R(2.0 * sm["r2"])
        if sm["fin"]:
            w, av = torch.zeros_like(wY), wV
            U_, z1_, z2_ = torch.zeros_like(X_), torch.zeros_like(d1), torch.zeros_like(d2)
        else:
            w, av = wY, wY * sm["coef"]
            U_, z1_, z2_ = R(sm["U"]), R(sm["z1t"]), R(sm["z2t"])
        w, av = w.unsqueeze(1), av.unsqueeze(1)
        z2w = w * z2_
        gz2t = w3h2 * d2
        gz2 = av * gz2t + w3h2 * step2(d2) * z2w
        gw3h2 += (av * (0.25 * d2 * d2) + d2 * z2w).sum(0)
        gb3 += av.sum()
        gh1t = w3h1 + adj(gz2t, W2h)
        gh1 = av * w3h1 + adj(gz2, W2h)
        z1w = w * z1_
        gz1 = gh1 * d1 + gh1t * step2(d1) * z1w
        gz1t = gh1t * d1
        A0x, A1x, A0h, A1h = X_, w * U_, 0.25 * d1 * d1, d1 * z1w
        gw3x += (av * A0x + A1x).sum(0)
        gw3h1 += (av * A0h + A1h).sum(0)
        gb2 += gz2.sum(0)
        gb1 += gz1.sum(0)
        gW2x += outer(A0x, gz2) + outer(A1x, gz2t)
        gW1 += outer(A0x, gz1) + outer(A1x, gz1t)
        gW2h += outer(A0h, gz2) + outer(A1h, gz2t)
    return flat([gW1, gb1, torch.cat([gW2x, gW2h], 0), gb2, torch.cat([gw3x, gw3h1, gw3h2]), gb3.reshape(1)])


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


def iteration(case, oprob, net, draws, tangent=True, operands="fp32", sweeps=None, dtype=None, backward="autograd"):
    """One iteration of the case (the layout of the golden cases: family, problem, solver) on the net `net64` returned and the
    draws of the fp32 oracle's trace.

    operands='bf16': the model of GeneralSolver(mlp_dtype='bf16_fwd') on the templated kernels (csrc/gen_kernels.h, MODE 1: gen_stage
    -> stage_aop_bf16 rounds every weight table, gen_gemm -> gemm_Tb rounds the register operand; both round to nearest even).  The
    rollout then runs on the kernels' own three sweeps (`sweeps`, on by default with bf16 operands) instead of autograd:
      up sweep       net_value: z1 = W1^T [x, t], z2 = W2x^T [x, t] + W2h^T h1 -- operands [x, t] (the TIME input sits in the state
                     panel, put_time, and is rounded with it), h1 = relu(z1)^2 and the tables oW1f, oW2xf, oW2hf; at every step, at
                     (X_0, t_0) for Y_0 and at (X_N, t_N) for V_N.  The output layer is fp32 (dot4) and exact here;
      reverse sweep  g_h1 = w3h1 + W2h g_z2, g_x = w3x + W2x g_z2 + W1 g_z1 (`gen_gemm<MODE, ..>(gz1, lds + oW2hr, gz2, ..)`, `(gx, lds +
                     oW2xr, gz2, ..)`, `(gx, lds + oW1r, gz1, ..)`): operands g_z2 = w3h2 2 r2, g_z1 = g_h1 2 r1 and the tables oW2hr,
                     oW2xr, oW1r.  Its result is the VALUE of Z = sigma^T grad_x V in the Y update, the adaptive shift and U;
      tangent sweep  z1^ = W1^T U, z2^ = W2x^T U + W2h^T (2 r1 z1^) (`gen_gemm<MODE, ..>(z1h, lds + oW1f, U, ..)`, `(z2h, lds + oW2xf, U,
                     ..)`, `(z2h, lds + oW2hf, h1d, ..)`): operands U = act sigma ((-h_z + c) dt + xi sqrt(dt)), h1' and the forward
                     tables again.  gen_bwd2_kernel differentiates U . grad_x V through THESE stored images (X, U, 2 r1, 2 r2, z1^,
                     z2^, all fp32 in this mode) with fp32 products on the unrounded weights, which is what autograd does to the
                     tangent sweep when `product` returns the unrounded adjoints.  So Z enters Y by the reverse sweep's value and
                     by the tangent sweep's gradient; with exact products the two are one function and this is the plain reference.
    The boundary terms and the Neumann residual are torch's, in fp32 on the device: exact here.  sweeps=True with operands='fp32'
    runs the same statements unrounded (tests/test_ref64_general_bf16.py: equal to the autograd form to float64 rounding);
    dtype=torch.float32 runs the whole iteration in fp32 -- with bf16 operands the torch stand-in of the kernels.
    backward='fp32' | 'bf16' (with the sweeps): the domain gradient by `kernel_backward` on the recorded sample blocks instead of
    autograd -- 'bf16' is the model of the full mlp_dtype='bf16', whose forward is the 'bf16_fwd' one.

    Returns dict(loss, grad, grad_domain, grad_boundary (flat; domain = the terms the kernels
    differentiate, boundary = the K_boundary-sized terms and the BSDE loss's Neumann residual, which the plans leave to torch
    autograd), YN, VN, XN, tN, steps (active steps per trajectory), K_count, n_loop, tile_steps, margins = dict(exit, time, relu))."""
    global F64
    if dtype is not None and dtype != F64:                       # every statement of this module computes in F64
        keep, F64 = F64, dtype
        try:
            cast = dict(net, params=[p.detach().to(dtype).requires_grad_(True) for p in net["params"]])
            return iteration(case, oprob, cast, draws, tangent, operands, sweeps, None, backward)
        finally:
            F64 = keep
    assert operands in ("fp32", "bf16")
    sweeps = (operands == "bf16") if sweeps is None else sweeps
    assert sweeps or operands == "fp32"
    assert backward in ("autograd", "fp32", "bf16") and (backward == "autograd" or (sweeps and tangent))
    samples = []
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
    Y = up_sweep(net, _inputs(X, t), operands)[0] if sweeps else value(net, _inputs(X, t), mg)
    stopped = torch.zeros(K, dtype=torch.bool)
    steps = torch.zeros(K, dtype=torch.int64)
    m_exit, m_time, n_loop, gV = float("inf"), float("inf"), 0, None
    for n in range(N):
        if not bool((~stopped).any()):                           # solver.py:1093-1097 / :742-744
            break
        assert n < len(draws["xi"]), "the float64 replay runs longer than the oracle's loop: a discrete decision differs"
        xi = draws["xi"][n].to(F64)
        if sweeps:
            Vn, r1, r2 = up_sweep(net, _inputs(X, t), operands)
            with torch.no_grad():
                gV = reverse_sweep(net, r1, r2, operands)[:, :d]
            Z = gV @ B                                           # the value; its gradient comes in by the tangent sweep below
        else:
            x = X.clone().requires_grad_(True)
            Vn = value(net, _inputs(x, t), mg)
            gV, = torch.autograd.grad(Vn.sum(), x, create_graph=True)
            Z = (gV if tangent else gV.detach()) @ B             # sigma^T grad_x V, row form
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
        incr = lambda V_, Z_: (-co["h"](n * dt, X, V_, Z_) + (Z_ * c).sum(1)) * dt + (Z_ * xi).sum(1) * sq
        Y = Y + incr(Vn, Z) * actf
        if sweeps and tangent:
            Zd = Z.clone().requires_grad_(True)
            u, = torch.autograd.grad(incr(Vn.detach(), Zd).sum(), Zd)            # (-h_z + c) dt + xi sqrt(dt), per trajectory
            U = torch.cat([(u @ B.t()) * actf.unsqueeze(1), torch.zeros(K, 0 if elliptic else 1, dtype=F64)], 1)
            Tn = tangent_sweep(net, r1, r2, U, operands)
            Y = Y + (Tn - Tn.detach())
            if backward != "autograd":
                Vd = Vn.detach().clone().requires_grad_(True)
                out = (incr(Vd, Z) * actf).sum()                # (an h that does not read y: no dependence, coefficient 0)
                coef = torch.autograd.grad(out, Vd)[0] if out.requires_grad else torch.zeros(K, dtype=F64)
                with torch.no_grad():
                    z1t, z2t = tangent_images(net, r1, r2, U, operands)
                samples.append(dict(a0=_inputs(X, t), U=U, r1=r1.detach(), r2=r2.detach(), z1t=z1t, z2t=z2t,
                                    coef=coef + (1.0 if n == 0 else 0.0), fin=False))
        X = torch.where(act.unsqueeze(1), X_prop, X).detach()
        if not elliptic:
            t = t + dt * actf
        steps += act.long()
        stopped = stopped | ~new_sel
        n_loop = n + 1
    if sweeps:
        VN, r1, r2 = up_sweep(net, _inputs(X, t), operands)
        samples.append(dict(a0=_inputs(X, t), r1=r1.detach(), r2=r2.detach(), fin=True))
    else:
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
        assert not sweeps, "the BSDE-Neumann residual is torch's (fp32 autograd on the device), not the kernels' sweep"
        if int(late.sum()) < K:                                  # grad_x V of the LAST executed step against the final X
            loss_b = loss_b + ((gV * X).sum(1) - (co["g"](X, t) * X).sum(1)).pow(2).mean()
    if s.get("loss_with_stopped", False):
        target = co["g"](X) if elliptic else co["f"](X)
        loss_d = loss_d + (Y[stopped] - target[stopped]).pow(2).mean()
    if backward == "autograd":
        g_d = _grad(loss_d, params)
    else:                                                        # the weights psp_gen_rollout_bwd2 is handed: dL / dY_N, dL / dV_N
        wY, wV = torch.autograd.grad(loss_d, [Y, VN], allow_unused=True, retain_graph=True)
        zero = torch.zeros(K, dtype=F64)
        g_d = kernel_backward(net, samples, zero if wY is None else wY, zero if wV is None else wV, backward == "bf16")
    g_b = _grad(loss_b, params)
    tile = steps.clone()
    pad = (-K) % 16
    tile = torch.cat([tile, torch.full((pad,), -1, dtype=torch.int64)]).view(-1, 16).max(1).values
    return dict(loss=float((loss_d + loss_b).detach()), grad=g_d + g_b, grad_domain=g_d, grad_boundary=g_b, YN=Y.detach(), VN=VN.detach(),
                XN=X, tN=(steps.to(F64) * dt if elliptic else t), steps=steps, K_count=int(steps.sum()), n_loop=n_loop,
                tile_steps=torch.clamp(tile + 1, max=N), margins=dict(exit=m_exit, time=m_time, relu=mg.relu))
