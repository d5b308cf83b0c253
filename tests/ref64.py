"""float64 reference of ONE iteration of the control-ansatz `Solver` (rollout, loss, backward) -- CPU only.

`iteration`: the tanh MLP of time_approx='inner'.  `iteration_dense` (below): DenseNet controls, 'outer' and 'inner'.

A plain torch-autograd restatement of oracle.pathspace_oracle.hjb_train (time_approx='inner', approx_method='control') in double
precision.  Every number it starts from is the fp32 oracle's own, cast to double: OracleProblem.B / .X_0 / .extra (A, alpha, P, R,
eta_, kappa_), the TanhMLP parameters, the step size (torch.tensor(delta_t), fp32, and its fp32 square root, as solver.py:39-40
forms them) and the noise tensor (K, d, N + 1).  Nothing is drawn here: a generator yields other numbers in double.

So the result is the exact (to double rounding) answer of the fp32 problem the kernels and the fp32 oracle are given, and the
distance of either from it is that implementation's own arithmetic error.
"""
import numpy as np
import torch

F64 = torch.float64
KINDS = ("LLGC", "LQGC", "DoubleWell_multidim")
LOSSES = ("log-variance", "moment", "variance", "cross_entropy", "relative_entropy")


def _coefficients(prob, dtype=F64):
    """(b, f, g) of the problem kind as double-precision closures over the oracle's fp32 data (pathspace_oracle.problem_*);
    dtype: the one they compute in (float64 but for the fp32 stand-in of `iteration`)."""
    ex = prob.extra
    if prob.kind == "LLGC":
        A, alpha = ex["A"].to(dtype), ex["alpha"].to(dtype)
        return (lambda x: x @ A.t()), (lambda x: torch.zeros(x.shape[0], dtype=dtype)), (lambda x: (x @ alpha)[:, 0])
    if prob.kind == "LQGC":
        A, P, R = ex["A"].to(dtype), ex["P"].to(dtype), ex["R"].to(dtype)
        return (lambda x: x @ A.t()), (lambda x: torch.sum(x * (x @ P.t()), 1)), (lambda x: torch.sum(x * (x @ R.t()), 1))
    if prob.kind == "DoubleWell_multidim":
        eta, kappa = ex["eta_"].to(dtype), ex["kappa_"].to(dtype)
        return ((lambda x: -4.0 * kappa * (x * (x ** 2 - 1.0))), (lambda x: torch.zeros(x.shape[0], dtype=dtype)),
                (lambda x: torch.sum(eta * (x - 1.0) ** 2, 1)))
    raise NotImplementedError(prob.kind)


def _loss(kind, D, Y, gX, Z_sum, adaptive):
    """pathspace_oracle.hjb_loss (solver.py:164-192)."""
    if kind == "moment":
        return D.pow(2).mean()
    if kind == "log-variance":
        return D.pow(2).mean() - D.mean().pow(2)
    if kind == "variance":
        return torch.var(torch.exp(-gX + Y))
    if kind == "cross_entropy":
        return (Y * torch.exp(-gX + (Y.detach() if adaptive else 0.0))).mean()
    if kind == "relative_entropy":
        return (Z_sum + gX).mean()
    raise NotImplementedError(kind)


def rb(x):
    """Round to nearest even onto bf16, back in the dtype of x: what `(__bf16)v` does to an fp32 MFMA operand."""
    return x.to(torch.bfloat16).to(x.dtype)


class _Product(torch.autograd.Function):
    """a (K, n) x W (m, n) -> a W^T (K, m) as the forward-only bf16 modes run it: both operands of the forward product are rounded to
    bf16 (exact sums: the MFMA accumulates in fp32, which float64 stands in for); the backward is the fp32 one of those modes, on the
    UNROUNDED a and W -- NOT the adjoint of the rounded product, which would carry rb(W) (a straight-through rounding op gets
    exactly that wrong)."""

    @staticmethod
    def forward(ctx, a, W, rounded):
        ctx.save_for_backward(a, W)
        return (rb(a) @ rb(W).t()) if rounded else a @ W.t()

    @staticmethod
    def backward(ctx, g):
        a, W = ctx.saved_tensors
        return g @ W, g.t() @ a, None


def product(a, W, operands="fp32"):
    """a W^T with the operand rounding of a matrix mode ('fp32': none, 'bf16': see _Product)."""
    assert operands in ("fp32", "bf16")
    return _Product.apply(a, W, operands == "bf16")


def iteration(prob, cfg, z, noise, weights=None, operands="fp32", dtype=F64, want_path=False):
    """One iteration in float64.

    operands='bf16': the model of Solver(mlp_dtype='bf16'), hjb_fwd_kernel<D, H, MODE = 1> (csrc/hjb_kernels.h).  The rounding
    points, all of them operands of v_mfma_f32_16x16x32_bf16 and all round-to-nearest-even:
      W1x, W2, W3        stage_aop_bf16: `v[e] = (__bf16)src(row, ...)`, once per workgroup;
      X_n, h1, h2        gemm_Tb: `b[e] = (__bf16)in[2 * S][e]`, per step, at the three calls `gemm_Tb<HB, DB>(h1, lds + oW1, X, ..)`,
                         `gemm_Tb<HB, HB>(h2, lds + oW2, h1, ..)` and `gemm_Tb<DB, HB>(Z, lds + oW3, h2, ..)`.
    Everything else is fp32 in the kernel and exact here: the accumulator starts from `vb1 + tn * vw1t` (time column and bias), the
    biases b2, b3, tanh, drift, sigma, the state update, Y, D and the loss.  The backward kernels of this mode (hjb_bwd2 / hjb_adj)
    run in fp32 on the stored fp32 X_n, h1, h2 and the fp32 weights: `product` returns the unrounded adjoints.

    dtype=torch.float32 runs the same statements in fp32: with operands='bf16' a torch stand-in of the bf16 kernels (fp32 arithmetic
    on bf16-rounded operands), which differs from the float64 model by fp32 rounding and by the rare operand that an fp32-sized
    perturbation moves to the other bf16 neighbour (tests/test_ref64_bf16.py).

    prob: OracleProblem; cfg: HJBConfig (time_approx='inner', control ansatz, fixed X_0, no learnable Y_0); z: the fp32 TanhMLP
    (read, never modified); noise: (K, d, N + 1) as hjb_train takes it; weights: optional (K,) -- the loss is then sum_k w_k D_k
    (tests/test_gpu_range_guard._oracle_weighted_gradient).

    Returns dict(D, loss, blocks=[dW1, db1, dW2, db2, dW3, db3], grad (flat, that order), h1, h2 (K, H) at step N // 2, N);
    D is -(Zsum + g(X_N)) for the relative entropy, as the kernels define it (include/psp.h).
    want_path: also Z (N, K, d), the net's output Z_n(X_n, t_n) of every step, and X (N + 1, K, d), the states X_0 .. X_N -- detached,
    in `dtype` (tests/ref64_ul2.py forms the u_L2 log from them).
    """
    assert cfg.time_approx == "inner" and cfg.approx_method == "control" and not cfg.learn_Y_0 and not cfg.random_X_0
    assert prob.kind in KINDS and cfg.loss_method in LOSSES
    d = prob.d
    xi = noise.detach().to(dtype)
    K = xi.shape[0]
    N = int(np.floor(prob.T / cfg.delta_t))                            # solver.py:41
    assert xi.shape == (K, d, N + 1), (tuple(xi.shape), (K, d, N + 1))
    dt32 = torch.tensor(cfg.delta_t)                                   # solver.py:39-40: the fp32 step and its fp32 root
    dt, sq = float(dt32), float(torch.sqrt(dt32))
    B = prob.B.to(dtype)
    b, f, g = _coefficients(prob, dtype)
    W1, b1, W2, b2, W3, b3 = params = [p.detach().to(dtype).clone().requires_grad_(True) for p in z.parameters()]
    assert W1.shape[1] == d + 1 and W3.shape[0] == d

    def net(t, X):                                                     # the input is [t, x]: column 0 of W1 is the time column
        h1 = torch.tanh(t * W1[:, 0] + product(X, W1[:, 1:], operands) + b1)
        h2 = torch.tanh(product(h1, W2, operands) + b2)
        return product(h2, W3, operands) + b3, h1, h2

    X = prob.X_0.to(dtype).repeat(K, 1)
    Y = torch.zeros(K, dtype=dtype)
    Z_sum = torch.zeros(K, dtype=dtype)
    mid = {}
    Zs, Xs = [], [X.detach().clone()]
    for n in range(N):
        Z, h1, h2 = net(n * dt, X)
        if n == N // 2:
            mid = dict(h1=h1.detach().clone(), h2=h2.detach().clone())
        c = -Z if cfg.adaptive_forward_process else torch.zeros_like(Z)
        if cfg.detach_forward:
            c = c.detach()
        dW = xi[:, :, n + 1]
        X = X + (b(X) + c @ B.t()) * dt + (dW @ B.t()) * sq
        fX = f(X)                                                      # h and the running cost see the UPDATED state
        Y = Y + (0.5 * torch.sum(Z ** 2, 1) + fX + torch.sum(Z * c, 1)) * dt + torch.sum(Z * dW, 1) * sq
        if cfg.loss_method == "relative_entropy":
            Z_sum = Z_sum + (0.5 * torch.sum(Z ** 2, 1) + fX) * dt
        if want_path:
            Zs.append(Z.detach().clone())
            Xs.append(X.detach().clone())
    gX = g(X)
    D = Y - gX
    if want_path:
        mid.update(Z=torch.stack(Zs), X=torch.stack(Xs))
    if weights is not None:
        loss = (weights.detach().to(dtype).cpu() * D).sum()
    else:
        loss = _loss(cfg.loss_method, D, Y, gX, Z_sum, cfg.adaptive_forward_process)
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    blocks = [torch.zeros_like(p) if q is None else q.detach() for p, q in zip(params, grads)]
    D_out = -(Z_sum + gX) if cfg.loss_method == "relative_entropy" else D
    return dict(D=D_out.detach(), loss=float(loss.detach()), blocks=blocks, grad=torch.cat([q.reshape(-1) for q in blocks]), N=N, **mid)


def iteration_dense(prob, cfg, nets, noise, weights=None):
    """One iteration in float64 with a DenseNet control (oracle.pathspace_oracle.DenseNetOracle: dense-concat layers, relu(.)**2,
    weights stored (in, out)).

    time_approx='outer': `nets` is the list of the N per-step nets DenseNet(d -> d), net n sees x at step n.  'inner': `nets` is
    one DenseNet(d + 1 -> d) (or a list of one) and sees [t_n, x], where t_n is the fp32 product of the fp32 step index and the fp32
    delta_t, cast to double -- the number control_eval forms (ones * n * dt32) and the one the plan's `tn` table holds
    (plan_dense_native.py: arange(N, fp32) * dt), NOT the double product n * dt.  Adaptive or not, attached or detached, the three
    problem kinds and the five losses of _coefficients / _loss; everything else as `iteration`: the inputs are the fp32 oracle's
    own numbers cast to double, nothing is drawn here, `weights` (K,) makes the loss sum_k w_k D_k.

    Returns dict(D, loss, sets=[[dW1, db1, dW2, db2, dW3, db3] per parameter set], grad (flat, the plan's order [set 0 | set 1 |
    ...]), z1, z2 (K, H): the hidden layers' PRE-activations at step N // 2, N); D is -(Zsum + g(X_N)) for the relative entropy, as
    the kernels define it (include/psp.h).
    """
    assert cfg.time_approx in ("outer", "inner") and cfg.approx_method == "control" and not cfg.learn_Y_0 and not cfg.random_X_0
    assert prob.kind in KINDS and cfg.loss_method in LOSSES
    outer = cfg.time_approx == "outer"
    nets = list(nets) if isinstance(nets, (list, tuple)) else [nets]
    d = prob.d
    xi = noise.detach().to(F64)
    K = xi.shape[0]
    N = int(np.floor(prob.T / cfg.delta_t))
    assert xi.shape == (K, d, N + 1), (tuple(xi.shape), (K, d, N + 1))
    assert len(nets) == (N if outer else 1), (len(nets), N)
    dt32 = torch.tensor(cfg.delta_t)
    dt, sq = float(dt32), float(torch.sqrt(dt32))
    B = prob.B.to(F64)
    b, f, g = _coefficients(prob)
    di = d + (0 if outer else 1)
    sets = [[p.detach().to(F64).clone().requires_grad_(True) for p in net.parameters()] for net in nets]
    for W1, b1, W2, b2, W3, b3 in sets:
        H = W1.shape[1]
        assert W1.shape == (di, H) and W2.shape == (di + H, H) and W3.shape == (di + 2 * H, d), (W1.shape, W2.shape, W3.shape)

    def net(n, X):
        W1, b1, W2, b2, W3, b3 = sets[n if outer else 0]
        u = X
        if not outer:
            t = float(torch.tensor(float(n)) * dt32)                   # fp32 n * dt
            u = torch.cat([torch.full((K, 1), t, dtype=F64), X], 1)
        z1 = u @ W1 + b1
        u = torch.cat([u, torch.relu(z1) ** 2], 1)
        z2 = u @ W2 + b2
        u = torch.cat([u, torch.relu(z2) ** 2], 1)
        return u @ W3 + b3, z1, z2

    X = prob.X_0.to(F64).repeat(K, 1)
    Y = torch.zeros(K, dtype=F64)
    Z_sum = torch.zeros(K, dtype=F64)
    mid = {}
    for n in range(N):
        Z, z1, z2 = net(n, X)
        if n == N // 2:
            mid = dict(z1=z1.detach().clone(), z2=z2.detach().clone())
        c = -Z if cfg.adaptive_forward_process else torch.zeros_like(Z)
        if cfg.detach_forward:
            c = c.detach()
        dW = xi[:, :, n + 1]
        X = X + (b(X) + c @ B.t()) * dt + (dW @ B.t()) * sq
        fX = f(X)                                                      # the running cost sees the UPDATED state
        Y = Y + (0.5 * torch.sum(Z ** 2, 1) + fX + torch.sum(Z * c, 1)) * dt + torch.sum(Z * dW, 1) * sq
        if cfg.loss_method == "relative_entropy":
            Z_sum = Z_sum + (0.5 * torch.sum(Z ** 2, 1) + fX) * dt
    gX = g(X)
    D = Y - gX
    if weights is not None:
        loss = (weights.detach().to(F64).cpu() * D).sum()
    else:
        loss = _loss(cfg.loss_method, D, Y, gX, Z_sum, cfg.adaptive_forward_process)
    flat = [p for s in sets for p in s]
    grads = torch.autograd.grad(loss, flat, allow_unused=True)
    grads = [torch.zeros_like(p) if q is None else q.detach() for p, q in zip(flat, grads)]
    D_out = -(Z_sum + gX) if cfg.loss_method == "relative_entropy" else D
    return dict(D=D_out.detach(), loss=float(loss.detach()), sets=[grads[6 * i:6 * i + 6] for i in range(len(sets))],
                grad=torch.cat([q.reshape(-1) for q in grads]), N=N, **mid)
