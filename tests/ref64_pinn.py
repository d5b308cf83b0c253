"""Float64 (or any dtype) torch-autograd statement of the PINN residual of a dense-concat value net and of the parameter
gradient of its loss -- what the forward-Laplacian kernels (csrc/pinn_kernels.h) are tested against.

    R_k = [dV/dt] + s^2/2 sum_{j<d} d^2 V/dx_j^2 + b(x) . grad_x V + h(x, V, s grad_x V)
    loss = alpha0 mean(R^2)        or        alpha0 var(R)  (unbiased, PINN_log_variance)

Nested autograd, one second derivative per space column, exactly as the solvers' composite plan takes them.  Parameters are the
flat list W_1, b_1, .., W_out, b_out with (in, out) weights, or (out, in) ones with ``linear=True``.
"""
import torch

DRIFT_ZERO, DRIFT_DIAG, DRIFT_DWELL = 0, 2, 3
H_ZERO, H_QUAD, H_ALLEN_CAHN, H_EXP_LIN, H_EXP_SQ, H_EXP_SIN = 0, 1, 2, 3, 4, 5
ACTS = ("relu2", "tanh2", "tanh")


def act_fn(act, z):
    if act == "relu2":
        return torch.relu(z) ** 2
    return torch.tanh(z) ** 2 if act == "tanh2" else torch.tanh(z)


def net(params, act, inp, linear=False, preacts=None):
    n = len(params) // 2
    a = inp
    for i in range(n):
        W = params[2 * i].t() if linear else params[2 * i]
        z = a @ W + params[2 * i + 1]
        if i == n - 1:
            return z.squeeze(1)
        if preacts is not None:
            preacts.append(z.detach())
        a = torch.cat([a, act_fn(act, z)], 1)


def drift(kind, vec, x):
    if kind == DRIFT_DWELL:
        return -(4.0 * vec * (x * (x * x - 1.0)))
    if kind == DRIFT_DIAG:
        return vec * x
    return torch.zeros_like(x)


def h_pde(kind, par, x, y, z):
    if kind == H_QUAD:
        return -0.5 * torch.sum(z ** 2, 1)
    if kind == H_ALLEN_CAHN:
        return y - y ** 3
    if kind >= H_EXP_LIN:
        al, dd, e = par[0], par[1], par[2]
        rr = torch.sum(x ** 2, 1)
        lin = 2.0 * al * (2.0 * al * rr + dd) + e
        nl = 0.0
        if kind != H_EXP_LIN:
            arg = torch.exp(2.0 * al * rr) - y ** 2
            nl = arg if kind == H_EXP_SQ else torch.sin(arg)
        return nl - y * lin
    return torch.zeros_like(y)


def terms(case, params=None, dtype=torch.float64, create_graph=True, preacts=None, lap_cols=None, detach_y=False):
    """(V (K,), grad V (K, n_in), Lap V over the first ``lap_cols`` input columns (K,), R (K,)) of ``case`` in ``dtype``, all on
    the graph of ``params``.  The two switches state wrong residuals for the tests of the tests: ``lap_cols`` other than d sums
    second derivatives over other columns, ``detach_y`` cuts h's dependence on V out of the gradient (R itself is unchanged)."""
    if params is None:
        params = [p.to(dtype) for p in case["params"]]
    d = case["d"]
    x = case["x"].to(dtype)
    cols = [x] + ([case["t"].to(dtype).reshape(-1, 1)] if case["parabolic"] else [])
    inp = torch.cat(cols, 1).requires_grad_(True)
    V = net(params, case["act"], inp, case["linear"], preacts)
    g, = torch.autograd.grad(V.sum(), inp, create_graph=True)
    lap = torch.zeros_like(V)
    for j in range(d if lap_cols is None else lap_cols):
        lap = lap + torch.autograd.grad(g[:, j].sum(), inp, create_graph=create_graph, retain_graph=True)[0][:, j]
    s = case["s"]
    xs = inp[:, :d].detach()
    vec = None if case["drift"] is None else case["drift"].to(dtype)
    R = 0.5 * s * s * lap + torch.sum(drift(case["drift_kind"], vec, xs) * g[:, :d], 1) \
        + h_pde(case["h_kind"], case["h_par"], xs, V.detach() if detach_y else V, s * g[:, :d])
    if case["parabolic"]:
        R = R + g[:, d]
    return V, g, lap, R


def residual(case, params=None, dtype=torch.float64, create_graph=True, preacts=None):
    """R (K,) of ``case`` (see make_case) in ``dtype``; differentiable in ``params`` (default: the case's, cast)."""
    return terms(case, params, dtype, create_graph, preacts)[3]


def parts(case, dtype=torch.float64, **switches):
    """(V (K,), grad V (K, n_in), the Laplacian summed over the space columns (K,), R (K,)) in ``dtype``, detached: what the
    forward kernel leaves in its scratch, what the finish kernel sums, and the residual."""
    return tuple(v.detach() for v in terms(case, None, dtype, create_graph=False, **switches))


def flat_grad(grads, params):
    return torch.cat([(torch.zeros_like(p) if g is None else g).reshape(-1) for g, p in zip(grads, params)])


def weighted_grads(case, rbars, dtype=torch.float64, **switches):
    """[d(sum_k rbar_k R_k)/dtheta for rbar in rbars], flat in registration order, in ``dtype``: one residual graph for all."""
    params = [p.to(dtype).clone().requires_grad_(True) for p in case["params"]]
    R = terms(case, params, dtype, **switches)[3]
    out = []
    for rbar in rbars:
        out.append(flat_grad(torch.autograd.grad(torch.sum(rbar.to(dtype) * R), params, allow_unused=True, retain_graph=True),
                             params))
    return out


def weighted_grad(case, rbar, dtype=torch.float64, **switches):
    """d(sum_k rbar_k R_k)/dtheta: what psp_pinn_backward returns for the weights ``rbar`` (K,)."""
    return weighted_grads(case, [rbar], dtype, **switches)[0]


def per_sample_grad(case, k, dtype=torch.float64):
    """dR_k/dtheta: weighted_grad with a one-hot weight."""
    return weighted_grad(case, one_hot(case["K"], k), dtype)


def one_hot(K, k):
    w = torch.zeros(K, dtype=torch.float64)
    w[k] = 1.0
    return w


def mean_square_rbar(alpha0, K):
    """R -> dLoss/dR of alpha0 mean(R^2)."""
    return lambda R: (2.0 * alpha0 / K) * R


def variance_rbar(alpha0, K):
    """R -> dLoss/dR of alpha0 var(R) (unbiased)."""
    return lambda R: (2.0 * alpha0 / (K - 1)) * (R - R.mean())


def blocks(case, flat):
    """A flat gradient split into its named blocks W1, b1, .., Wout, bout (registration order), as an ordered dict of views."""
    n, off, out = len(case["params"]) // 2, 0, {}
    for i, p in enumerate(case["params"]):
        layer = "out" if i // 2 == n - 1 else str(i // 2 + 1)
        out[("W" if i % 2 == 0 else "b") + layer] = flat[off:off + p.numel()]
        off += p.numel()
    assert off == flat.numel(), (off, flat.numel())
    return out


def loss_and_grad(case, alpha0=1.0, log_variance=False, dtype=torch.float64):
    """(R, loss, flat gradient of the loss in the parameters' registration order), all in ``dtype``."""
    params = [p.to(dtype).clone().requires_grad_(True) for p in case["params"]]
    R = residual(case, params, dtype)
    loss = alpha0 * (torch.var(R) if log_variance else torch.mean(R ** 2))
    grads = torch.autograd.grad(loss, params, allow_unused=True)           # (an h without y never reads the output bias)
    return R.detach(), loss.detach(), torch.cat([(torch.zeros_like(p) if g is None else g).reshape(-1)
                                                 for g, p in zip(grads, params)])


def preact_margin(case):
    """min |z| / max |z| over every sample and hidden unit in float64 (relu^2: phi'' jumps at z = 0)."""
    pre = []
    params = [p.to(torch.float64) for p in case["params"]]
    cols = [case["x"].double()] + ([case["t"].double().reshape(-1, 1)] if case["parabolic"] else [])
    net(params, case["act"], torch.cat(cols, 1), case["linear"], pre)
    z = torch.cat([p.reshape(-1) for p in pre]).abs()
    return float(z.min() / z.max())


def make_case(d, parabolic, arch, K, act="relu2", seed=0, linear=False, drift_kind=DRIFT_ZERO, h_kind=H_ALLEN_CAHN,
              h_par=(0.0, 0.0, 0.0, 0.0), s=2.0 ** 0.5):
    """Fixed inputs: fp32-representable float64 parameters of fan-in scale, x in (-1, 1)^d, t in (0, 1)."""
    g = torch.Generator().manual_seed(seed)
    n_in = d + (1 if parabolic else 0)
    dims = [n_in] + list(arch) + [1]
    params, fan = [], 0
    for i in range(len(dims) - 1):
        fan += dims[i]
        W = torch.randn(fan, dims[i + 1], generator=g) / fan ** 0.5
        params += [(W.t().contiguous() if linear else W).double(), (0.3 * torch.randn(dims[i + 1], generator=g)).double()]
    x = (2.0 * torch.rand(K, d, generator=g) - 1.0).double()
    t = torch.rand(K, generator=g).double()
    vec = None if drift_kind == DRIFT_ZERO else (0.5 + torch.rand(d, generator=g)).double()
    return dict(d=d, parabolic=parabolic, arch=list(arch), K=K, act=act, linear=linear, params=params, x=x, t=t,
                s=float(torch.tensor(s, dtype=torch.float32)),
                drift_kind=drift_kind, drift=vec, h_kind=h_kind, h_par=tuple(float(v) for v in h_par))
