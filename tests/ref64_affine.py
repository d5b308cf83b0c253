"""Float64 statement of what the linear-control kernels (csrc/aff_kernels.h behind psp_aff_*) compute: plain torch autograd on the
CPU, nothing drawn inside.  Every argument is what the kernels get (fp32 values), cast to `dtype`; dtype=torch.float32 runs the
same statement in fp32, the yardstick printed next to every kernel error.

Per step n (reference solver.py:449-486), with Z_n = M_n X_n + c_n:
    X_{n+1} = X_n + b(X_n) dt + B (xi_{n+1} sqrt(dt) - Z_n dt [adaptive])
    Y      += (|Z|^2 / 2 + f(X_{n+1}) - |Z|^2 [adaptive]) dt + Z . xi_{n+1} sqrt(dt)
    Zsum   += (|Z|^2 / 2 + f(X_{n+1})) dt
    u_L2   += |-Z_n - u*_n|^2 dt,   u*_n = table row n (TABLE) or G_n X_{n+1} (LINEAR)
D = Y - g(X_N), or -(Zsum + g(X_N)) for the relative entropy (include/psp.h).

The loss is given by per-trajectory numbers (include/psp.h, psp_aff_adjoint_sweep / psp_aff_rollout_bwd):
    detached or non-adaptive (store_path 1):  L = sum_k w_k D_k, the control in the increment and in Z . c held constant
    attached (store_path 2 and 3):            L = sum_k mu_k Y_k + nu_k Zsum_k + wT_k g(X_N,k),  wT = nu - mu when not given
"""
import torch

# include/psp.h
DRIFT_ZERO, DRIFT_DENSE, DRIFT_DIAG, DRIFT_DWELL = 0, 1, 2, 3
SIGMA_IDENTITY, SIGMA_DENSE, SIGMA_SCALED = 0, 1, 2
RUN_ZERO, RUN_DIAGQ = 0, 1
TERM_LINEAR, TERM_DIAGQ, TERM_SHIFTED = 0, 1, 2
UL2_TABLE, UL2_LINEAR = 0, 1


def drift_of(kind, tab, x):
    if kind == DRIFT_DENSE:
        return x @ tab.t()
    if kind == DRIFT_DIAG:
        return tab * x
    if kind == DRIFT_DWELL:
        return -4.0 * tab * (x * (x * x - 1.0))
    return torch.zeros_like(x)


def terminal_of(kind, tab, x):
    if kind == TERM_LINEAR:
        return (tab * x).sum(1)
    if kind == TERM_DIAGQ:
        return (tab * x * x).sum(1)
    return (tab * (x - 1.0) ** 2).sum(1)


def statement(d, K, N, dt, sqdt, M, c, drift, sigma, runcost, term, sigma_scale, adaptive, attached, x0, xi, relent=False,
              ul2=None, w=None, mu=None, nu=None, wT=None, y0=0.0, ul2_at_old_state=False, dtype=torch.float64):
    """drift / sigma / runcost / term: (kind, table or None); M (N, d, d) or None; c (N, d) or None; x0 (d) or (K, d);
    xi (N + 1, K, d), slice n + 1 drives step n; y0: the start of Y (the kernels' optional device scalar); ul2: None or (UL2_TABLE, (N, d)) or (UL2_LINEAR, (N, d, d)).
    ul2_at_old_state evaluates the LINEAR reference at X_n: a planted error for tests/test_ref64_affine.py, never the kernels'.
    Returns a dict of `dtype` tensors: D, Y, Zsum, XN, ul2 (K) or None, X (N + 1, K, d), Z (N, K, d), dZ (N, K, d) = dL/dZ_n per
    trajectory, dM (N, d, d) or None, dc (N, d) or None."""
    cast = lambda t: None if t is None else torch.as_tensor(t).detach().to(dtype)
    dt, sqdt, s = float(dt), float(sqdt), float(sigma_scale)
    M = None if M is None else cast(M).clone().requires_grad_(True)
    c = None if c is None else cast(c).clone().requires_grad_(True)
    (dk, dtab), (sk, stab), (rk, rtab), (tk, ttab) = [(k, cast(t)) for k, t in (drift, sigma, runcost, term)]
    xi = cast(xi)
    X = cast(x0).expand(K, d) if x0.dim() == 1 else cast(x0)
    assert X.shape == (K, d) and xi.shape == (N + 1, K, d)
    uk, utab = (None, None) if ul2 is None else (ul2[0], cast(ul2[1]))
    Y, Zs, ul = torch.full((K,), float(y0), dtype=dtype), torch.zeros(K, dtype=dtype), torch.zeros(K, dtype=dtype)
    Xs, Zl = [X], []
    through_state = attached and adaptive
    for n in range(N):
        Z = torch.zeros(K, d, dtype=dtype)
        if M is not None:
            Z = Z + X @ M[n].t()
        if c is not None:
            Z = Z + c[n]
        Z.retain_grad()
        Zl.append(Z)
        x_n = xi[n + 1]
        ctl = -(Z if through_state else Z.detach()) if adaptive else torch.zeros_like(Z)      # solver.py:451-469
        wiener = x_n * sqdt + ctl * dt
        if sk == SIGMA_DENSE:
            wiener = wiener @ stab.t()
        elif sk == SIGMA_SCALED:
            wiener = s * wiener
        Xn = X + drift_of(dk, dtab, X) * dt + wiener
        f = (rtab * Xn * Xn).sum(1) if rk == RUN_DIAGQ else torch.zeros(K, dtype=dtype)
        zz = (Z * Z).sum(1)
        Y = Y + (0.5 * zz + f + (Z * ctl).sum(1)) * dt + (Z * x_n).sum(1) * sqdt
        Zs = Zs + (0.5 * zz + f) * dt
        if uk == UL2_TABLE:
            ul = ul + ((-Z - utab[n]) ** 2).sum(1) * dt
        elif uk == UL2_LINEAR:
            ul = ul + ((-Z - (X if ul2_at_old_state else Xn) @ utab[n].t()) ** 2).sum(1) * dt
        X = Xn
        Xs.append(X)
    g = terminal_of(tk, ttab, X)
    D = -(Zs + g) if relent else Y - g
    if attached:
        mu_ = cast(mu) if mu is not None else torch.zeros(K, dtype=dtype)
        nu_ = cast(nu) if nu is not None else torch.zeros(K, dtype=dtype)
        wT_ = cast(wT) if wT is not None else nu_ - mu_
        L = (mu_ * Y + nu_ * Zs + wT_ * g).sum()
    else:
        L = (cast(w) * D).sum()
    L.backward()
    det = lambda t: None if t is None else t.detach()
    return dict(D=det(D), Y=det(Y), Zsum=det(Zs), XN=det(X), ul2=det(ul) if uk is not None else None,
                X=torch.stack([det(x) for x in Xs]), Z=torch.stack([det(z) for z in Zl]),
                dZ=torch.stack([z.grad if z.grad is not None else torch.zeros(K, d, dtype=dtype) for z in Zl]),
                dM=None if M is None else M.grad, dc=None if c is None else c.grad, L=det(L))
