"""Plain numpy references of ONE psp_is_rollout call (include/psp.h psp_is_config, csrc/hjbe_kernels.h): the forward-only
importance-sampling rollout under a reference control u* or under no control.  numpy only: no torch device, no ctypes.

A call is described by a dict `desc` (tests/is_kernel_cases.py builds it):
  d, K_local, K_global, k_offset, N     ints
  dt, sqrt_dt                           the fp32 values the config holds (Python floats)
  drift_kind, sigma_kind, runcost_kind, term_kind, dwell_form, sigma_scale
  drift     DENSE: A (d, d); DIAG: a (d); DOUBLE_WELL: kappa (d); ZERO: None          fp32 arrays
  sigma     DENSE: B (d, d), else None
  runcost   DIAG_QUAD: p (d), else None
  term      (d)
  control_kind and its data: TABLE 'table' (N, d); LINEAR 'gains' (N, d, d); GRID 'tables' (G, nrows, ncols), 'group' (d) int,
            'row' (N) int, 'xb', 'dx', 'xhi' (fp32 values), 'nrows', 'ncols'
  x0 (d), noise (N + 1, K_local, d)     fp32 arrays; slice n + 1 drives step n, slice 0 is never read

The recursion, per step n from X_0 = x0 (psp_is_config):
    u       = u*(X_n, t_n)                                  taken BEFORE the update; 0 for ISC_NONE
    X_n+1   = X_n + (b(X_n) + sigma u) dt + sigma xi_n+1 sqrt(dt)
    logw   += -f(X_n+1) dt - u . xi_n+1 sqrt(dt) - |u|^2 dt / 2
and logw -= g(X_N) at the end.

rollout64: every sum in float64, every fp32 input at its fp32 value.  The grid cell follows csrc/ugrid.h on the float64 state.
rollout32: the same recursion in numpy float32 in the order the kernel documents, one rounding per operation (numpy fuses
nothing); the elementwise drift / sigma kinds and the TABLE / GRID controls are promised to match the kernel bit for bit.
"""
import numpy as np

DRIFT_ZERO, DRIFT_DENSE, DRIFT_DIAG, DRIFT_DWELL = 0, 1, 2, 3
SIGMA_IDENTITY, SIGMA_DENSE, SIGMA_SCALED = 0, 1, 2
RUN_ZERO, RUN_DIAGQ = 0, 1
TERM_LINEAR, TERM_DIAGQ, TERM_SHIFTED = 0, 1, 2
ISC_NONE, ISC_TABLE, ISC_LINEAR, ISC_GRID = 0, 1, 2, 3

NEAR_WINDOW = 1e-4          # in cells: a lookup this close to a cell edge may resolve differently from an fp32 state


def last_local(desc):
    """Local index of the globally last trajectory (k_offset + k = K_global - 1), or None when another call holds it."""
    k = int(desc["K_global"]) - 1 - int(desc["k_offset"])
    return k if 0 <= k < int(desc["K_local"]) else None


def _grid_cells(X, desc, dtype):
    """(cells (K, d) int, q (K, d), xc (K, d)) of csrc/ugrid.h in `dtype` arithmetic: clamp to [-xb, xhi], floor((xc + xb) / dx),
    the last global trajectory lowered by two, a negative cell counting from the row's end, the final clamp."""
    xb, dx, xhi = dtype(desc["xb"]), dtype(desc["dx"]), dtype(desc["xhi"])
    nc = int(desc["ncols"])
    xc = np.minimum(np.maximum(X, -xb), xhi)
    q = (xc + xb) / dx
    assert q.dtype == dtype
    cell = np.floor(q).astype(np.int64)
    kl = last_local(desc)
    if kl is not None:
        cell[kl] -= 2
    cell = np.where(cell < 0, cell + nc, cell)
    return np.clip(cell, 0, nc - 1), q, xc


def _grid_u(X, n, desc, dtype):
    cell, q, xc = _grid_cells(X, desc, dtype)
    tables = np.asarray(desc["tables"])
    group = np.clip(np.asarray(desc["group"], dtype=np.int64), 0, tables.shape[0] - 1)
    row = int(np.clip(int(desc["row"][n]), 0, int(desc["nrows"]) - 1))
    return tables[group[None, :], row, cell].astype(dtype), q, xc


def _near(X, q, xc, desc):
    """Lookups whose cell an fp32 state may legitimately resolve differently: (xc + xb) / dx within NEAR_WINDOW of an integer, or
    the state within NEAR_WINDOW dx of a clamp bound.  A state clamped to -xb gives (xc + xb) / dx = 0 exactly in every precision
    (not flagged: the bound test on the state itself covers the ambiguous ones); a state clamped to xhi is flagged when
    (xhi + xb) / dx lies near an integer."""
    xb, dx, xhi = float(desc["xb"]), float(desc["dx"]), float(desc["xhi"])
    edge = (np.abs(q - np.rint(q)) < NEAR_WINDOW) & (xc > -xb)
    bound = (np.abs(X + xb) < NEAR_WINDOW * dx) | (np.abs(X - xhi) < NEAR_WINDOW * dx)
    return np.any(edge | bound, axis=1)


def rollout64(desc):
    """(logw (K_local), XN (K_local, d)) float64, and for ISC_GRID a boolean near (K_local)."""
    d, K, N = int(desc["d"]), int(desc["K_local"]), int(desc["N"])
    f8 = np.float64
    dt, sq, s = f8(desc["dt"]), f8(desc["sqrt_dt"]), f8(desc["sigma_scale"])
    ctrl = desc["control_kind"]
    arr = lambda v: None if v is None else np.asarray(v).astype(f8)      # (an fp32 array keeps its fp32 values)
    drift, B, p, term = arr(desc["drift"]), arr(desc["sigma"]), arr(desc["runcost"]), arr(desc["term"])
    noise = np.asarray(desc["noise"])
    assert noise.shape == (N + 1, K, d), noise.shape
    X = np.tile(arr(desc["x0"]).reshape(1, d), (K, 1))
    fint, ito, riem = np.zeros(K), np.zeros(K), np.zeros(K)
    near = np.zeros(K, dtype=bool)

    def apply_sigma(v):
        if desc["sigma_kind"] == SIGMA_DENSE:
            return v @ B.T
        return s * v if desc["sigma_kind"] == SIGMA_SCALED else v

    for n in range(N):
        if ctrl == ISC_TABLE:
            u = np.tile(arr(desc["table"])[n].reshape(1, d), (K, 1))
        elif ctrl == ISC_LINEAR:
            u = X @ arr(desc["gains"])[n].T
        elif ctrl == ISC_GRID:
            u, q, xc = _grid_u(X, n, desc, f8)
            near |= _near(X, q, xc, desc)
        else:
            u = np.zeros((K, d))
        xi = noise[n + 1].astype(f8)
        kind = desc["drift_kind"]
        if kind == DRIFT_DENSE:
            b = X @ drift.T
        elif kind == DRIFT_DIAG:
            b = drift * X
        elif kind == DRIFT_DWELL:
            b = -4.0 * drift * X * (X * X - 1.0)
        else:
            b = np.zeros((K, d))
        ito += np.sum(u * xi, axis=1) * sq
        riem += np.sum(u * u, axis=1) * dt
        X = X + (b + apply_sigma(u)) * dt + apply_sigma(xi) * sq
        if desc["runcost_kind"] == RUN_DIAGQ:
            fint += np.sum(p * X * X, axis=1) * dt
    tk = desc["term_kind"]
    if tk == TERM_LINEAR:
        g = X @ term
    elif tk == TERM_DIAGQ:
        g = np.sum(term * X * X, axis=1)
    else:
        g = np.sum(term * (X - 1.0) ** 2, axis=1)
    logw = -fint - g - ito - 0.5 * riem
    return (logw, X, near) if ctrl == ISC_GRID else (logw, X)


def rollout32(desc):
    """(logw (K_local), XN (K_local, d)) float32: the kernel's documented operation order, every operation rounded once."""
    d, K, N = int(desc["d"]), int(desc["K_local"]), int(desc["N"])
    f4 = np.float32
    dt, sq, s = f4(desc["dt"]), f4(desc["sqrt_dt"]), f4(desc["sigma_scale"])
    one, four, half = f4(1.0), f4(4.0), f4(0.5)
    ctrl = desc["control_kind"]
    arr = lambda v: None if v is None else np.asarray(v, dtype=f4)
    drift, B, p, term = arr(desc["drift"]), arr(desc["sigma"]), arr(desc["runcost"]), arr(desc["term"])
    noise = arr(desc["noise"])
    x = np.tile(arr(desc["x0"]).reshape(1, d), (K, 1))
    fint, ito, riem = np.zeros(K, f4), np.zeros(K, f4), np.zeros(K, f4)
    denseA, denseB = desc["drift_kind"] == DRIFT_DENSE, desc["sigma_kind"] == SIGMA_DENSE
    scaled = desc["sigma_kind"] == SIGMA_SCALED

    def drift_elem(xv):
        if desc["drift_kind"] == DRIFT_DIAG:
            return drift * xv
        if desc["drift_kind"] == DRIFT_DWELL:
            k4 = four * drift
            if desc["dwell_form"]:
                return -((k4 * xv) * (xv * xv - one))
            return -(k4 * (xv * (xv * xv - one)))
        return np.zeros((K, d), f4)

    for n in range(N):
        if ctrl == ISC_TABLE:
            u = np.tile(arr(desc["table"])[n].reshape(1, d), (K, 1))
        elif ctrl == ISC_LINEAR:
            u = np.dot(x, arr(desc["gains"])[n].T)
        elif ctrl == ISC_GRID:
            u = _grid_u(x, n, desc, f4)[0]
        else:
            u = np.zeros((K, d), f4)
        xi = noise[n + 1]
        if ctrl != ISC_NONE:
            pu, uu = np.zeros(K, f4), np.zeros(K, f4)
            for i in range(d):
                pu = pu + u[:, i] * xi[:, i]
                uu = uu + u[:, i] * u[:, i]
            ito = ito + pu * sq
            riem = riem + uu * dt
        b = np.dot(x, drift.T) if denseA else drift_elem(x)
        if denseB:
            v = (u * dt + xi * sq) if ctrl != ISC_NONE else xi * sq
            x = (x + b * dt) + np.dot(v, B.T)
        else:
            if ctrl != ISC_NONE:
                b = b + (s * u if scaled else u)
            x = (x + b * dt) + (s * xi if scaled else xi) * sq
        assert x.dtype == f4 and b.dtype == f4
        if desc["runcost_kind"] == RUN_DIAGQ:
            f = np.zeros(K, f4)
            for i in range(d):
                f = f + x[:, i] * (p[i] * x[:, i])
            fint = fint + f * dt
    g = np.zeros(K, f4)
    for i in range(d):
        xv = x[:, i]
        if desc["term_kind"] == TERM_LINEAR:
            g = g + term[i] * xv
        elif desc["term_kind"] == TERM_DIAGQ:
            g = g + xv * (term[i] * xv)
        else:
            e = xv - one
            g = g + term[i] * (e * e)
    lw = -fint - g
    if ctrl != ISC_NONE:
        lw = (lw - ito) - half * riem
    assert lw.dtype == f4
    return lw, x


def errors(logw, XN, logw64, XN64, keep=None):
    """(E_w, E_x) of a result against rollout64: E_w = max_k |logw - logw64| / max(1, |logw64|) per trajectory,
    E_x = max |XN - XN64| / max(1, max |XN64|); `keep` selects the trajectories that count (the scale of E_x is theirs)."""
    logw, XN = np.asarray(logw, dtype=np.float64), np.asarray(XN, dtype=np.float64)
    if keep is None:
        keep = np.ones(logw64.shape[0], dtype=bool)
    if not keep.any():
        return 0.0, 0.0
    ew = np.abs(logw - logw64)[keep] / np.maximum(1.0, np.abs(logw64[keep]))
    ex = np.abs(XN - XN64)[keep] / max(1.0, float(np.abs(XN64[keep]).max()))
    return float(ew.max()), float(ex.max())
