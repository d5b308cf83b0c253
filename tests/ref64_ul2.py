"""float64 statement of the control-ansatz Solver's u_L2 log, PER TRAJECTORY -- CPU only.

solver.py:491-494 (the log line sits AFTER the Euler step of solver.py:471-472):

    ul2_k = dt sum_n | -Z_n(X_n, t_n) - u*(X_{n+1}, t_n) |^2,        u_L2_loss = mean_k ul2_k

Z (N, K, d) and X (N + 1, K, d) are those of ref64.iteration(..., want_path=True); dt is the fp32 step cast to double, as there.
u* comes from the PACKAGE problem's own data (problems.py), in the three descriptions HjbNativePlan forms of it; each starts from
the fp32 numbers the plan uploads, cast to double:
  'table'  u* does not depend on x (LLGC): rows u_true(0, n dt), accumulated inside the forward kernels;
  'gains'  u* = M_n x (LQGC): M_n by probing u_true with the unit vectors, logged from the path store;
  'grid'   per-coordinate tables on a grid (the double wells, u_true_tables()), read with the reference's cell rule: clamp to
           [-xb, xb - 2 dx], floor((x + xb) / dx), the globally LAST trajectory's index lowered by two (a negative index counts
           from the row's end, as numpy and torch read it).
dtype=torch.float32 runs the same statements in fp32: the stand-in ul2_32 whose distance from ul2_64 is the error scale of the
GPU bound (tests/test_ref64_ul2.py).
"""
import numpy as np
import torch

F64 = torch.float64


def describe(problem, N, dt_np):
    """The description of u* on the time grid t_n = n dt_np, n < N, from a package problem (device 'cpu'): dict(kind, ...)
    with fp32 tensors, formed as HjbNativePlan.__init__ forms what it uploads."""
    d = problem.d
    tables = getattr(problem, "u_true_tables", lambda: None)()
    if tables is not None:
        return dict(kind="grid", tables=[torch.tensor(np.asarray(t), dtype=torch.float32) for t in tables["tables"]],
                    group=torch.tensor(tables["group_of_dim"], dtype=torch.long), xb=float(tables["xb"]), dx=float(tables["dx"]),
                    row=[int(np.ceil(n * dt_np / tables["delta_t"])) for n in range(N)])
    if getattr(problem, "u_true_x_independent", False) is True:
        probe = torch.zeros(1, d)
        rows = [torch.tensor(np.asarray(problem.u_true(probe, n * dt_np))).reshape(d, -1)[:, 0].float() for n in range(N)]
        return dict(kind="table", table=torch.stack(rows))
    assert getattr(problem, "u_true_linear_in_x", False) is True, "no description of u_true for this problem"
    eye = torch.eye(d)                                                   # u_true returns (d, K): column i = M e_i
    gains = [torch.tensor(np.asarray(problem.u_true(eye, n * dt_np))).reshape(d, d).float() for n in range(N)]
    return dict(kind="gains", gains=torch.stack(gains))


def grid_cells(desc, X, last, dtype=F64):
    """(cell (K, d) int64, q (K, d), xc (K, d)) of the reference's rule in `dtype` arithmetic; last: whether row K - 1 is the
    globally last trajectory."""
    xb, dx = desc["xb"], desc["dx"]
    xc = torch.clamp(X.to(dtype), -xb, xb - 2 * dx)
    q = (xc + xb) / dx
    cell = torch.floor(q).long()
    if last:
        cell[-1, :] -= 2
    return cell, q, xc


def u_star(desc, X, n, last=True, dtype=F64):
    """u*(X, t_n) (K, d) in `dtype`; for the grid kind also the quotient q and the clamped state (else None, None)."""
    X = X.to(dtype)
    if desc["kind"] == "table":
        return desc["table"][n].to(dtype).expand_as(X), None, None
    if desc["kind"] == "gains":
        return X @ desc["gains"][n].to(dtype).t(), None, None
    cell, q, xc = grid_cells(desc, X, last, dtype)
    u = torch.empty_like(X)
    for gi, tab in enumerate(desc["tables"]):
        dims = torch.nonzero(desc["group"] == gi).flatten()
        if dims.numel():
            u[:, dims] = tab[desc["row"][n]].to(dtype)[cell[:, dims]]
    return u, q, xc


def ul2(desc, Z, X, dt, last=True, dtype=F64, delta=None):
    """ul2_k (K,) in `dtype` from Z (N, K, d) and X (N + 1, K, d).  Grid kind with delta: returns (ul2, near), near_k true if some
    (n, i) has its cell quotient (xc + xb) / dx within delta of an integer; a state clamped to -xb has quotient 0 exactly in every
    precision and is not near (tests/ref64_is.py)."""
    N, K, d = Z.shape
    assert X.shape == (N + 1, K, d), (tuple(X.shape), (N + 1, K, d))
    tot = torch.zeros(K, dtype=dtype)
    near = torch.zeros(K, dtype=torch.bool)
    for n in range(N):
        u, q, xc = u_star(desc, X[n + 1], n, last, dtype)
        tot = tot + torch.sum((-Z[n].to(dtype) - u) ** 2, 1)
        if q is not None and delta is not None:
            near |= (((q - torch.round(q)).abs() < delta) & (xc > -desc["xb"])).any(1)
    out = tot * dt
    assert out.dtype == dtype
    return (out, near) if (desc["kind"] == "grid" and delta is not None) else out
