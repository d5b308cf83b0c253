"""PDE / control problem definitions (API mirror of the hot-path part of the reference's
problems.py).  A problem is a duck-typed object with attributes ``d, T, X_0, B, name`` and
methods ``b(x), sigma(x), h(t, x, y, z), f(...), g(x)`` -- exactly what the reference's
solvers call.  Differences from the reference:

* the device is a constructor argument (``device=None`` -> CUDA/HIP if present, else CPU)
  instead of the module global ``device = pt.device('cuda')`` (reference problems.py:11);
* ``native_spec()`` describes the coefficient functions as a closed catalogue entry
  (dense / diagonal / double-well drift, dense / identity sigma, diagonal quadratic costs)
  so that Solver can run the hand-written HIP rollout.  Objects without ``native_spec``
  (any user-supplied problem) run through the composite torch plan.

Random matrices are drawn from the torch CPU generator in the reference's order, so equal
seeds give identical A, B.
"""
import numpy as np
import torch
from scipy.linalg import expm

try:
    from . import native as _nat
except ImportError:  # flat import (sys.path points at this directory)
    import native as _nat


def default_device():
    return torch.device('cuda' if torch.cuda.is_available() else 'cpu')


def _resolve(device):
    return default_device() if device is None else torch.device(device)


def coefficients_overridden(problem, names=('b', 'sigma', 'h', 'f', 'g')):
    """Name of a coefficient method that is NOT this module's catalogue implementation (a subclass override or an attribute
    patched onto the instance), else None.  native_spec() / general_native_spec() describe the catalogue formulas, so a
    problem whose b / sigma / h / f / g was replaced must run on the composite torch plan, which calls the Python methods."""
    for name in names:
        if name in getattr(problem, '__dict__', {}):
            return name
        fn = getattr(type(problem), name, None)
        if fn is not None and getattr(fn, '__module__', None) != __name__:
            return name
    return None


def _classify_matrix(M):
    """'identity' | ('scaled', s) | ('diag', vec) | 'dense' for a square matrix."""
    Mc = M.detach().cpu()
    d = Mc.shape[0]
    off = Mc - torch.diag(torch.diagonal(Mc))
    if torch.count_nonzero(off) != 0:
        return 'dense', None
    diag = torch.diagonal(Mc).clone()
    if torch.equal(diag, torch.ones(d)):
        return 'identity', None
    if torch.all(diag == diag[0]):
        return 'scaled', float(diag[0])
    return 'diag', diag


class _LinearDriftMixin:
    """Shared pieces of the Ornstein-Uhlenbeck families (dense A, dense B)."""

    def b(self, x):
        return torch.mm(self.A, x.t()).t()

    def sigma(self, x):
        return self.B

    def _linear_spec(self):
        spec = {}
        kind, val = _classify_matrix(self.A)
        if kind == 'dense':
            spec['drift'] = (_nat.DRIFT_DENSE, self.A.contiguous())
        else:
            diag = torch.diagonal(self.A).contiguous()
            spec['drift'] = (_nat.DRIFT_DIAG, diag)
        kind, val = _classify_matrix(self.B)
        if kind == 'identity':
            spec['sigma'] = (_nat.SIGMA_IDENTITY, None, 1.0)
        elif kind == 'scaled':
            spec['sigma'] = (_nat.SIGMA_SCALED_IDENTITY, None, val)
        else:
            spec['sigma'] = (_nat.SIGMA_DENSE, self.B.contiguous(), 1.0)
        return spec


class LLGC(_LinearDriftMixin):
    """Ornstein-Uhlenbeck dynamics with linear terminal cost g(x) = alpha . x
    (reference problems.py:14-65)."""

    def __init__(self, name='LLGC', d=1, off_diag=0, T=5, seed=42, device=None):
        self.device = _resolve(device)
        torch.manual_seed(seed)
        self.name, self.d, self.T = name, d, T
        self.A = (-torch.eye(d) + off_diag * torch.randn(d, d)).to(self.device)
        self.B = (torch.eye(d) + off_diag * torch.randn(d, d)).to(self.device)
        self.alpha = torch.ones(d, 1).to(self.device)
        self.X_0 = torch.zeros(d).to(self.device)
        self.boundary, self.one_boundary, self.X_l, self.X_r = 'square', False, -2.0, 2.0
        if not np.all(np.linalg.eigvals(self.A.cpu().numpy()).real < 0):
            print('not all EV of A are negative')

    def f(self, x, t):
        return torch.zeros(x.shape[0]).to(x.device)

    def h(self, t, x, y, z):
        return -0.5 * torch.sum(z ** 2, dim=1)

    def g(self, x):
        return torch.mm(x, self.alpha)[:, 0]

    u_true_x_independent = True    # lets the native plan tabulate u*(t_n) once (plan_native.py)

    def u_true(self, x, t):
        # u*(x,t) = -B^T exp(A^T (T-t)) alpha, independent of x (reference problems.py:51-53)
        A, B = self.A.cpu().numpy(), self.B.cpu().numpy()
        col = B.T.dot(expm(A.T * (self.T - t)).dot(self.alpha.cpu().numpy()))
        return -(col * np.ones(x.shape).T)

    def native_spec(self):
        spec = self._linear_spec()
        spec['runcost'] = (_nat.RUNCOST_ZERO, None)
        spec['term'] = (_nat.TERM_LINEAR, self.alpha[:, 0].contiguous())
        return spec


class LQGC(_LinearDriftMixin):
    """Linear-quadratic Gaussian control: running cost x'Px, terminal cost x'Rx
    (reference problems.py:118-175)."""

    def __init__(self, name='LQGC', delta_t=0.05, d=1, off_diag=0, T=5, seed=42, device=None):
        self.device = _resolve(device)
        torch.manual_seed(seed)
        self.name, self.d, self.T = name, d, T
        self.A = (-torch.eye(d) + off_diag * torch.randn(d, d)).to(self.device)
        self.B = (torch.eye(d) + off_diag * torch.randn(d, d)).to(self.device)
        self.delta_t = delta_t
        self.N = int(np.floor(self.T / self.delta_t))
        self.X_0 = torch.zeros(d).to(self.device)
        if not np.all(np.linalg.eigvals(self.A.cpu().numpy()).real < 0):
            print('not all EV of A are negative')
        self.P = 0.5 * torch.eye(d).to(self.device)
        self.Q = 0.5 * torch.eye(d).to(self.device)
        self.R = torch.eye(d).to(self.device)
        self._riccati()

    def _riccati(self):
        """Backward Euler recursion for the value-function matrices F_n and offsets G_n
        (reference problems.py:140-152); host-side diagnostics only."""
        A, B, Q, P = (m.cpu() for m in (self.A, self.B, self.Q, self.P))
        F = torch.zeros(self.N + 1, self.d, self.d)
        F[self.N] = self.R.cpu()
        Qinv = Q.inverse()
        for n in range(self.N, 0, -1):
            Fn = F[n]
            F[n - 1] = Fn + (A.t() @ Fn + Fn @ A - Fn @ B @ Qinv @ B.t() @ Fn + P) * self.delta_t
        G = torch.zeros(self.N + 1)
        for n in range(self.N, 0, -1):
            G[n - 1] = G[n] - torch.trace(B @ F[n] @ B) * self.delta_t
        self.F, self.G = F, G

    def f(self, x, t):
        return torch.sum(x.t() * torch.mm(self.P, x.t()), 0)

    def g(self, x):
        return torch.sum(x.t() * torch.mm(self.R, x.t()), 0)

    def h(self, t, x, y, z):
        return -0.5 * torch.sum(z ** 2, dim=1) - self.f(x, t)

    u_true_linear_in_x = True      # u*(x, t) = M(t) x: the native plan tabulates M(t_n) once and logs u_L2 from its path store

    def u_true(self, x, t):
        n = int(np.ceil(t / self.delta_t))
        gain = self.Q.cpu().inverse() @ self.B.cpu().t() @ self.F[n]
        return -(gain @ x.t()).detach().numpy()

    def v_true(self, x, t):
        n = int(np.ceil(t / self.delta_t))
        return -torch.mm(x, torch.mm(self.F[n], x.t())).t() + self.G[n]

    def native_spec(self):
        kp, _ = _classify_matrix(self.P)
        kr, _ = _classify_matrix(self.R)
        if kp == 'dense' or kr == 'dense':
            return None
        spec = self._linear_spec()
        spec['runcost'] = (_nat.RUNCOST_DIAG_QUAD, torch.diagonal(self.P).contiguous())
        spec['term'] = (_nat.TERM_DIAG_QUAD, torch.diagonal(self.R).contiguous())
        return spec


class _DoubleWellBase:
    def _setup(self, d, d_1, d_2, eta, kappa):
        self.d, self.d_1, self.d_2 = d, d_1, d_2
        self.eta, self.kappa = eta, kappa
        self.eta_ = torch.tensor([eta] * d_1 + [1.0] * d_2).to(self.device)
        self.kappa_ = torch.tensor([kappa] * d_1 + [1.0] * d_2).to(self.device)
        self.B = torch.eye(d).to(self.device)
        self.X_0 = -torch.ones(d).to(self.device)
        self.ref_sol_is_defined = False

    def V(self, x):
        return self.kappa * (x ** 2 - 1) ** 2

    def grad_V(self, x):
        return 4.0 * self.kappa_ * (x * (x ** 2 - torch.ones(self.d).to(x.device)))

    def b(self, x):
        return -self.grad_V(x)

    def sigma(self, x):
        return self.B

    def _well_cost(self, x):
        return (torch.sum(self.eta_ * (x - torch.ones(self.d).to(x.device)) ** 2, 1)).squeeze()

    # ---- reference solution of the ONE-dimensional problem by finite differences (reference problems.py:216-281, 336-476) ---------
    # psi = exp(-v) solves the linear backward equation d_t psi + L psi = 0, psi(T) = exp(-g), L = generator of dX = -V'(X) dt + dW
    # (beta = 2): symmetrised as A = D^-1 L D with D = exp(beta V / 2), a tridiagonal matrix on nx cells of [-xb, xb] (reflecting
    # ends), stepped backwards by implicit Euler; the optimal control is u* = -d_x v = (1 / psi) d_x psi taken as a forward
    # difference of log psi.  Written here as array expressions (the reference fills the matrix entry by entry); the band of the
    # implicit step and the FLOAT32 rounding of the control table -- the reference multiplies by its fp32 tensor B[0, 0], which
    # makes every entry an fp32 number -- are kept, because u_L2 logs are compared with the reference's to the last digits.
    def _fd_reference(self, potential, terminal, delta_t, xb, nx):
        import numpy as np
        from scipy.linalg import solve_banded
        beta = 2
        dx = 2.0 * xb / nx
        cells = np.arange(nx)
        mid = -xb + (cells + 0.5) * dx                                   # cell midpoints
        lo_far, lo_edge = -xb + (cells - 0.5) * dx, -xb + cells * dx      # the neighbour below and the edge between
        hi_far, hi_edge = -xb + (cells + 1.5) * dx, -xb + (cells + 1) * dx
        V = potential
        diag_lo = np.exp(beta * (V(mid) - V(lo_edge))) / dx ** 2
        diag_hi = np.exp(beta * (V(mid) - V(hi_edge))) / dx ** 2
        off_hi = np.exp(beta * 0.5 * (V(hi_far) + V(mid) - 2 * V(hi_edge))) / dx ** 2
        main = np.where(cells > 0, diag_lo, 0.0) + np.where(cells < nx - 1, diag_hi, 0.0)
        A_main, A_up = -main / beta, off_hi[:nx - 1] / beta              # A = -(.) / beta; A[i, i + 1] = +off_hi[i] / beta
        n_steps = int(self.T / delta_t)
        xvec = np.linspace(-xb, xb, nx, endpoint=True)
        scale, unscale = np.exp(beta * V(xvec) / 2), np.exp(-beta * V(xvec) / 2)
        band = -delta_t * np.vstack([np.append([0], A_up), A_main - n_steps / self.T, np.append(A_up, [0])])
        psi = np.zeros([n_steps + 1, nx])
        psi[n_steps] = np.exp(-terminal(xvec))
        for n in range(n_steps - 1, -1, -1):
            psi[n] = scale * solve_banded([1, 1], band, unscale * psi[n + 1])
        diff = -np.log(psi[:, 1:]) + np.log(psi[:, :-1])
        u = ((np.float32(-2 / beta) * np.float32(self.B[0, 0].item())) * diff.astype(np.float32) / np.float32(dx)).astype(np.float64)
        return dict(xb=xb, nx=nx, dx=dx, delta_t=delta_t, xvec=xvec), psi, u

    def _table_index(self, x_col):
        """Grid cell of every entry of a (K,) column of states, as the reference computes it (fp32 arithmetic, states clamped to
        the grid) -- including its decrement of the LAST entry's index by two (problems.py:270, 276)."""
        x_col = x_col.detach().cpu().float().reshape(-1)
        idx = torch.floor((torch.clamp(x_col, -self.xb, self.xb - 2 * self.dx) + self.xb) / self.dx).long()
        idx[-1] -= 2
        return idx

    def _time_index(self, t):
        import numpy as np
        return int(np.ceil(float(t) / self.delta_t))

    def _value_index(self, x_col):
        """Grid cell for the VALUE tables (problems.py:392-394, 592-594): no clamp, same decrement of the last entry."""
        x_col = x_col.detach().cpu().float().reshape(-1)
        idx = torch.floor((x_col + self.xb) / self.dx).long()
        idx[-1] -= 2
        return idx

    # ---- the two tables of the multidimensional classes: coordinates < d_1 use (kappa, eta), the others (1, 1) ----------------------
    def V_2(self, x):
        return (x ** 2 - 1) ** 2

    def g_1(self, x_1):
        return self.eta * (x_1 - 1) ** 2

    def g_2(self, x_1):
        return (x_1 - 1) ** 2

    def _take_grid(self, grid):
        self.xb, self.nx, self.dx, self.delta_t, self.xvec = grid['xb'], grid['nx'], grid['dx'], grid['delta_t'], grid['xvec']

    def compute_reference_solution(self, delta_t=0.005, xb=2.5, nx=1000):
        grid, self.psi, self.u = self._fd_reference(self.V, self.g_1, delta_t, xb, nx)
        self._take_grid(grid)
        self._publish_u_true()

    def compute_reference_solution_2(self, delta_t=0.005, xb=2.5, nx=1000):
        grid, self.psi_2, self.u_2 = self._fd_reference(self.V_2, self.g_2, delta_t, xb, nx)
        self._take_grid(grid)
        self._publish_u_true()

    def _tables_ready(self):
        return hasattr(self, 'u') and (self.d_2 == 0 or hasattr(self, 'u_2'))

    def _publish_u_true(self):
        if self._tables_ready():
            self.ref_sol_is_defined = True
            self.u_true = self._u_true

    def _table_read(self, table, idx, t, transform=None):
        import numpy as np
        vals = table[self._time_index(t), idx.numpy()]
        return np.array(vals if transform is None else transform(vals)).reshape([1, len(idx)])

    def u_true_1(self, x, t):
        return self._table_read(self.u, self._table_index(x), t)

    def u_true_2(self, x, t):
        return self._table_read(self.u_2, self._table_index(x), t)

    def _value_transform(self):
        import numpy as np
        return None if getattr(self, 'modus', 'HJB') == 'linear' else (lambda p: -np.log(p))

    def v_true_1(self, x, t):
        return self._table_read(self.psi, self._value_index(x), t, self._value_transform())

    def v_true_2(self, x, t):
        return self._table_read(self.psi_2, self._value_index(x), t, self._value_transform())

    def _u_true(self, x, t):
        import numpy as np
        cols = [self.u_true_1(x[:, i], t).T for i in range(self.d_1)] + [self.u_true_2(x[:, i], t).T for i in range(self.d_1, self.d)]
        return np.concatenate(cols, 1).T

    def u_true_tables(self):
        """Tables and the coordinate -> table map for the native plan's device-side u_L2 log (plan_native._ul2_from_path)."""
        if not self.ref_sol_is_defined:
            return None
        tables = [self.u] + ([self.u_2] if self.d_2 > 0 else [])
        return dict(tables=tables, group_of_dim=[0] * self.d_1 + [1] * self.d_2, xb=self.xb, dx=self.dx, delta_t=self.delta_t)


class DoubleWell(_DoubleWellBase):
    """One-dimensional double-well potential (reference problems.py:178-283): dX = -V'(X) dt + dW, V = kappa (x^2 - 1)^2,
    g = eta (x - 1)^2; ``compute_reference_solution()`` tabulates the optimal control, ``u_true`` / ``v_true`` read the table."""

    def __init__(self, name='Double well', d=1, T=1, eta=1, kappa=1, device=None):
        self.device = _resolve(device)
        self.name, self.T = name, T
        self._setup(d, d, 0, eta, kappa)
        if d != 1:
            print('The double well example is only implemented for d = 1.')

    def h(self, t, x, y, z):
        return -0.5 * torch.sum(z ** 2, dim=1)

    def f(self, x, t):
        return torch.zeros(x.shape[0]).to(x.device)

    def g(self, x):
        return (self.eta * (x - 1) ** 2).squeeze()

    def grad_V(self, x):
        return 4.0 * self.kappa * x * (x ** 2 - 1)

    def compute_reference_solution(self, delta_t=0.005, xb=2.5, nx=1000):
        grid, self.psi, self.u = self._fd_reference(self.V, lambda x: self.eta * (x - 1) ** 2, delta_t, xb, nx)
        self.xb, self.nx, self.dx, self.delta_t, self.xvec = grid['xb'], grid['nx'], grid['dx'], grid['delta_t'], grid['xvec']
        self.ref_sol_is_defined = True

    def v_true(self, x, t):
        import numpy as np
        x = x.detach().cpu().float()
        idx = torch.floor((x.squeeze(0) + self.xb) / self.dx).long()
        idx[-1] -= 2
        return np.array(-np.log(self.psi[self._time_index(t), idx.numpy()])).reshape([1, len(idx)])

    def u_true(self, x, t):
        import numpy as np
        idx = self._table_index(x).reshape(x.shape) if x.dim() > 1 else self._table_index(x)
        return np.array(self.u[self._time_index(t), idx.numpy()]).reshape([1, len(idx)])

    def u_true_tables(self):
        """What the native plan needs to log u_L2 on the device (plan_native._ul2_from_path): one table for all coordinates."""
        if not self.ref_sol_is_defined:
            return None
        return dict(tables=[self.u], group_of_dim=[0] * self.d, xb=self.xb, dx=self.dx, delta_t=self.delta_t)

    def native_spec(self):
        return {
            'drift': (_nat.DRIFT_DOUBLE_WELL, self.kappa_.float().contiguous()),
            'sigma': (_nat.SIGMA_IDENTITY, None, 1.0),
            'runcost': (_nat.RUNCOST_ZERO, None),
            'term': (_nat.TERM_SHIFTED_QUAD, self.eta_.float().contiguous()),
        }


class DoubleWell_multidim(_DoubleWellBase):
    """Independent double-well potential in every coordinate, identity diffusion
    (reference problems.py:285-334)."""

    def __init__(self, name='Double well', d=1, d_1=1, d_2=0, T=1, eta=1, kappa=1, device=None):
        self.device = _resolve(device)
        self.name, self.T = name, T
        self._setup(d, d_1, d_2, eta, kappa)
        self.boundary, self.boundary_distance = 'unbounded', 2.0

    def h(self, t, x, y, z):
        return -0.5 * torch.sum(z ** 2, dim=1)

    def f(self, x, t):
        return torch.zeros(x.shape[0]).to(x.device)

    def g(self, x):
        return self._well_cost(x)

    # reference solution: the coordinates decouple -- one table for the first d_1 (kappa, eta), one for the others (1, 1)
    # (reference problems.py:336-476; methods on _DoubleWellBase).  The reference defines u_true on the class, where it fails until
    # both tables exist; here ``u_true`` appears with the tables, so a run without them logs no u_L2 instead of raising.
    def v_true(self, x, t):
        return None                                                      # problems.py:472-473

    def native_spec(self):
        return {
            'drift': (_nat.DRIFT_DOUBLE_WELL, self.kappa_.float().contiguous()),
            'sigma': (_nat.SIGMA_IDENTITY, None, 1.0),
            'runcost': (_nat.RUNCOST_ZERO, None),
            'term': (_nat.TERM_SHIFTED_QUAD, self.eta_.float().contiguous()),
        }


class DoubleWell_multidim_3(_DoubleWellBase):
    """DoubleWell_multidim with one (kappa, eta) for every coordinate (reference problems.py:730-840): one table for all."""

    def __init__(self, name='Double well', d=1, T=1, eta=1, kappa=1, device=None):
        self.device = _resolve(device)
        self.name, self.T = name, T
        self._setup(d, d, 0, eta, kappa)

    def grad_V(self, x):
        return 4.0 * self.kappa * (x * (x ** 2 - torch.ones(self.d).to(x.device)))

    def h(self, t, x, y, z):
        return -0.5 * torch.sum(z ** 2, dim=1)

    def f(self, x, t):
        return torch.zeros(x.shape[0]).to(x.device)

    def g(self, x):
        return (self.eta * (torch.sum((x - torch.ones(self.d).to(x.device)) ** 2, 1))).squeeze()

    def v_true(self, x, t):
        return None                                                      # problems.py:836-837

    def native_spec(self):
        return {
            'drift': (_nat.DRIFT_DOUBLE_WELL, self.kappa_.float().contiguous()),
            'sigma': (_nat.SIGMA_IDENTITY, None, 1.0),
            'runcost': (_nat.RUNCOST_ZERO, None),
            'term': (_nat.TERM_SHIFTED_QUAD, self.eta_.float().contiguous()),
        }


class DoubleWell_OU(_DoubleWellBase):
    """A double well in coordinate 0, Ornstein-Uhlenbeck in the others (reference problems.py:843-959):
    b = -[(4 kappa x_0)(x_0^2 - 1), a x_1, ..], a = 5;  g = alpha (x_0 - 1)^2 + gamma . x_{1:}.
    ``compute_reference_solution_x_1()`` tabulates the control of coordinate 0; the others have u*_i = -exp(a (t - T)) gamma_i."""

    def __init__(self, name='Double well', d=1, T=1, alpha=1, kappa=1, device=None):
        self.device = _resolve(device)
        self.name, self.d, self.T = name, d, T
        self.alpha, self.kappa = alpha, kappa
        self.gamma = torch.ones(d - 1, 1).to(self.device) * 1
        self.a = 5
        self.B = torch.eye(d).to(self.device)
        self.X_0 = torch.tensor([-1.0] + [0.0] * (d - 1)).to(self.device)
        self.ref_sol_is_defined = False

    def grad_V_1(self, x):
        return 4.0 * self.kappa * x * (x ** 2 - 1)

    def b(self, x):
        return -torch.cat([self.grad_V_1(x[:, 0]).unsqueeze(1), self.a * x[:, 1:]], 1)

    def f(self, x, t):
        return torch.zeros(x.shape[0]).to(x.device)

    def h(self, t, x, y, z):
        return -0.5 * torch.sum(z ** 2, dim=1)

    def g_1(self, x_1):
        return self.alpha * (x_1 - 1) ** 2

    def g(self, x):
        return self.alpha * (x[:, 0] - 1) ** 2 + torch.mm(x[:, 1:], self.gamma)[:, 0]

    def compute_reference_solution_x_1(self, delta_t=0.005, xb=2.5, nx=1000):
        grid, self.psi, self.u = self._fd_reference(self.V, self.g_1, delta_t, xb, nx)
        self._take_grid(grid)
        self.ref_sol_is_defined = True
        self.u_true = self._u_true

    def v_true_1(self, x, t):
        return self._table_read(self.psi, self._value_index(x), t, lambda p: -np.log(p))

    def v_true(self, x, t):
        return None                                                      # problems.py:954-955

    # (like DoubleWell_multidim: ``u_true`` appears with the table, so a run without it logs no u_L2 instead of raising)
    def _u_true(self, x, t):
        u_ou = -np.exp(self.a * (t - self.T)) * np.ones(x[:, 1:].shape) * self.gamma.cpu().numpy().T
        return np.concatenate([self.u_true_1(x[:, 0], t).T, u_ou], 1).T

    def u_true_tables(self):
        """The grid table of coordinate 0 plus, for the native plan's device-side u_L2 log, the coordinates whose u* does not depend
        on x: ``constant`` maps such a coordinate to a function t -> u*_i(t) (plan_common.ul2_reference tabulates it per step as a
        table that is constant along the cell axis)."""
        if not self.ref_sol_is_defined:
            return None
        gam = self.gamma.cpu().numpy()
        const = {i: (lambda t, i=i: (-np.exp(self.a * (t - self.T)) * np.ones((1, 1)) * gam[i - 1:i].T)[0, 0]) for i in range(1, self.d)}
        return dict(tables=[self.u], group_of_dim=[0] * self.d, xb=self.xb, dx=self.dx, delta_t=self.delta_t, constant=const)

    def native_spec(self):
        d = self.d
        return {
            'drift': (_nat.DRIFT_WELL_DIAG, torch.tensor([float(self.kappa)] + [-float(self.a)] * (d - 1))),
            'sigma': (_nat.SIGMA_IDENTITY, None, 1.0),
            'runcost': (_nat.RUNCOST_ZERO, None),
            'term': (_nat.TERM_QUAD_LINEAR, torch.cat([torch.tensor([float(self.alpha)]), self.gamma[:, 0].detach().cpu().float()])),
            'split': 1,
        }


class DoubleWell_multidim_2:
    """Radial double well (reference problems.py:691-727): b = -phi(r) x / r with r = |x|, phi = 4 kappa (r - 3)((r - 3)^2 - 1);
    g = alpha (r - 2)^2; X_0 = 1 / sqrt(d).  Its ``u_true`` returns zeros(x.shape), which the solver's u_L2 line cannot broadcast
    against the (d, K) control unless K = d -- as in the reference; pass u_l2_error_flag=False."""

    def __init__(self, name='Double well', d=1, T=1, alpha=1, kappa=1, device=None):
        self.device = _resolve(device)
        self.name, self.d, self.T = name, d, T
        self.alpha, self.kappa = alpha, kappa
        self.B = torch.eye(d).to(self.device)
        self.X_0 = (torch.ones(d) / torch.sqrt((torch.tensor(d).float()))).to(self.device)
        self.ref_sol_is_defined = False

    def V(self, x):
        return self.kappa * ((torch.sum(x ** 2, 1) - 3) ** 2 - 1) ** 2

    def grad_V(self, x):
        r = torch.sqrt(torch.sum(x ** 2, 1))
        return 4.0 * self.kappa * (r - 3).unsqueeze(1) * ((r - 3).unsqueeze(1) ** 2 - 1) * x / r.unsqueeze(1)

    def b(self, x):
        return -self.grad_V(x)

    def sigma(self, x):
        return self.B

    def h(self, t, x, y, z):
        return -0.5 * torch.sum(z ** 2, dim=1)

    def f(self, x, t):
        return torch.zeros(x.shape[0]).to(x.device)

    def g(self, x):
        return (self.alpha * (torch.sqrt(torch.sum(x ** 2, 1)) - 2) ** 2).squeeze()

    def v_true(self, x, t):
        return torch.zeros(x.shape)

    def u_true(self, x, t):
        return torch.zeros(x.shape)

    def native_spec(self):
        return {
            'drift': (_nat.DRIFT_RADIAL_WELL, torch.tensor([float(self.kappa), 3.0, 1.0])),
            'sigma': (_nat.SIGMA_IDENTITY, None, 1.0),
            'runcost': (_nat.RUNCOST_ZERO, None),
            'term': (_nat.TERM_RADIAL_QUAD, torch.tensor([float(self.alpha), 2.0])),
        }


class LLGC_general_f(_LinearDriftMixin):
    """LLGC dynamics with A = 0 and a running cost that is not quadratic in the control (reference problems.py:68-115):
    h = -(0.8 |z|^1.25 + x exp(T - t) - 0.8 exp(1.25 (T - t)))[:, 0].  No ``native_spec()``: the kernels' h is -|z|^2 / 2, so it
    runs on the composite plan.  (|z|^1.25 has no gradient at z = 0, where the reference's nets start: its own training is NaN
    from the second iteration.)"""

    def __init__(self, name='LLGC', d=1, off_diag=0, T=5, seed=42, device=None):
        self.device = _resolve(device)
        torch.manual_seed(seed)
        self.name, self.d, self.T = name, d, T
        self.A = 0 * (-torch.eye(d) + off_diag * torch.randn(d, d)).to(self.device)
        self.B = (torch.eye(d) + off_diag * torch.randn(d, d)).to(self.device)
        self.alpha = -torch.ones(d, 1).to(self.device)
        self.X_0 = torch.zeros(d).to(self.device)
        if not np.all(np.linalg.eigvals(self.A.cpu().numpy()) < 0):
            print('not all EV of A are negative')

    def f(self, x, t):
        return torch.zeros(x.shape[0])

    def h(self, t, x, y, z):
        return -(0.8 * ((- z) ** 2) ** (0.625) + x * torch.exp(self.T - t) - 0.8 * torch.exp(1.25 * (self.T - t)))[:, 0]

    def g(self, x):
        return torch.mm(x, self.alpha)[:, 0]

    def u_true(self, x, t):
        return -self.sigma(x).cpu().numpy().T.dot(expm(1 * self.B.cpu().numpy().T * (self.T - t)).dot(
            self.alpha.cpu().numpy()) * np.ones(x.shape).T)

    native_plan_reason = 'LLGC_general_f: h is not -|z|^2 / 2 (the running cost 0.8 |z|^1.25 is outside the native catalogue)'


class DoubleWell_multidim_for_general_solver(_DoubleWellBase):
    """Same dynamics posed as a parabolic terminal-value problem for GeneralSolver
    (reference problems.py:479-534): ``f(x)`` is the terminal condition."""

    def __init__(self, name='Double well', d=1, d_1=1, d_2=0, T=1, eta=1, kappa=1, modus='HJB', device=None):
        self.device = _resolve(device)
        self.name, self.T, self.modus = name, T, modus
        self._setup(d, d_1, d_2, eta, kappa)
        self.boundary, self.X_l, self.X_r = 'unbounded_square', -2.5, 2.5

    def h(self, t, x, y, z):
        if self.modus == 'linear':
            return torch.zeros(x.shape[0]).to(x.device)
        return -0.5 * torch.sum(z ** 2, dim=1)

    def f(self, x):
        if self.modus == 'linear':
            return torch.exp(-self._well_cost(x))
        return self._well_cost(x)

    def v_true(self, x, t):
        """Reference value from the per-coordinate tables (reference problems.py:682-685): the values add; in modus 'linear' the
        tabulated psi = exp(-v) multiply."""
        import numpy as np
        cols = np.array([self.v_true_1(x[:, i], t).squeeze() for i in range(self.d_1)]
                        + [self.v_true_2(x[:, i], t).squeeze() for i in range(self.d_1, self.d)])
        return np.prod(cols, 0) if self.modus == 'linear' else np.sum(cols, 0)

    def _publish_u_true(self):                                           # GeneralSolver never asks hasattr(problem, 'u_true')
        self.ref_sol_is_defined = self._tables_ready()

    def u_true(self, x, t):
        return self._u_true(x, t)                                        # problems.py:687-688

    def general_native_spec(self):
        return {'drift': (_nat.DRIFT_DOUBLE_WELL, self.kappa_.float().contiguous()), 'sigma_scale': 1.0,
                'h': _nat.GH_ZERO if self.modus == 'linear' else _nat.GH_QUAD}


class AllenCahn:
    """Allen-Cahn reaction term h = y - y^3, sigma = sqrt(2) I (reference problems.py:1175-1217,
    torch branch ``modus='pt'``)."""

    def __init__(self, name='Allen-Cahn', d=1, T=0.3, seed=42, modus='pt', device=None):
        self.device = _resolve(device)
        np.random.seed(seed)
        self.name, self.d, self.T, self.modus = name, d, T, modus
        self.B = np.eye(d) * np.sqrt(2)
        self.B_pt = torch.tensor(self.B).float().to(self.device)
        self.X_0 = np.zeros(d)
        self.sigma_modus, self.boundary, self.boundary_distance = 'constant', 'unbounded', 2.0

    def b(self, x):
        return torch.zeros(x.shape).to(x.device)

    def sigma(self, x):
        return self.B_pt

    def h(self, t, x, y, z):
        return y - y ** 3

    def f(self, x):
        return 1 / (2 + 2 / 5 * torch.sum(x ** 2, 1))

    def general_native_spec(self):
        return {'drift': (_nat.DRIFT_ZERO, None), 'sigma_scale': float(self.B_pt[0, 0]), 'h': _nat.GH_ALLEN_CAHN}


class HeatEquation:
    """Heat equation with terminal condition |x|^2 (reference problems.py:1733-1764)."""

    def __init__(self, name='Heat equation', d=1, T=1, seed=42, device=None):
        self.device = _resolve(device)
        torch.manual_seed(seed)
        self.name, self.d, self.T = name, d, T
        self.B = torch.sqrt(torch.tensor(2.0)) * torch.eye(d).to(self.device)
        self.boundary, self.boundary_type, self.boundary_distance = 'unbounded', 'Dirichlet', 1.0

    def b(self, x):
        return torch.zeros(x.shape).to(x.device)

    def sigma(self, x):
        return self.B

    def g(self, x, t):
        return torch.zeros(x.shape[0]).to(x.device)

    def h(self, t, x, y, z):
        return torch.zeros(x.shape[0]).to(x.device)

    def f(self, x):
        return torch.sum(x ** 2, 1)

    def general_native_spec(self):
        return {'drift': (_nat.DRIFT_ZERO, None), 'sigma_scale': float(self.B[0, 0]), 'h': _nat.GH_ZERO}

    def v_true(self, x, t):
        return torch.sum(x ** 2, 1) + 2 * (self.T - t) * self.d

    def native_vtrue_spec(self):
        """v_true as a closed form of the device test log (include/psp.h PSP_VTRUE_QUAD: |x|^2 + p0 (p1 - t))."""
        return {'kind': _nat.VTRUE_QUAD, 'par': (2.0 * self.d, float(self.T), 0.0, 0.0)}


# ---------------------------------------------------------------------------------------------
# bounded domains: the exponential-on-the-ball family and a box problem
# ---------------------------------------------------------------------------------------------
class _ExpBall:
    """v(x[,t]) = exp(alpha |x|^2 [+ t]) on the unit ball, b = 0, sigma = sqrt(2) I (reference problems.py:962-1172).
    ``_nl`` selects the nonlinearity of h: 'none' | 'sq' | 'sin'; ``_parabolic`` adds the time argument, the extra -y
    and the 2t in the exponent (ExponentialOnSphereNonlinearParabolic, :1166); ``_full`` makes the diffusion matrix the
    dense sqrt(2 / d) ones(d, d) -- a full second-order operator -- and with it the linear part of h carries
    (sum_i x_i)^2 = sum_ij x_i x_j where the others carry |x|^2 (ExponentialOnBallNonlinearSinHessian, :1067-1100)."""
    _nl, _parabolic, _full = 'none', False, False

    def _setup(self, name, d, alpha, boundary_type, device):
        self.device = _resolve(device)
        self.name, self.d, self.alpha = name, d, alpha
        if self._full:
            self.B = (torch.sqrt(torch.tensor(2.0) / d) * torch.ones(d, d)).to(self.device)
        else:
            self.B = (torch.sqrt(torch.tensor(2.0)) * torch.eye(d)).to(self.device)
        self.X_0 = torch.zeros(d).to(self.device)
        self.Y_0 = torch.zeros(1).to(self.device)
        self.boundary, self.boundary_distance = 'sphere', 1.0
        self.boundary_type = boundary_type

    def b(self, x):
        return torch.zeros(x.shape).to(x.device)

    def sigma(self, x):
        return self.B

    def _r2(self, x):
        return torch.sum(x ** 2, 1)

    def _h(self, x, y, t):
        al, d = self.alpha, self.d
        if self._nl == 'none':
            return -al * y * (al * 4 * self._r2(x) + 2 * d)
        lin = -2 * al * y * (al * 2 * (torch.sum(x, 1) ** 2 if self._full else self._r2(x)) + d)
        if self._parabolic:
            return lin - y + torch.sin(torch.exp(2 * al * self._r2(x) + 2 * t) - y ** 2)
        e = torch.exp(2 * al * self._r2(x))
        return lin + e - y ** 2 if self._nl == 'sq' else lin + torch.sin(e - y ** 2)

    def u_true(self, x):
        return -2 * torch.sqrt(torch.tensor(2.0)) * self.alpha * x * torch.exp(self.alpha * self._r2(x).unsqueeze(1))

    def general_native_spec(self):
        kind = {'none': _nat.GH_EXPBALL_LIN, 'sq': _nat.GH_EXPBALL_SQ, 'sin': _nat.GH_EXPBALL_SIN}[self._nl]
        par = 1.0 if self._parabolic else 0.0
        if self._full:                                   # a dense constant sigma: the matrix itself (plan_general_native.set_sigma)
            return {'drift': (_nat.DRIFT_ZERO, None), 'sigma': self.B, 'h': _nat.GH_EXPBALL_SIN_FULL,
                    'h_par': (float(self.alpha), float(self.d), par, par)}
        return {'drift': (_nat.DRIFT_ZERO, None), 'sigma_scale': float(self.B[0, 0]), 'h': kind,
                'h_par': (float(self.alpha), float(self.d), par, par)}

    def native_vtrue_spec(self):
        """v_true = exp(alpha |x|^2 [+ t]) as a closed form of the device test log (include/psp.h PSP_VTRUE_EXP)."""
        return {'kind': _nat.VTRUE_EXP, 'par': (float(self.alpha), 1.0 if self._parabolic else 0.0, 0.0, 0.0)}


class _ExpBallElliptic(_ExpBall):
    def f(self, x, t=None):
        return torch.zeros(x.shape[0]).to(x.device)

    def g(self, x):
        if self.boundary_type == 'Neumann':
            return 2 * self.alpha * x * torch.exp(self.alpha * self._r2(x)).unsqueeze(1)
        return torch.exp(self.alpha * self._r2(x))

    def h(self, x, y, z):
        return self._h(x, y, None)

    def v_true(self, x):
        return torch.exp(self.alpha * self._r2(x))


class ExponentialOnSphere(_ExpBallElliptic):
    """Linear elliptic problem (reference problems.py:962-993)."""

    def __init__(self, name='Exponential on sphere', d=2, alpha=1.0, device=None):
        self._setup(name, d, alpha, 'Dirichlet', device)


class ExponentialOnBallNonlinear(_ExpBallElliptic):
    """h carries exp(2 alpha |x|^2) - y^2 (reference problems.py:995-1029)."""
    _nl = 'sq'

    def __init__(self, name='Exponential on ball nonlinear', d=2, alpha=1.0, boundary_type='Dirichlet', device=None):
        self._setup(name, d, alpha, boundary_type, device)


class ExponentialOnBallNonlinearSin(_ExpBallElliptic):
    """h carries sin(exp(2 alpha |x|^2) - y^2) (reference problems.py:1031-1065)."""
    _nl = 'sin'

    def __init__(self, name='Exponential on ball nonlinear', d=2, alpha=1.0, boundary_type='Dirichlet', device=None):
        self._setup(name, d, alpha, boundary_type, device)


class ExponentialOnBallNonlinearSinHessian(_ExpBallElliptic):
    """The elliptic problem with a full Hessian (reference problems.py:1067-1100): sigma = sqrt(2 / d) ones(d, d), so the
    operator is sum_ij d_i d_j v, and h carries sum_ij x_i x_j in its linear part; same solution exp(alpha |x|^2)."""
    _nl, _full = 'sin', True

    def __init__(self, name='Exponential on ball nonlinear', d=2, alpha=1.0, boundary_type='Dirichlet', device=None):
        self._setup(name, d, alpha, boundary_type, device)


class ExponentialOnSphereNonlinearParabolic(_ExpBall):
    """Parabolic version for GeneralSolver (reference problems.py:1137-1172); ``boundary_type`` is 'Dirichlet' and the
    Neumann notebook sets it to 'Neumann' on the instance."""
    _nl, _parabolic = 'sin', True

    def __init__(self, name='Exponential on ball', d=2, T=1.0, alpha=1.0, device=None):
        self._setup(name, d, alpha, 'Dirichlet', device)
        self.T = T

    def f(self, x):
        return torch.exp(self.alpha * self._r2(x) + self.T)

    def g(self, x, t):
        if self.boundary_type == 'Neumann':
            return 2 * self.alpha * x * torch.exp(self.alpha * self._r2(x) + t).unsqueeze(1)
        return torch.exp(self.alpha * self._r2(x) + t)

    def h(self, t, x, y, z):
        return self._h(x, y, t)

    def v_true(self, x, t):
        return torch.exp(self.alpha * self._r2(x) + t)


class ExponentialOnSphereParabolic(_ExpBall):
    """The linear parabolic problem (reference problems.py:1103-1134): h = -y (2 alpha (2 alpha |x|^2 + d) + 1), Dirichlet
    data exp(alpha |x|^2 + t).  As in the reference the class sets no ``boundary_type``: GeneralSolver reads it from the problem,
    and the Neumann notebook sets it on the instance.  Native: PSP_GH_EXPBALL_LIN with e = 1."""
    _parabolic = True

    def __init__(self, name='Exponential on sphere', d=2, T=1.0, alpha=1.0, device=None):
        self._setup(name, d, alpha, None, device)
        del self.boundary_type
        self.T = T

    def f(self, x):
        return torch.exp(self.alpha * self._r2(x) + self.T)

    def g(self, x, t):
        return torch.exp(self.alpha * self._r2(x) + t)

    def h(self, t, x, y, z):
        return -y * (2 * self.alpha * (self.alpha * 2 * self._r2(x) + self.d) + 1)

    def v_true(self, x, t):
        return torch.exp(self.alpha * self._r2(x) + t)

    def general_native_spec(self):
        return {'drift': (_nat.DRIFT_ZERO, None), 'sigma_scale': float(self.B[0, 0]), 'h': _nat.GH_EXPBALL_LIN,
                'h_par': (float(self.alpha), float(self.d), 1.0, 0.0)}


class Committor:
    """Committor function between two concentric spheres of radius a = 1 and c = 2 (reference problems.py:1546-1579): b = 0,
    sigma = I, h = 0, boundary data 0 on the inner and 1 on the outer sphere; ``boundary = 'two_spheres'`` (EllipticSolver:
    the batch size changes with the rejection step of every iteration; native: PSP_DOM_ANNULUS)."""

    def __init__(self, name='Committor', d=2, alpha=1.0, device=None):
        self.device = _resolve(device)
        self.name, self.d = name, d
        self.a, self.c = 1.0, 2.0
        self.B = torch.eye(d).to(self.device)
        self.X_0 = torch.zeros(d).to(self.device)
        self.Y_0 = torch.zeros(1).to(self.device)
        self.boundary = 'two_spheres'
        self.boundary_distance_1, self.boundary_distance_2 = self.a, self.c

    def b(self, x):
        return torch.zeros(x.shape).to(x.device)

    def sigma(self, x):
        return self.B

    def f(self, x):
        return torch.zeros(x.shape[0]).to(x.device)

    def g(self, x):
        return (torch.sqrt(torch.sum(x ** 2, 1)) > self.a).float()

    def h(self, x, y, z):
        return torch.zeros(x.shape[0]).to(x.device)

    def u_true(self, x):
        return torch.zeros(x.shape)

    def v_true(self, x):
        r = torch.sqrt(torch.sum(x ** 2, 1))
        return (self.a ** 2 - r ** (2 - self.d) * self.a ** self.d) / (self.a ** 2 - self.c ** (2 - self.d) * self.a ** self.d)

    def native_vtrue_spec(self):
        """v_true as a closed form of the device test log (include/psp.h PSP_VTRUE_COMMITTOR: a, c, d)."""
        return {'kind': _nat.VTRUE_COMMITTOR, 'par': (float(self.a), float(self.c), float(self.d), 0.0)}

    def general_native_spec(self):
        return {'drift': (_nat.DRIFT_ZERO, None), 'sigma_scale': 1.0, 'h': _nat.GH_ZERO}


class QuadraticOnBox:
    """NOT a reference class: b = 0, sigma = scale I, h = -|z|^2/2 (or 0) with data |x|^2 on the box [X_l, X_r]^d.
    It exercises the 'square' exit tests of the solvers (reference solver.py:1125-1129, :762-767) with coefficients
    the kernels have; ``parabolic`` selects the GeneralSolver (h(t,x,y,z), f(x), g(x,t)) or the EllipticSolver
    (h(x,y,z), g(x)) calling convention.  ``B`` (optional, d x d) replaces scale I by a dense constant diffusion matrix."""

    def __init__(self, name='Quadratic on box', d=2, T=0.5, X_l=-1.0, X_r=1.0, one_boundary=False, scale=1.0,
                 parabolic=True, quad_h=True, device=None, B=None):
        self.device = _resolve(device)
        self.name, self.d, self.T = name, d, T
        self.dense_B = B is not None
        if self.dense_B:
            self.B = torch.as_tensor(B, dtype=torch.float32).reshape(d, d).clone().to(self.device)
        else:
            self.B = (scale * torch.eye(d)).to(self.device)
        self.boundary, self.boundary_type = 'square', 'Dirichlet'
        self.X_l, self.X_r, self.one_boundary = X_l, X_r, one_boundary
        self.parabolic, self.quad_h = parabolic, quad_h

    def b(self, x):
        return torch.zeros(x.shape).to(x.device)

    def sigma(self, x):
        return self.B

    def h(self, *args):
        z = args[-1]
        return -0.5 * torch.sum(z ** 2, dim=1) if self.quad_h else torch.zeros(z.shape[0]).to(z.device)

    def f(self, x, t=None):
        return torch.sum(x ** 2, 1) if self.parabolic else torch.zeros(x.shape[0]).to(x.device)

    def g(self, x, t=None):
        return torch.sum(x ** 2, 1) + (self.T - t) if self.parabolic else torch.sum(x ** 2, 1)

    def v_true(self, x, t=None):
        return torch.sum(x ** 2, 1)

    def native_vtrue_spec(self):
        """v_true = |x|^2 as a closed form of the device test log (include/psp.h PSP_VTRUE_QUAD with p0 = 0)."""
        return {'kind': _nat.VTRUE_QUAD, 'par': (0.0, 0.0, 0.0, 0.0)}

    def general_native_spec(self):
        h = _nat.GH_QUAD if self.quad_h else _nat.GH_ZERO
        if self.dense_B:
            return {'drift': (_nat.DRIFT_ZERO, None), 'sigma': self.B, 'h': h}
        return {'drift': (_nat.DRIFT_ZERO, None), 'sigma_scale': float(self.B[0, 0]), 'h': h}


# ---------------------------------------------------------------------------------------------
# exit-time and box-domain problems of the diffusion-loss paper (reference problems.py:1220-1730)
# ---------------------------------------------------------------------------------------------
class _ExitDoubleWell:
    """One-dimensional double well V = beta (x^2 - 1)^2 started in the left well, stopped at X_r (EllipticSolver on the box
    [X_l, X_r] with ``one_boundary``): b = -grad V, sigma = eta I.  ``compute_reference_solution()`` solves the stationary
    problem L psi - f psi = rhs by finite differences on [-2, 2] with psi pinned on a band of grid rows right of X_r; ``v_true``
    reads the table by the reference's index arithmetic (floor((x + 2) / dx), clamped at ``_clamp_hi``)."""
    _f_rate = 1            # the zeroth-order coefficient of the tabulated problem
    _rhs = 0.0             # right-hand side away from the pinned rows
    _pinned = 1.0          # psi on the pinned rows

    def _setup(self, name, d, beta, eta, device):
        self.device = _resolve(device)
        self.name, self.d, self.beta = name, d, beta
        self.B = (torch.eye(d).to(self.device) if eta is None else eta * torch.eye(d).to(self.device))
        self.X_0 = -torch.ones(d).to(self.device)
        self.Y_0 = -torch.zeros(d).to(self.device)
        self.boundary, self.one_boundary = 'square', True
        self.X_l, self.X_r = -2.0, 1.0
        if d != 1:
            print('The double well example is only implemented for d = 1.')

    def _pinned_rows(self):
        return 300, 310

    def compute_reference_solution(self):
        f = self._f_rate
        sigma = self.B[0, 0].cpu().numpy()
        self.xr = [-2, 2]
        dx = self.dx
        Nx = int(np.ceil((self.xr[1] - self.xr[0]) / dx))
        x_val = np.linspace(self.xr[0], self.xr[1], Nx)
        gV = self.grad_V
        L = np.zeros([Nx, Nx])
        L[0, 0] = - 2 * sigma**2 / 2 / dx**2 - gV(x_val[0]) / dx - f
        L[0, 1] = sigma**2 / dx
        L[Nx - 1, Nx - 2] = sigma**2 / 2 / dx**2 + gV(x_val[Nx - 1]) / dx
        L[Nx - 1, Nx - 1] = - sigma**2 / dx**2 - sigma * gV(x_val[Nx - 1]) / dx - f
        for i in range(1, Nx - 1):
            L[i, i - 1] = sigma**2 / 2 / dx**2 + gV(x_val[i]) / dx
            L[i, i] = - sigma**2 / dx**2 - gV(x_val[i]) / dx - f
            L[i, i + 1] = sigma**2 / 2 / dx**2
        rhs = np.zeros(Nx) + self._rhs
        lo, hi = self._pinned_rows()                       # the boundary value on several rows, for numerical stability
        L[lo:hi, :] = 0
        for i in range(lo, hi):
            L[i, i] = 1
        rhs[lo:hi] = self._pinned
        L[0, :] = 0                                        # psi flat at both ends of the grid
        L[0, 0], L[0, 1], rhs[0] = 1, -1, 0
        L[Nx - 1, :] = 0
        L[Nx - 1, Nx - 1], L[Nx - 1, Nx - 2], rhs[Nx - 1] = 1, -1, 0
        self.psi = np.linalg.solve(L, rhs)
        self.u = sigma * (- np.log(self.psi[:-1]) + np.log(self.psi[1:])) / dx

    def V(self, x):
        return self.beta * (x**2 - 1)**2

    def grad_V(self, x):
        return 4.0 * self.beta * x * (x**2 - 1)

    def b(self, x):
        return -self.grad_V(x)

    def sigma(self, x):
        return self.B

    def _clamp_hi(self):
        return 298

    def _index(self, x):
        return torch.clamp(torch.floor((x + self.xr[1]) / self.dx).long(), 0, self._clamp_hi()).view(-1)

    def _read(self, table, x):
        """table[i(x)] as a (1, len) float64 tensor on x's device (the reference returns the same numbers as a numpy array)."""
        i = self._index(x.detach().squeeze())
        return torch.as_tensor(np.asarray(table), device=x.device)[i].reshape(1, len(i))

    def u_true(self, x, t):
        i = self._index(x.detach().cpu().squeeze(0))
        return np.array(self.u[i.numpy()]).reshape([1, len(i)])

    def _spec(self, p):
        return {'drift': (_nat.DRIFT_DOUBLE_WELL, (self.beta * torch.ones(self.d)).float().contiguous()), 'dwell_form': 1,
                'sigma_scale': float(self.B[0, 0]), 'h': _nat.GH_AFFINE_EXP, 'h_par': p}


class DoubleWell_stopping(_ExitDoubleWell):
    """Exit from the left well with the quadratic control cost (reference problems.py:1220-1309): h = -|z|^2 / 2 + 1, data 0;
    ``v_true`` = -log psi of the tabulated linear problem."""

    def __init__(self, name='Double well', d=1, beta=1, device=None):
        self._setup(name, d, beta, None, device)
        self.dx = 0.01

    def f(self, x):
        return torch.ones(x.shape[0]).to(x.device)

    def g(self, x):
        return torch.zeros(x.shape[0]).to(x.device)

    def h(self, x, y, z):
        return -0.5 * torch.sum(z**2, dim=1) + self.f(x)

    def v_true(self, x):
        return self._read(-np.log(self.psi), x)

    def general_native_spec(self):
        return self._spec((1.0, 0.0, -0.5, 0.0))


class DoubleWell_stopping_linear(_ExitDoubleWell):
    """The same exit problem in its linear form (reference problems.py:1312-1401): h = -y, data 1; ``v_true`` = psi."""

    def __init__(self, name='Double well', d=1, beta=1, device=None):
        self._setup(name, d, beta, None, device)
        self.dx = 0.01

    def f(self, x):
        return torch.ones(x.shape[0]).to(x.device)

    def g(self, x):
        return torch.ones(x.shape[0]).to(x.device)

    def h(self, x, y, z):
        return -self.f(x) * y

    def v_true(self, x):
        return self._read(self.psi, x)

    def general_native_spec(self):
        return self._spec((0.0, -1.0, 0.0, 0.0))


class DoubleWell_expectation_hitting_time(_ExitDoubleWell):
    """Mean hitting time of X_r from the left well (reference problems.py:1404-1496): sigma = eta I, h = 1, data 0; the table
    solves L psi = -1 with psi = 0 on the rows index_r .. 1.1 index_r, and ``v_true`` clamps its index at index_r."""
    _f_rate, _rhs, _pinned = 0, -1.0, 0.0

    def __init__(self, name='Double well', d=1, beta=1, dx=0.01, eta=2.0, device=None):
        self._setup(name, d, beta, eta, device)
        self.dx = dx

    def _index_r(self):
        return int((self.X_r - self.X_l) / self.dx)

    def _pinned_rows(self):
        return self._index_r(), int(self._index_r() * 1.1)

    def _clamp_hi(self):
        return self._index_r()

    def f(self, x):
        return torch.zeros(x.shape[0]).to(x.device)

    def g(self, x):
        return torch.zeros(x.shape[0]).to(x.device)

    def h(self, x, y, z):
        return torch.ones(y.shape[0]).to(y.device)

    def u_true(self, x):
        return x

    def v_true(self, x):
        return self._read(self.psi, x)

    def general_native_spec(self):
        return self._spec((1.0, 0.0, 0.0, 0.0))


class Committor_DoubleWell:
    """Committor of the one-dimensional double well between X_l and X_r = 0 (reference problems.py:1499-1543).  Ported as a class
    only: the reference writes ``sigma(x, t)`` and ``h(x, t, y, z)``, which is the calling convention of neither GeneralSolver
    (``sigma(x)``, ``h(t, x, y, z)``) nor EllipticSolver (``h(x, y, z)``), so no solver of the reference runs it; it has no
    ``general_native_spec()`` and no ``native_vtrue_spec()``."""

    def __init__(self, name='Double well', d=1, beta=1, dx=0.01, eta=2.0, T=1.0, device=None):
        self.device = _resolve(device)
        self.name, self.T, self.d, self.beta, self.dx = name, T, d, beta, dx
        self.B = np.sqrt(eta) * torch.eye(d).to(self.device)
        self.X_0 = -torch.ones(d).to(self.device)
        self.Y_0 = -torch.zeros(d).to(self.device)
        self.boundary, self.one_boundary, self.boundary_type = 'square', True, 'Dirichlet'
        self.X_l, self.X_r = -2.0, 0.0
        if d != 1:
            print('The double well example is only implemented for d = 1.')

    def V(self, x):
        return self.beta * (x**2 - 1)**2

    def grad_V(self, x):
        return 4.0 * self.beta * x * (x**2 - 1)

    def b(self, x):
        return -self.grad_V(x)

    def sigma(self, x, t):
        return self.B

    def f(self, x):
        return torch.zeros(x.shape[0]).to(x.device)

    def g(self, x, t):
        return torch.ones(x.shape[0]).to(x.device)

    def h(self, x, t, y, z):
        return torch.zeros(y.shape[0]).to(y.device)

    def u_true(self, x, t):
        return torch.zeros(x.shape[0]).to(x.device)

    def v_true(self, x, t):
        return torch.zeros(x.shape[0]).to(x.device)


class _ZeroDriftElliptic:
    """b = 0, f = 0, constant sigma, a control reference that is zero: what the four closed-form elliptic problems share."""

    def _setup(self, name, d, B, device):
        self.device = _resolve(device)
        self.name, self.d = name, d
        self.B = B.to(self.device)
        self.X_0 = -torch.ones(d).to(self.device)
        self.Y_0 = -torch.zeros(d).to(self.device)
        self.pi = torch.tensor(np.pi)

    def b(self, x):
        return torch.zeros(x.shape).to(x.device)

    def sigma(self, x):
        return self.B

    def f(self, x):
        return torch.zeros(x.shape[0]).to(x.device)

    def u_true(self, x, t):
        return torch.zeros(x.shape[0], 1).to(x.device)


class QuadraticGradient(_ZeroDriftElliptic):
    """v = log((|x|^2 + 1) / d) on the ball of radius r (reference problems.py:1582-1611): sigma = sqrt(2) I,
    h = |z|^2 / B_00^2 - 2 exp(-y)."""

    def __init__(self, name='Quadratic Gradient', d=1, r=1.0, device=None):
        self._setup(name, d, torch.sqrt(torch.tensor(2.0)) * torch.eye(d), device)
        self.boundary, self.boundary_distance = 'sphere', r

    def g(self, x):
        return torch.log((torch.sum(x**2, 1) + 1) / self.d)

    def h(self, x, y, z):
        return torch.sum(z**2, dim=1) / self.B[0, 0]**2 - 2 * torch.exp(-y)

    def v_true(self, x):
        return torch.log((torch.sum(x**2, 1) + 1) / self.d)

    def general_native_spec(self):
        return {'drift': (_nat.DRIFT_ZERO, None), 'sigma_scale': float(self.B[0, 0]), 'h': _nat.GH_AFFINE_EXP,
                'h_par': (0.0, 0.0, 1.0 / float(self.B[0, 0]**2), -2.0)}

    def native_vtrue_spec(self):
        """v_true as a closed form of the device test log (include/psp.h PSP_VTRUE_LOGQ: log((|x|^2 + 1) / p0))."""
        return {'kind': _nat.VTRUE_LOGQ, 'par': (float(self.d), 0.0, 0.0, 0.0)}


class Helmholtz(_ZeroDriftElliptic):
    """Helmholtz equation on the square [-1, 1]^2 with the solution sin(a_1 pi x_0) sin(a_2 pi x_1) (reference
    problems.py:1614-1654); ``a_1``, ``a_2``, ``k`` are attributes the notebooks change on the instance."""

    def __init__(self, name='Helmholtz', d=2, r=1.0, device=None):
        self._setup(name, d, torch.sqrt(torch.tensor(2.0)) * torch.eye(d), device)
        self.a_1, self.a_2, self.k = 1.0, 4.0, 1.0
        self.boundary, self.one_boundary, self.X_l, self.X_r = 'square', False, -1.0, 1.0
        if d != 2:
            print('Only implemented for d = 2.')

    def _s(self, x):
        pi = self.pi.to(x.device)
        return torch.sin(self.a_1 * pi * x[:, 0]) * torch.sin(self.a_2 * pi * x[:, 1])

    def g(self, x):
        return self._s(x)

    def h(self, x, y, z):
        pi = self.pi.to(x.device)
        s1, s2 = torch.sin(self.a_1 * pi * x[:, 0]), torch.sin(self.a_2 * pi * x[:, 1])
        return (self.k**2 * y + (self.a_1 * pi)**2 * s1 * s2 + (self.a_2 * pi)**2 * s1 * s2 - self.k**2 * s1 * s2)

    def v_true(self, x):
        return self._s(x)

    def general_native_spec(self):
        """PSP_GH_SINE_SOURCE, sub-mode 0: h_par = (0, a_1 pi, a_2 pi, k^2), the products rounded to fp32 as ``h`` forms them."""
        return {'drift': (_nat.DRIFT_ZERO, None), 'sigma_scale': float(self.B[0, 0]), 'h': _nat.GH_SINE_SOURCE,
                'h_par': (0.0, float(self.a_1 * self.pi), float(self.a_2 * self.pi), float(self.k ** 2))}

    def native_vtrue_spec(self):
        """v_true as a closed form of the device test log (include/psp.h PSP_VTRUE_SINPROD: sin(p0 x_0) sin(p1 x_1))."""
        return {'kind': _nat.VTRUE_SINPROD, 'par': (float(self.a_1 * self.pi), float(self.a_2 * self.pi), 0.0, 0.0)}


class Oscillations(_ZeroDriftElliptic):
    """Two-scale oscillation on [0, 1]: v = sin(2 pi x) + 0.1 sin(a pi x), h the matching source (reference
    problems.py:1657-1693); ``a`` is an attribute the notebooks change on the instance."""

    def __init__(self, name='Oscillations', d=1, r=1.0, device=None):
        self._setup(name, d, torch.sqrt(torch.tensor(2.0)) * torch.eye(d), device)
        self.a = 5
        self.boundary, self.one_boundary, self.X_l, self.X_r = 'square', False, 0.0, 1.0
        if d != 1:
            print('Only implemented for d = 1.')

    def g(self, x):
        return torch.zeros(x.shape[0]).to(x.device)

    def h(self, x, y, z):
        pi = self.pi.to(x.device)
        return (2 * pi)**2 * torch.sin(2 * pi * x[:, 0]) + (self.a * pi)**2 * 0.1 * torch.sin(self.a * pi * x[:, 0])

    def v_true(self, x):
        pi = self.pi.to(x.device)
        return torch.sin(2 * pi * x[:, 0]) + 0.1 * torch.sin(self.a * pi * x[:, 0])

    def general_native_spec(self):
        """PSP_GH_SINE_SOURCE, sub-mode 1: h_par = (1, 2 pi, a pi, 0.1)."""
        return {'drift': (_nat.DRIFT_ZERO, None), 'sigma_scale': float(self.B[0, 0]), 'h': _nat.GH_SINE_SOURCE,
                'h_par': (1.0, float(2 * self.pi), float(self.a * self.pi), 0.1)}

    def native_vtrue_spec(self):
        """v_true as a closed form of the device test log (include/psp.h PSP_VTRUE_SINSUM: sin(p0 x_0) + p2 sin(p1 x_0))."""
        return {'kind': _nat.VTRUE_SINSUM, 'par': (float(2 * self.pi), float(self.a * self.pi), 0.1, 0.0)}


class SinNorm2(_ZeroDriftElliptic):
    """v = sin(pi |x|^2) on the unit ball under the dense sigma = alpha sqrt(2 / d) ones(d, d) (reference problems.py:1696-1730):
    the operator is alpha^2 sum_ij d_i d_j, so h carries (sum_i x_i)^2; ``linear`` selects the source-only h or the one that
    reads y."""

    def __init__(self, name='SinNorm2', d=1, r=1.0, linear=True, alpha=1.0, device=None):
        self.alpha = alpha
        self._setup(name, d, alpha * torch.sqrt(torch.tensor(2.0) / d) * torch.ones(d, d), device)
        self.linear = linear
        self.boundary, self.boundary_distance = 'sphere', 1.0

    def g(self, x):
        return torch.zeros(x.shape[0]).to(x.device)

    def h(self, x, y, z):
        pi = self.pi.to(x.device)
        rr, sx = torch.sum(x**2, 1), torch.sum(x, 1)
        if self.linear:
            return self.alpha**2 * (4 * pi**2 * torch.sin(pi * rr) * sx**2 - 2 * self.d * pi * torch.cos(pi * rr))
        return self.alpha**2 * (4 * pi**2 * y * sx**2 - 2 * self.d * pi * torch.cos(pi * rr) + torch.sin(pi * rr)**2 - y**2)

    def v_true(self, x):
        return torch.sin(self.pi.to(x.device) * torch.sum(x**2, 1))

    def general_native_spec(self):
        """PSP_GH_SINNORM2 with the dense B (psp_genl_* only): h_par = (alpha, d, linear, 0)."""
        return {'drift': (_nat.DRIFT_ZERO, None), 'sigma': self.B, 'h': _nat.GH_SINNORM2,
                'h_par': (float(self.alpha), float(self.d), 1.0 if self.linear else 0.0, 0.0)}

    def native_vtrue_spec(self):
        """v_true as a closed form of the device test log (include/psp.h PSP_VTRUE_SINR2: sin(pi |x|^2))."""
        return {'kind': _nat.VTRUE_SINR2, 'par': (0.0, 0.0, 0.0, 0.0)}


class _EigenvalueOnBox:
    """What the eigenvalue problems of the diffusion-loss notebooks share (`Eigenvalue - *.ipynb`): the periodic box
    [0, 2 pi]^d, sigma = sqrt(2) I, the centre X_0 = pi 1, zero boundary data (the notebooks use periodic terms instead)."""

    def _setup(self, name, d, device):
        self.device = _resolve(device)
        self.name, self.d = name, d
        self.B = (torch.sqrt(torch.tensor(2.0)) * torch.eye(d)).to(self.device)
        self.X_0 = (torch.tensor(np.pi) * torch.ones(d)).to(self.device)
        self.Y_0 = torch.zeros(1).to(self.device)
        self.X_l, self.X_r = 0.0, 2 * np.pi
        self.boundary, self.one_boundary = 'square', False

    def sigma(self, x):
        return self.B

    def g(self, x):
        return torch.zeros(x.shape[0]).to(x.device)


class FokkerPlanckEigenvalue(_EigenvalueOnBox):
    """The Fokker-Planck eigenvalue problem of `Eigenvalue - Fokker-Planck.ipynb`: with c = 0.1 1 and S(x) = sum_j c_j cos x_j,
    b = -cos(S) c sin x, h = y (-sin(S) sum_i c_i^2 sin^2 x_i - cos(S) S); eigenfunction exp(-sin S), eigenvalue 0."""

    def __init__(self, name='Eigenvalue', d=1, device=None):
        self._setup(name, d, device)
        self.c = (0.1 * torch.ones(1, d)).to(self.device)
        self.lambda_ = 0.0

    def b(self, x):
        c = self.c.to(x.device)
        return -torch.cos(torch.sum(c * torch.cos(x), 1)).unsqueeze(1) * c * torch.sin(x)

    def h(self, x, y, z):
        c = self.c.to(x.device)
        S = torch.sum(c * torch.cos(x), 1)
        return y * (-torch.sum(c**2 * torch.sin(x)**2, 1) * torch.sin(S) - torch.cos(S) * S)

    def v_true(self, x):
        return torch.exp(-torch.sin(torch.sum(self.c.to(x.device) * torch.cos(x), 1)))

    def general_native_spec(self):
        """PSP_DRIFT_EIG_FP / PSP_GH_EIG_FP (psp_genl_*_eig only): both read the vector c."""
        return {'drift': (_nat.DRIFT_EIG_FP, self.c.reshape(-1).float().contiguous()), 'sigma_scale': float(self.B[0, 0]),
                'h': _nat.GH_EIG_FP, 'h_par': (0.0, float(self.d), 0.0, 0.0)}


class SchroedingerEigenvalue(_EigenvalueOnBox):
    """The nonlinear Schroedinger eigenvalue problem of `Eigenvalue - nonlinear Schroedinger equation, d = *.ipynb`: b = 0,
    h = -y^3 - y (-exp((2 / d) sum cos x_i) / c^2 + sum (sin^2 x_i / d^2 - cos x_i / d) - 3) with the normalising constant
    c = sqrt((int_0^{2 pi} exp((2 / d) cos x) dx)^d / (2 pi)^d) formed by quadrature as the notebook's first cell does;
    eigenfunction exp((1 / d) sum cos x_i) / c, eigenvalue -3."""

    def __init__(self, name='Eigenvalue', d=1, device=None):
        from scipy import integrate
        self._setup(name, d, device)
        self.c = float(np.sqrt(integrate.quad(lambda x: np.exp(2 / d * np.cos(x)), 0, 2 * np.pi)[0]**d / (2 * np.pi)**d))
        self.lambda_ = -3.0

    def b(self, x):
        return torch.zeros(x.shape).to(x.device)

    def h(self, x, y, z):
        return -y**3 - y * (-1 / self.c**2 * torch.exp(2 / self.d * torch.sum(torch.cos(x), 1))
                            + torch.sum((torch.sin(x)**2 / self.d**2 - torch.cos(x) / self.d), 1) - 3)

    def v_true(self, x):
        return 1 / self.c * torch.exp(1 / self.d * torch.sum(torch.cos(x), 1))

    def general_native_spec(self):
        """PSP_GH_EIG_NLS (psp_genl_*_eig only): h_par = (1 / c^2, d, -, -)."""
        return {'drift': (_nat.DRIFT_ZERO, None), 'sigma_scale': float(self.B[0, 0]), 'h': _nat.GH_EIG_NLS,
                'h_par': (1.0 / self.c**2, float(self.d), 0.0, 0.0)}
