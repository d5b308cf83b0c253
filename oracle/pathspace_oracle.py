"""CPU oracle for the path-space hot path -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A plain torch-CPU restatement of the reference algorithm
(lorenzrichter/path-space-PDE-solver: solver.py / problems.py / function_space.py),
written as flat functions, each citing the reference lines it follows.  It is used
ONLY by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg as the
checker; nothing under path-space-pde-solver_amd/ imports it.

Pinning: tests/test_oracle_golden.py checks this file bit-for-bit (same torch build,
CPU) against tests/golden/*.json, which were produced by importing and running the
reference itself (tests/golden/make_golden.py).  Arithmetic is torch ATen fp32, the
same library the reference calls; the reference pins no torch version, so parity is
pinned against torch 2.10.0 as installed in the image.

Everything is fp32 on CPU; noise comes from torch's global CPU generator in exactly
the reference's draw order unless a ``noise`` tensor is supplied.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

CPU = torch.device("cpu")


# --------------------------------------------------------------------------------------
# problems  (reference problems.py)
# --------------------------------------------------------------------------------------
@dataclass
class OracleProblem:
    kind: str
    d: int
    T: float
    X_0: torch.Tensor
    B: torch.Tensor
    b: Callable
    sigma: Callable
    h: Callable
    f: Callable
    g: Optional[Callable] = None
    extra: Dict = field(default_factory=dict)


def problem_llgc(d=1, off_diag=0.0, T=5, seed=42) -> OracleProblem:
    """Ornstein-Uhlenbeck, linear terminal cost.  problems.py:14-49."""
    torch.manual_seed(seed)                                          # :20
    A = -torch.eye(d) + off_diag * torch.randn(d, d)                 # :24
    B = torch.eye(d) + off_diag * torch.randn(d, d)                  # :25
    alpha = torch.ones(d, 1)                                         # :26
    return OracleProblem(
        kind="LLGC", d=d, T=T, X_0=torch.zeros(d), B=B,
        b=lambda x: torch.mm(A, x.t()).t(),                          # :37
        sigma=lambda x: B,                                           # :40
        h=lambda t, x, y, z: -0.5 * torch.sum(z ** 2, dim=1),        # :46
        f=lambda x, t: torch.zeros(x.shape[0]),                      # :43
        g=lambda x: torch.mm(x, alpha)[:, 0],                        # :49
        extra=dict(A=A, alpha=alpha))


def problem_lqgc(d=1, off_diag=0.0, T=5, seed=42, delta_t=0.05) -> OracleProblem:
    """Linear-quadratic Gaussian control.  problems.py:118-167."""
    torch.manual_seed(seed)                                          # :124
    A = -torch.eye(d) + off_diag * torch.randn(d, d)                 # :128
    B = torch.eye(d) + off_diag * torch.randn(d, d)                  # :129
    P = 0.5 * torch.eye(d)                                           # :137
    R = torch.eye(d)                                                 # :139
    f = lambda x, t: torch.sum(x.t() * torch.mm(P, x.t()), 0)        # :161
    return OracleProblem(
        kind="LQGC", d=d, T=T, X_0=torch.zeros(d), B=B,
        b=lambda x: torch.mm(A, x.t()).t(),                          # :155
        sigma=lambda x: B,                                           # :158
        h=lambda t, x, y, z: -0.5 * torch.sum(z ** 2, dim=1) - f(x, t),   # :167
        f=f,
        g=lambda x: torch.sum(x.t() * torch.mm(R, x.t()), 0),        # :164
        extra=dict(A=A, P=P, R=R))


def _double_well_parts(d, d_1, d_2, eta, kappa):
    eta_ = torch.tensor([eta] * d_1 + [1.0] * d_2)                   # problems.py:296 / :490
    kappa_ = torch.tensor([kappa] * d_1 + [1.0] * d_2)               # :298 / :492
    ones = torch.ones(d)
    grad_V = lambda x: 4.0 * kappa_ * (x * (x ** 2 - ones))          # :312 / :507
    cost = lambda x: (torch.sum(eta_ * (x - ones) ** 2, 1)).squeeze()   # :334 / :534
    return eta_, kappa_, grad_V, cost


def problem_double_well(d=1, d_1=1, d_2=0, T=1, eta=1, kappa=1) -> OracleProblem:
    """problems.py:285-334 (DoubleWell_multidim)."""
    eta_, kappa_, grad_V, cost = _double_well_parts(d, d_1, d_2, eta, kappa)
    B = torch.eye(d)                                                 # :299
    return OracleProblem(
        kind="DoubleWell_multidim", d=d, T=T, X_0=-torch.ones(d), B=B,      # :300
        b=lambda x: -grad_V(x),                                      # :315
        sigma=lambda x: B,                                           # :318
        h=lambda t, x, y, z: -0.5 * torch.sum(z ** 2, dim=1),        # :321
        f=lambda x, t: torch.zeros(x.shape[0]),                      # :324
        g=cost, extra=dict(eta_=eta_, kappa_=kappa_))


def problem_double_well_1d(d=1, T=1, eta=1, kappa=1) -> OracleProblem:
    """problems.py:178-213 (DoubleWell, one-dimensional): the dynamics of the multidimensional class at d = 1, with the products
    of grad V taken in the order written there."""
    B = torch.eye(d)                                                 # :188
    return OracleProblem(
        kind="DoubleWell", d=d, T=T, X_0=-torch.ones(d), B=B,        # :189
        b=lambda x: -(4.0 * kappa * x * (x ** 2 - 1)),               # :198-201
        sigma=lambda x: B,                                           # :204
        h=lambda t, x, y, z: -0.5 * torch.sum(z ** 2, dim=1),        # :210
        f=lambda x, t: torch.zeros(x.shape[0]),                      # :207
        g=lambda x: (eta * (x - 1) ** 2).squeeze(), extra={})        # :213


def problem_double_well_general(d=1, d_1=1, d_2=0, T=1, eta=1, kappa=1, modus="HJB") -> OracleProblem:
    """problems.py:479-534 (DoubleWell_multidim_for_general_solver); f is the terminal value."""
    eta_, kappa_, grad_V, cost = _double_well_parts(d, d_1, d_2, eta, kappa)
    B = torch.eye(d)                                                 # :493
    if modus == "linear":
        h = lambda t, x, y, z: torch.zeros(x.shape[0])               # :517-518
        f = lambda x: torch.exp(-cost(x))                            # :531-532
    else:
        h = lambda t, x, y, z: -0.5 * torch.sum(z ** 2, dim=1)       # :519
        f = cost                                                     # :534
    return OracleProblem(
        kind="DoubleWell_multidim_for_general_solver", d=d, T=T, X_0=-torch.ones(d), B=B,
        b=lambda x: -grad_V(x), sigma=lambda x: B, h=h, f=f,
        extra=dict(boundary="unbounded_square", X_l=-2.5, X_r=2.5, eta_=eta_, kappa_=kappa_))   # :496-498


def problem_allen_cahn(d=1, T=0.3, seed=42, modus="pt") -> OracleProblem:
    """problems.py:1175-1209 (AllenCahn, modus='pt')."""
    np.random.seed(seed)                                             # :1178
    B = torch.tensor(np.eye(d) * np.sqrt(2)).float()                 # :1183-1184
    return OracleProblem(
        kind="AllenCahn", d=d, T=T, X_0=torch.zeros(d), B=B,
        b=lambda x: torch.zeros(x.shape),                            # :1194
        sigma=lambda x: B,                                           # :1200
        h=lambda t, x, y, z: y - y ** 3,                             # :1204
        f=lambda x: 1 / (2 + 2 / 5 * torch.sum(x ** 2, 1)),          # :1208
        extra=dict(boundary="unbounded", boundary_distance=2.0))     # :1190-1191


def problem_heat(d=1, T=1, seed=42) -> OracleProblem:
    """problems.py:1733-1758 (HeatEquation)."""
    torch.manual_seed(seed)                                          # :1736
    B = torch.sqrt(torch.tensor(2.0)) * torch.eye(d)                 # :1740
    return OracleProblem(
        kind="HeatEquation", d=d, T=T, X_0=torch.zeros(d), B=B,
        b=lambda x: torch.zeros(x.shape),                            # :1746
        sigma=lambda x: B,                                           # :1749
        h=lambda t, x, y, z: torch.zeros(x.shape[0]),                # :1755
        f=lambda x: torch.sum(x ** 2, 1),                            # :1758
        extra=dict(boundary="unbounded", boundary_distance=1.0))     # :1741-1743


def _exp_ball(kind, d, alpha, T, parabolic, extra_y, nonlinear, boundary_type):
    """The exponential-on-the-ball family (problems.py:962-993 ExponentialOnSphere, :995-1029 ExponentialOnBallNonlinear,
    :1031-1065 ExponentialOnBallNonlinearSin, :1137-1172 ExponentialOnSphereNonlinearParabolic):
    sigma = sqrt(2) I, b = 0, unit ball, v_true = exp(alpha |x|^2 [+ t])."""
    B = torch.sqrt(torch.tensor(2.0)) * torch.eye(d)                 # :967, :1000, :1036, :1142
    r2 = lambda x: torch.sum(x ** 2, 1)

    def h_elliptic(x, y, z):
        if nonlinear == "none":
            return -alpha * y * (alpha * 4 * r2(x) + 2 * d)          # :985
        lin = -2 * alpha * y * (alpha * 2 * r2(x) + d)
        if nonlinear == "sq":
            return lin + torch.exp(2 * alpha * r2(x)) - y ** 2       # :1022
        return lin + torch.sin(torch.exp(2 * alpha * r2(x)) - y ** 2)    # :1058

    def h_parabolic(t, x, y, z):                                     # :1166
        return -2 * alpha * y * (alpha * 2 * r2(x) + d) - y + torch.sin(torch.exp(2 * alpha * r2(x) + 2 * t) - y ** 2)

    if parabolic:
        def g(x, t):                                                 # :1159-1163
            if boundary_type == "Neumann":
                return 2 * alpha * x * torch.exp(alpha * r2(x) + t).unsqueeze(1)
            return torch.exp(alpha * r2(x) + t)
        f = lambda x: torch.exp(alpha * r2(x) + T)                   # :1157
        v_true = lambda x, t: torch.exp(alpha * r2(x) + t)
    else:
        def g(x):                                                    # :982, :1016-1019
            if boundary_type == "Neumann":
                return 2 * alpha * x * torch.exp(alpha * r2(x)).unsqueeze(1)
            return torch.exp(alpha * r2(x))
        f = lambda x, t=None: torch.zeros(x.shape[0])
        v_true = lambda x: torch.exp(alpha * r2(x))
    return OracleProblem(
        kind=kind, d=d, T=T, X_0=torch.zeros(d), B=B, b=lambda x: torch.zeros(x.shape), sigma=lambda x: B,
        h=h_parabolic if parabolic else h_elliptic, f=f, g=g,
        extra=dict(boundary="sphere", boundary_distance=1.0, boundary_type=boundary_type, v_true=v_true))


def problem_exp_sphere(d=2, alpha=1.0) -> OracleProblem:
    return _exp_ball("ExponentialOnSphere", d, alpha, None, False, 0, "none", "Dirichlet")


def problem_exp_ball_nonlinear(d=2, alpha=1.0, boundary_type="Dirichlet") -> OracleProblem:
    return _exp_ball("ExponentialOnBallNonlinear", d, alpha, None, False, 0, "sq", boundary_type)


def problem_exp_ball_nonlinear_sin(d=2, alpha=1.0, boundary_type="Dirichlet") -> OracleProblem:
    return _exp_ball("ExponentialOnBallNonlinearSin", d, alpha, None, False, 0, "sin", boundary_type)


def problem_exp_sphere_nonlinear_parabolic(d=2, T=1.0, alpha=1.0, boundary_type="Dirichlet") -> OracleProblem:
    """boundary_type is an attribute the reference class fixes to 'Dirichlet' (:1148); callers set 'Neumann' on the
    instance (the Neumann notebook), which is what the keyword stands for here."""
    return _exp_ball("ExponentialOnSphereNonlinearParabolic", d, alpha, T, True, 1, "sin", boundary_type)


def problem_quadratic_on_box(d=2, T=0.5, X_l=-1.0, X_r=1.0, one_boundary=False, scale=1.0, parabolic=True,
                             quad_h=True) -> OracleProblem:
    """NOT a reference class: a duck-typed problem on the box [X_l, X_r]^d that pins the 'square' exit
    tests (solver.py:1125-1129, :762-767) with coefficients the kernels have: b = 0, sigma = scale I,
    h = -|z|^2/2 (or 0), boundary/terminal data |x|^2.  The golden script hands the same object to the reference solvers."""
    B = scale * torch.eye(d)
    hq = (lambda z: -0.5 * torch.sum(z ** 2, dim=1)) if quad_h else (lambda z: torch.zeros(z.shape[0]))
    q = lambda x: torch.sum(x ** 2, 1)
    if parabolic:
        h, f, g = (lambda t, x, y, z: hq(z)), (lambda x: q(x)), (lambda x, t: q(x) + (T - t))
        v_true = lambda x, t: q(x)
    else:
        h, f, g = (lambda x, y, z: hq(z)), (lambda x, t=None: torch.zeros(x.shape[0])), (lambda x: q(x))
        v_true = lambda x: q(x)
    return OracleProblem(kind="QuadraticOnBox", d=d, T=T, X_0=torch.zeros(d), B=B, b=lambda x: torch.zeros(x.shape),
                         sigma=lambda x: B, h=h, f=f, g=g,
                         extra=dict(boundary="square", X_l=X_l, X_r=X_r, one_boundary=one_boundary,
                                    boundary_type="Dirichlet", v_true=v_true))


def problem_committor(d=2, alpha=1.0) -> OracleProblem:
    """Committor between two concentric spheres (problems.py:1546-1579): b = 0, sigma = I, h = 0, boundary data 1 on the outer
    and 0 on the inner sphere, radii a = 1 and c = 2."""
    a, c = 1.0, 2.0                                                  # :1549-1550
    B = torch.eye(d)                                                 # :1552
    r = lambda x: torch.sqrt(torch.sum(x ** 2, 1))
    v_true = lambda x: ((a ** 2 - r(x) ** (2 - d) * a ** d) / (a ** 2 - c ** (2 - d) * a ** d))     # :1577-1579
    return OracleProblem(kind="Committor", d=d, T=None, X_0=torch.zeros(d), B=B, b=lambda x: torch.zeros(x.shape),
                         sigma=lambda x: B, h=lambda x, y, z: torch.zeros(x.shape[0]),                # :1571-1572
                         f=lambda x, t=None: torch.zeros(x.shape[0]), g=lambda x: (r(x) > a).float(),  # :1565-1569
                         extra=dict(boundary="two_spheres", boundary_distance_1=a, boundary_distance_2=c,
                                    boundary_type="Dirichlet", v_true=v_true))


PROBLEMS = {
    "Committor": problem_committor,
    "ExponentialOnSphere": problem_exp_sphere, "ExponentialOnBallNonlinear": problem_exp_ball_nonlinear,
    "ExponentialOnBallNonlinearSin": problem_exp_ball_nonlinear_sin,
    "ExponentialOnSphereNonlinearParabolic": problem_exp_sphere_nonlinear_parabolic,
    "QuadraticOnBox": problem_quadratic_on_box,
    "LLGC": problem_llgc, "LQGC": problem_lqgc, "DoubleWell_multidim": problem_double_well,
    "DoubleWell": lambda **kw: problem_double_well_1d(**kw),
    "DoubleWell_multidim_for_general_solver": problem_double_well_general,
    "AllenCahn": problem_allen_cahn, "HeatEquation": problem_heat,
}


_DOMAIN_ATTRS = ("boundary", "boundary_distance", "boundary_distance_1", "boundary_distance_2", "X_corner", "X_l", "X_r")


def make_problem(kind: str, **kwargs) -> OracleProblem:
    """Domain attributes a caller sets on the problem INSTANCE (problem.boundary = 'two_spheres', ...) are accepted as
    keywords next to the constructor's own and land in `extra`."""
    over = {k: kwargs.pop(k) for k in list(kwargs) if k in _DOMAIN_ATTRS and k not in _ctor_args(PROBLEMS[kind])}
    pb = PROBLEMS[kind](**kwargs)
    pb.extra.update(over)
    return pb


def _ctor_args(fn):
    import inspect
    return set(inspect.signature(fn).parameters)


# --------------------------------------------------------------------------------------
# ansatz spaces (reference function_space.py)
# --------------------------------------------------------------------------------------
class TanhMLP(torch.nn.Module):
    """function_space.py:177-195 (MySequential) with configurable hidden widths.

    Seeding recipe :180-188: manual_seed(seed); one nn.Linear per layer (its default
    init consumes generator state); then normal_(0, 0.01) on weight and bias, layer by
    layer.  widths=[30,30] is the reference's hard-coded :181.
    """

    def __init__(self, d_in, d_out, lr, seed, widths=(30, 30)):
        super().__init__()
        torch.manual_seed(seed)
        dims = [d_in] + list(widths) + [d_out]
        self.dims = dims
        self.linears = torch.nn.ModuleList(
            [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)])
        self.optim = torch.optim.Adam(self.parameters(), lr=lr)      # :185 (before the re-init)
        for lin in self.linears:
            torch.nn.init.normal_(lin.weight, 0, 0.01)
            torch.nn.init.normal_(lin.bias, 0, 0.01)

    def forward(self, x):                                            # :190-195
        last = len(self.linears) - 1
        for i, lin in enumerate(self.linears):
            x = lin(x)
            if i < last:
                x = torch.tanh(x)
        return x


class DenseNetOracle(torch.nn.Module):
    """function_space.py:116-140: dense-concat net, relu(.)**2, weights randn*0.1, zero bias.  ``activation='tanh2'`` is the
    variant `Committor function.ipynb` (cell 1, DenseNet_tanh_2) defines for itself and swaps into model.V: the same
    constructor, tanh(.)**2 in the forward.  ``activation='tanh'``: the same constructor with tanh, the dense-concat layout the
    package's DenseNet(activation='tanh') keeps (unlike DenseNet_tanh, whose weights are nn.Linear layers)."""

    def __init__(self, d_in, d_out, lr, arch=(30, 30), seed=42, activation="relu2"):
        super().__init__()
        self.activation = activation
        torch.manual_seed(seed)                                      # :119
        dims = [d_in] + list(arch) + [d_out]
        self.dims = dims
        ws = []
        for i in range(len(dims) - 1):                               # :121-125
            ws.append(torch.nn.Parameter(torch.randn(sum(dims[:i + 1]), dims[i + 1]) * 0.1))
            ws.append(torch.nn.Parameter(torch.zeros(dims[i + 1])))
        self.W = ws
        for i, w in enumerate(ws):
            self.register_parameter("param %d" % i, w)               # :128-129
        self.optim = torch.optim.Adam(self.parameters(), lr=lr)      # :131

    def forward(self, x):                                            # :133-140
        nl = len(self.dims) - 1
        for i in range(nl):
            lin = torch.matmul(x, self.W[2 * i]) + self.W[2 * i + 1]
            if i == nl - 1:
                x = lin
            elif self.activation == "tanh2":
                x = torch.cat([x, torch.tanh(lin) ** 2], dim=1)      # Committor function.ipynb cell 1
            elif self.activation == "tanh":
                x = torch.cat([x, torch.tanh(lin)], dim=1)           # the package's DenseNet(activation='tanh')
            else:
                x = torch.cat([x, torch.nn.functional.relu(lin) ** 2], dim=1)
        return x


class DenseNetTanhOracle(torch.nn.Module):
    """function_space.py:143-158 (DenseNet_tanh): dense-concat net of nn.Linear layers with tanh."""

    def __init__(self, d_in, d_out, lr, arch=(30, 30), seed=42):
        super().__init__()
        torch.manual_seed(seed)                                      # :146
        dims = [d_in] + list(arch) + [d_out]
        self.dims = dims
        self.layers = torch.nn.ModuleList([torch.nn.Linear(sum(dims[:i + 1]), dims[i + 1])
                                           for i in range(len(dims) - 1)])     # :148-149
        self.optim = torch.optim.Adam(self.parameters(), lr=lr)      # :150

    def forward(self, x):                                            # :152-158
        nl = len(self.dims) - 1
        for i in range(nl):
            if i == nl - 1:
                x = self.layers[i](x)
            else:
                x = torch.cat([x, torch.tanh(self.layers[i](x))], dim=1)
        return x


def value_net(d_in, lr, seed, net=None, arch=None):
    """The value net of a golden case: ``net`` = dict(kind, arch, seed) ('densenet' / absent kind: DenseNet; 'user_tanh2': the
    committor notebook's own class; 'densenet_tanh': DenseNet_tanh; 'densenet_concat_tanh': DenseNet with tanh), or just
    ``arch`` for a DenseNet with the solver's seed."""
    if net is None:
        kw = {} if arch is None else dict(arch=arch)
        return DenseNetOracle(d_in, 1, lr, seed=seed, **kw)
    kind = net.get("kind", "densenet")
    if kind == "densenet_tanh":
        return DenseNetTanhOracle(d_in, 1, lr, arch=net["arch"], seed=net["seed"])
    act = {"user_tanh2": "tanh2", "densenet_concat_tanh": "tanh"}.get(kind, "relu2")
    return DenseNetOracle(d_in, 1, lr, arch=net["arch"], seed=net["seed"], activation=act)


class ScalarY0(torch.nn.Module):
    """function_space.py:6-21 (SingleParam, initial=None)."""

    def __init__(self, lr, seed=42):
        super().__init__()
        torch.manual_seed(seed)                                      # :9
        self.Y_0 = torch.nn.Parameter(torch.tensor([0.0]))           # :11
        self.register_parameter("param", self.Y_0)                   # :17
        self.optim = torch.optim.Adam(self.parameters(), lr=lr)      # :18

    def forward(self, x):
        return self.Y_0


# --------------------------------------------------------------------------------------
# Solver.train restatement (reference solver.py:420-557), control ansatz
# --------------------------------------------------------------------------------------
@dataclass
class HJBConfig:
    K: int
    delta_t: float
    lr: float = 0.001
    L: int = 1
    seed: int = 42
    loss_method: str = "log-variance"
    time_approx: str = "inner"
    learn_Y_0: bool = False
    adaptive_forward_process: bool = True
    detach_forward: bool = False
    random_X_0: bool = False
    IS_variance_K: int = 0
    IS_variance_iter: int = 1
    approx_method: str = "control"       # or 'value_function' (solver.py:93-97, 334-339, 438-440; time_approx='inner')


def hjb_build(problem: OracleProblem, cfg: HJBConfig, net: Optional[torch.nn.Module] = None):
    """Constructor side effects of Solver.__init__ that matter for parity (solver.py:84-99)."""
    torch.manual_seed(cfg.seed)                                      # :84
    y0 = ScalarY0(lr=cfg.lr)                                         # :86 (re-seeds with 42)
    N = int(np.floor(problem.T / cfg.delta_t))                       # :41 (float64)
    if cfg.approx_method == "value_function":
        assert cfg.time_approx == "inner"
        z = DenseNetOracle(problem.d + 1, 1, cfg.lr, seed=cfg.seed)  # :97 (y_n = [DenseNet(d + 1 -> 1)]; no y_0 in this ansatz)
    elif cfg.time_approx == "inner":
        z = TanhMLP(problem.d + 1, problem.d, cfg.lr, seed=123)      # :91
    else:
        z = [DenseNetOracle(problem.d, problem.d, cfg.lr, seed=cfg.seed) for _ in range(N)]   # :88
    if net is not None:
        z = net
    return z, y0, N


def control_eval(z, X, n, dt32, N, time_approx="inner"):
    """solver.py:349-356 (Z_n_)."""
    if time_approx == "outer":
        return z[max(0, min(n, N - 1))](X)                           # :352-353
    t_X = torch.cat([torch.ones([X.shape[0], 1]) * n * dt32, X], 1)  # :355
    return z(t_X)                                                    # :356


def value_eval(y_n, X, t):
    """solver.py:334-339 (Y_n, 'inner'): the time feature is the ARGUMENT t as passed -- the training loop passes the step
    index n, not n * delta_t (:439, :328)."""
    t_X = torch.cat([torch.ones([X.shape[0], 1]) * t, X], 1)          # :338
    return y_n(t_X)                                                  # :339


def value_gradient(y_n, X, n, problem):
    """solver.py:326-332 (compute_grad_Y): Z = sigma(X) grad_x Y_n(X, n), differentiable (create_graph)."""
    Y_eval = value_eval(y_n, X, n).squeeze(1).sum()                  # :327
    Zg, = torch.autograd.grad(Y_eval, X, create_graph=True)          # :329 (the .backward of :328 only fills .grad, cleared at :194)
    return torch.mm(problem.sigma(X), Zg.t()).t()                    # :330


def hjb_loss(kind, D, Y, gX, Z_sum=None, adaptive=True):
    """solver.py:164-192 for the losses in scope."""
    if kind == "moment":
        return D.pow(2).mean()                                       # :166
    if kind == "log-variance":
        return D.pow(2).mean() - D.mean().pow(2)                     # :168
    if kind == "variance":
        return torch.var(torch.exp(-gX + Y))                         # :172
    if kind == "cross_entropy":
        if adaptive:
            return (Y * torch.exp(-gX + Y.detach())).mean()          # :185
        return (Y * torch.exp(-gX)).mean()                           # :186
    if kind == "relative_entropy":
        return (Z_sum + gX).mean()                                   # :179-180
    raise NotImplementedError(kind)


def hjb_train(problem: OracleProblem, cfg: HJBConfig, net=None, noise: Optional[List[torch.Tensor]] = None,
              x0_noise: Optional[List[torch.Tensor]] = None, trace: bool = False, step_models=None):
    """Restates Solver.train (solver.py:420-557) for approx_method='control'.

    noise: optional list (one per iteration) of xi tensors shaped (K, d, N+1) replacing the
    CPU-generator draw of :381 (used to feed device-generated Philox noise to the oracle).
    Returns dict(loss_log, Y_0_log, z, y0, traces).
    """
    z, y0, N = step_models if step_models is not None else hjb_build(problem, cfg, net)
    phis = (list(z) if isinstance(z, list) else [z]) + ([y0] if cfg.learn_Y_0 else [])   # :142-153
    for p_ in phis:
        p_.train()
    dt32 = torch.tensor(cfg.delta_t)                                 # :39
    sq_dt32 = torch.sqrt(dt32)                                       # :40
    K, d = cfg.K, problem.d
    out = dict(loss_log=[], Y_0_log=[], traces=[], N=N, IS_rel_log=[])
    torch.manual_seed(cfg.seed)                                      # :422
    for l in range(cfg.L):
        X = problem.X_0.repeat(K, 1)                                 # :365
        if cfg.random_X_0:
            X = torch.randn(K, d) if x0_noise is None else x0_noise[l]   # :367
        Y = torch.tensor([0.0]).repeat(K)                            # :368
        if cfg.learn_Y_0:
            Y = y0(X)                                                # :373 (shape (1,), broadcasts)
            out["Y_0_log"].append(Y[0].item())                       # :374
        vf = cfg.approx_method == "value_function"
        if vf:
            X = X.clone().requires_grad_(True)                       # :370
            Y = value_eval(z, X, 0)[:, 0]                            # :371
        xi = torch.randn(K, d, N + 1) if noise is None else noise[l]     # :381
        tr = dict(X=[X.detach().clone()], Y=[]) if trace else None
        Z_sum = torch.zeros(K)                                       # :376
        additional_loss = torch.zeros(K)                             # :434
        for n in range(N):
            if vf and n > 0:
                additional_loss = additional_loss + (value_eval(z, X, n)[:, 0] - Y).pow(2)    # :438-440
            Z = value_gradient(z, X, n, problem) if vf else control_eval(z, X, n, dt32, N, cfg.time_approx)      # :449
            c = torch.zeros(d, K)                                    # :451
            if cfg.adaptive_forward_process:
                c = -(value_gradient(z, X, n, problem) if vf else control_eval(z, X, n, dt32, N, cfg.time_approx)).t()     # :456 (2nd forward)
            if cfg.detach_forward:
                c = c.detach()                                       # :468-469
            sig = problem.sigma(X)
            X = (X + (problem.b(X) + torch.mm(sig, c).t()) * dt32
                 + torch.mm(sig, xi[:, :, n + 1].t()).t() * sq_dt32)     # :471-472
            Y = (Y + (-problem.h(dt32 * n, X, Y, Z) + torch.sum(Z * c.t(), 1)) * dt32
                 + torch.sum(Z * xi[:, :, n + 1], 1) * sq_dt32)      # :477-478 (h sees X_{n+1})
            if "relative_entropy" in cfg.loss_method:                # :484-486 (f at the UPDATED state, time n dt)
                Z_sum = Z_sum + (0.5 * torch.sum(Z ** 2, dim=1) + problem.f(X, n * dt32)) * dt32
            if trace:
                tr["X"].append(X.detach().clone())
                tr["Y"].append(Y.detach().clone())
        for p_ in phis:
            p_.optim.zero_grad()                                     # :194-196
        gX = problem.g(X)
        D = Y - gX
        loss = hjb_loss(cfg.loss_method, D, Y, gX, Z_sum=Z_sum, adaptive=cfg.adaptive_forward_process) + additional_loss.mean()   # :220, :434, :499
        loss.backward()                                              # :221
        if trace:
            tr["D"] = D.detach().clone()
            tr["Zsum_g"] = (Z_sum + gX).detach().clone()
            nets_ = z if isinstance(z, list) else [z]                # 'outer': every step's net, in step order
            tr["grads"] = [p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)
                           for net_ in nets_ for p in net_.parameters()]
            out["traces"].append(tr)
        for p_ in phis:
            p_.optim.step()                                          # :198-200
        out["loss_log"].append(loss.item())                          # :514
        if cfg.IS_variance_K > 0 and l % cfg.IS_variance_iter == 0:  # :521-528 (draws from the same generator)
            out["IS_rel_log"].append(is_eval(problem, z, cfg.delta_t, N, cfg.IS_variance_K,
                                             time_approx=cfg.time_approx)[2])
    out["z"], out["y0"] = z, y0
    return out


def is_eval(problem: OracleProblem, z, model_delta_t, N_model, K, delta_t=0.01, time_approx="inner"):
    """Restates utilities.do_importance_sampling_me (utilities.py:287-359), control='approx',
    simulate_naive=False: forward-only controlled rollout with its own step delta_t, Girsanov weight
    exp(-int u.dW - 0.5 int |u|^2 dt), statistics of exp(-int f - g(X_T)) * weight."""
    sq_dt = np.sqrt(delta_t)                                          # :298 (float64 numpy scalars)
    N = int(np.ceil(problem.T / delta_t))                            # :299
    dt32 = torch.tensor(model_delta_t)
    X_u = problem.X_0.repeat(K, 1)                                   # :303
    ito = torch.zeros(K)
    riemann = torch.zeros(K)
    f_int_u = torch.zeros(K)
    for n in range(N):
        xi = torch.randn(K, problem.d)                               # :310
        t = n * delta_t
        n_idx = int(torch.ceil(t / dt32))                            # solver.py:361 (Z_n)
        with torch.no_grad():
            ut = -control_eval(z, X_u, n_idx, dt32, N_model, time_approx)     # :321
        sig = problem.sigma(X_u)
        X_u = (X_u + (problem.b(X_u) + torch.mm(sig, ut.t()).t()) * delta_t
               + torch.mm(sig, xi.t()).t() * sq_dt)                  # :324-325
        ito = ito + torch.sum(ut * xi, 1) * sq_dt                    # :326
        riemann = riemann + torch.sum(ut ** 2, 1) * delta_t          # :327
        f_int_u = f_int_u + problem.f(X_u, n * delta_t) * delta_t    # :328
    girsanov = torch.exp(-ito - 0.5 * riemann)                       # :330
    w = torch.exp(-f_int_u - problem.g(X_u)) * girsanov
    mean_IS = torch.mean(w).item()                                   # :336
    var_IS = torch.var(w).item()                                     # :337
    return mean_IS, var_IS, float(np.sqrt(var_IS) / mean_IS)         # :338


def control_on_grid(z, X, t, delta_t, N, time_approx="inner"):
    """solver.py:360-362: n = ceil(t/dt) in fp32 then Z_n_; the control is u = -Z."""
    dt32 = torch.tensor(delta_t)
    n = int(torch.ceil(torch.tensor(t) / dt32))
    with torch.no_grad():
        return -control_eval(z, X, n, dt32, N, time_approx)


# --------------------------------------------------------------------------------------
# GeneralSolver.train restatement (reference solver.py:1001-1206), unbounded and bounded (sphere / square) domains
# --------------------------------------------------------------------------------------
@dataclass
class GeneralConfig:
    K: int
    N: int
    delta_t: float
    lr: float = 0.001
    L: int = 1
    seed: int = 42
    K_boundary: int = 50
    alpha: tuple = (1.0, 1.0, 1.0)
    loss_method: str = "diffusion"
    adaptive_forward_process: bool = False
    detach_forward: bool = True
    uniform_square: bool = False
    loss_with_stopped: bool = False
    K_test_log: Optional[int] = None
    sample_center: bool = False


def general_build(problem: OracleProblem, cfg: GeneralConfig, arch=None, net=None):
    torch.manual_seed(cfg.seed)                                      # :978
    return value_net(problem.d + 1, cfg.lr, cfg.seed, net=net, arch=arch)    # :980 (or the net the caller swaps in)


def compute_test_error(V, problem: OracleProblem, K: int, modus: str):
    """utilities.py:441-472: Monte-Carlo error of V on K fresh points of the domain (CPU generator)."""
    ex, d = problem.extra, problem.d
    if ex["boundary"] in ("sphere", "unbounded"):
        X = torch.randn(K, d)                                        # :446
        X = ex["boundary_distance"] * X / torch.sqrt(torch.sum(X ** 2, 1)).unsqueeze(1) * (torch.rand(K).unsqueeze(1) ** (1 / d))
    elif ex["boundary"] == "two_spheres":
        X = torch.randn(K, d)                                        # :449
        X = ex["boundary_distance_2"] * X / torch.sqrt(torch.sum(X ** 2, 1)).unsqueeze(1) * (torch.rand(K).unsqueeze(1) ** (1 / d))
        X = X[torch.sqrt(torch.sum(X ** 2, 1)) > ex["boundary_distance_1"], :]      # :451-452
    else:
        X = (ex["X_r"] - ex["X_l"]) * torch.rand(K, d) + ex["X_l"]   # :456
    if modus == "parabolic":
        t_n = torch.rand(K, 1) * problem.T                           # :459
        v_true = np.array(ex["v_true"](X.detach(), t_n.squeeze()).squeeze())
        v_est = V(torch.cat([X, t_n], 1)).squeeze().detach().numpy()
    else:
        v_true = np.array(ex["v_true"](X.detach()).squeeze())        # :467
        v_est = V(X).squeeze().detach().numpy()
    return float(np.mean((v_true - v_est) ** 2)), float(np.mean(np.abs(v_true - v_est))), \
        float(np.mean(np.abs(v_true - v_est) / v_true))


def sample_boundary(problem: OracleProblem, Kb: int):
    """Uniform points on the boundary (solver.py:1020-1038 == :650-680).  The square variant shuffles with numpy's
    GLOBAL generator (np.random.shuffle), as the reference does."""
    d, ex = problem.d, problem.extra
    if ex["boundary"] == "sphere":
        Xb = torch.randn(Kb, d)                                      # :1021
        return ex["boundary_distance"] * Xb / torch.sqrt(torch.sum(Xb ** 2, 1)).unsqueeze(1)    # :1022
    half = int(Kb / 2)
    if ex["boundary"] == "two_spheres":
        Xb = torch.randn(Kb, d)                                      # :1024 == :654
        radii = torch.tensor([ex["boundary_distance_1"]] * half + [ex["boundary_distance_2"]] * half).unsqueeze(1)   # :1025-1026
        return radii * Xb / torch.sqrt(torch.sum(Xb ** 2, 1)).unsqueeze(1)                        # :1027
    assert ex["boundary"] in ("square", "square-corner")
    sel = np.concatenate([np.ones(half)[:, np.newaxis], np.zeros([half, d - 1])], 1)     # :1029
    np.apply_along_axis(np.random.shuffle, 1, sel)                   # :1030
    a = np.concatenate([sel, np.zeros([half, d])]).astype(bool)      # :1031
    b = np.concatenate([np.zeros([half, d]), sel]).astype(bool)      # :1032
    X_l, X_r = ex["X_l"], ex["X_r"]
    if ex["boundary"] == "square-corner":
        Xc = ex["X_corner"]
        Xb = (X_r - Xc) * torch.rand(Kb, d) + Xc                     # :671
        Xb[torch.tensor(a.astype(float)).bool()] = Xc                # :672
        Xb[torch.tensor(b.astype(float)).bool()] = Xc                # :673
        return Xb
    Xb = (X_r - X_l) * torch.rand(Kb, d) + X_l                       # :1033
    Xb[torch.tensor(a.astype(float)).bool()] = X_l                   # :1034
    Xb[torch.tensor(b.astype(float)).bool()] = X_r                   # :1035
    if ex["one_boundary"]:
        Xb[torch.tensor(a.astype(float)).bool()] = X_r               # :1037
        Xb[torch.tensor(b.astype(float)).bool()] = X_r               # :1038
    return Xb


def exit_test(problem: OracleProblem, X, X_prop, elliptic: bool):
    """new_selection of solver.py:1119-1129 (GeneralSolver) / :758-767 (EllipticSolver)."""
    ex = problem.extra
    if ex["boundary"] == "sphere":
        return torch.all(torch.sqrt(torch.sum(X ** 2, 1)).unsqueeze(1) < ex["boundary_distance"], 1)   # :1121 (X, not the proposal)
    if ex["boundary"] == "square":
        if ex["one_boundary"]:
            le = X_prop <= ex["X_r"]
            return torch.all(le, 1) if elliptic else torch.any(le, 1)            # :764 vs :1127
        return torch.all((X_prop >= ex["X_l"]) & (X_prop <= ex["X_r"]), 1)       # :1129
    if ex["boundary"] == "two_spheres":                                         # :1122-1123 == :752-753 (X, not the proposal)
        r = torch.sqrt(torch.sum(X ** 2, 1))
        return (r > ex["boundary_distance_1"]) & (r < ex["boundary_distance_2"])
    if ex["boundary"] == "square-corner":
        return torch.any(X_prop <= ex["X_r"], 1)                                 # :759-760
    return torch.ones(X.shape[0]).bool()


def neumann_residual(V, Xb_in, g_val, d):
    """mean((grad_x V . x - g . x)^2) on the boundary batch (solver.py:1069-1074, :688-693)."""
    Xb_in = Xb_in.clone().requires_grad_(True)
    Y_eval = V(Xb_in).squeeze().sum()
    grad_V, = torch.autograd.grad(Y_eval, Xb_in, create_graph=True)
    xb = Xb_in[:, :d]
    return torch.mean((torch.sum(grad_V[:, :d] * xb, 1) - torch.sum(g_val * xb, 1)) ** 2)


def general_train(problem: OracleProblem, cfg: GeneralConfig, V=None, trace=False):
    """Restates GeneralSolver.train for loss_method in {'diffusion','BSDE'} on
    boundary in {'unbounded','unbounded_square','sphere','two_spheres','square'} (solver.py:1001-1206)."""
    if V is None:
        V = general_build(problem, cfg)
    dt32 = torch.tensor(cfg.delta_t)                                 # :950
    sq_dt32 = torch.sqrt(dt32)                                       # :951
    K, d, T = cfg.K, problem.d, problem.T
    bnd = problem.extra["boundary"]
    bounded = "unbounded" not in bnd
    btype = problem.extra.get("boundary_type")
    out = dict(loss_log=[], K_log=[], traces=[], V_test_L2=[])
    torch.manual_seed(cfg.seed)                                      # :1003
    for l in range(cfg.L):
        loss = 0
        if cfg.sample_center:                                        # :1015-1017
            X_center = torch.zeros(1, 1)
            loss = loss + torch.mean((V(X_center).squeeze() - problem.extra["v_true"](X_center).squeeze()) ** 2)
        if bounded:
            X_boundary = sample_boundary(problem, cfg.K_boundary)    # :1020-1038
        if bnd in ("unbounded", "sphere"):                           # :1040
            if cfg.uniform_square:
                X = torch.rand(K, d) * 2 - 1                         # :1042
                X = problem.extra["boundary_distance"] * X / torch.sqrt(torch.sum(X ** 2, 1)).unsqueeze(1) \
                    * (torch.rand(K).unsqueeze(1))                   # :1043
            else:
                X = torch.randn(K, d)                                # :1045
                X = problem.extra["boundary_distance"] * X / torch.sqrt(torch.sum(X ** 2, 1)).unsqueeze(1) \
                    * (torch.rand(K).unsqueeze(1) ** (1 / d))        # :1046
        elif bnd == "two_spheres":
            X = torch.randn(cfg.K, d)                                # :1048 (K_original draws)
            X = problem.extra["boundary_distance_2"] * X / torch.sqrt(torch.sum(X ** 2, 1)).unsqueeze(1) \
                * (torch.rand(cfg.K).unsqueeze(1) ** (1 / d))        # :1049
            selection = torch.sqrt(torch.sum(X ** 2, 1)) > problem.extra["boundary_distance_1"]      # :1050
            X = X[selection, :]                                      # :1051
            K = int(torch.sum(selection))                            # :1052: the batch size follows the rejection step
        else:
            X_l, X_r = problem.extra["X_l"], problem.extra["X_r"]
            X = (X_r - X_l) * torch.rand(K, d) + X_l                 # :1056
        if bounded:
            t_b = torch.rand(cfg.K_boundary, 1) * T                  # :1059
            X_t_b = torch.cat([X_boundary, t_b], 1)                  # :1060
        if cfg.loss_method != "BSDE":                                # :1062 (boundary_loss=True)
            Kb = cfg.K_boundary
            X_T = torch.cat([X[:Kb, :], T * torch.ones(Kb).unsqueeze(1)], 1)    # :1063
            loss = loss + cfg.alpha[1] * torch.mean((V(X_T).squeeze() - problem.f(X[:Kb, :])) ** 2)   # :1064
            if bounded and btype == "Dirichlet":                     # :1066-1067
                loss = loss + cfg.alpha[2] * torch.mean((V(X_t_b).squeeze() - problem.g(X_boundary, t_b.squeeze())) ** 2)
            elif bounded and btype == "Neumann":                     # :1068-1074
                loss = loss + cfg.alpha[2] * neumann_residual(V, X_t_b, problem.g(X_boundary, t_b.squeeze()), d)
        X = X.clone().requires_grad_(True)                           # :1076
        t_n = torch.rand(K, 1) * T                                   # :1078
        X_t_n = torch.cat([X, t_n], 1)                               # :1079
        Y = V(X_t_n).squeeze()                                       # :1081
        stopped = torch.zeros(K).bool()                              # :1084
        K_count = 0
        tr = dict(X0=X.detach().clone(), t0=t_n.clone(), xi=[]) if trace else None
        if trace and bounded:                                        # the boundary batch and its times, for a replay of the draws
            tr["X_boundary"], tr["t_b"] = X_boundary.clone(), t_b.clone()
        for n in range(cfg.N):
            if torch.sum(~stopped) == 0:                             # :1093-1097
                break
            Y_ = V(X_t_n)                                            # :1100
            Y_eval = Y_.squeeze().sum()
            grad_V, = torch.autograd.grad(Y_eval, X, create_graph=True)      # :1103 (the extra .backward of :1102 only fills .grad, cleared at :1164)
            Z = torch.mm(problem.sigma(X).t(), grad_V.t()).t()       # :1104
            xi = torch.randn(K, d)                                   # :1106
            if trace:
                tr["xi"].append(xi.clone())
            c = torch.zeros(d, K)                                    # :1110
            if cfg.adaptive_forward_process:
                c = -Z.t()                                           # :1112
            if cfg.detach_forward:
                c = c.detach()                                       # :1114
            sel = (~stopped).float().unsqueeze(1).repeat(1, d)
            X_prop = (X + ((problem.b(X) + torch.mm(problem.sigma(X), c).t()) * dt32
                           + torch.mm(problem.sigma(X), xi.t()).t() * sq_dt32) * sel)   # :1116-1117
            new_sel = exit_test(problem, X, X_prop, elliptic=False)  # :1119-1129
            new_sel = new_sel & ((t_n.squeeze() + dt32) <= T)        # :1131
            act = (new_sel & ~stopped)
            Y = (Y + ((-problem.h(n * dt32, X, Y_.squeeze(), Z) + torch.sum(Z * c.t(), 1)) * dt32
                      + torch.sum(Z * xi, 1) * sq_dt32) * act.float())       # :1141-1142
            X = (X * (~new_sel | stopped).float().unsqueeze(1).repeat(1, d)
                 + X_prop * act.float().unsqueeze(1).repeat(1, d))   # :1145-1146
            t_n = t_n + dt32 * act.float().unsqueeze(1)              # :1148
            X_t_n = torch.cat([X, t_n], 1)                           # :1149
            K_count = K_count + torch.sum(act)                       # :1152
            if trace:
                tr["steps"] = tr.get("steps", 0) + act.long()
            stopped = stopped | (~new_sel & ~stopped)                # :1154-1155
        if cfg.loss_method == "diffusion":
            loss = loss + cfg.alpha[0] * torch.mean((V(X_t_n).squeeze() - Y) ** 2)   # :1163
        V.zero_grad()                                                # :1164
        out["K_log"].append(int(K_count))                            # :1168
        if cfg.loss_method == "BSDE":
            if not bounded:
                loss = loss + torch.mean((Y - problem.f(X)) ** 2)    # :1174
            elif btype == "Dirichlet":
                loss = loss + torch.mean((Y - problem.g(X, t_n.squeeze())) ** 2)     # :1176
            else:                                                    # 'Neumann', :1177-1183
                T_selection = (t_n > (T - dt32)).squeeze()           # :1178
                if torch.sum(T_selection) > 0:
                    loss = loss + torch.mean((Y[T_selection] - problem.f(X[T_selection, :])) ** 2)   # :1181
                if torch.sum(T_selection) < K:                       # :1182-1183: grad_V of the LAST executed step, final X, all K
                    loss = loss + torch.mean((torch.sum(grad_V * X, 1) - torch.sum(problem.g(X, t_n.squeeze()) * X, 1)) ** 2)
        if cfg.loss_with_stopped:                                    # :1185-1186
            loss = loss + torch.mean((Y[stopped] - problem.f(X[stopped, :])) ** 2)
        loss.backward()                                              # :1187
        if trace:
            tr["grads"] = [p.grad.detach().clone() for p in V.parameters()]
            tr["VN_minus_Y"] = None
            with torch.no_grad():                                    # per-trajectory end points of the rollout
                tr.update(Y_N=Y.detach().clone(), X_N=X.detach().clone(), t_N=t_n.detach().squeeze(1).clone(),
                          V_N=V(X_t_n).squeeze(1).clone())
        V.optim.step()                                               # :1188
        out["loss_log"].append(loss.item())                          # :1192
        if cfg.K_test_log is not None:                               # :1193-1197
            out["V_test_L2"].append(compute_test_error(V, problem, cfg.K_test_log, "parabolic")[0])
        if trace:
            out["traces"].append(tr)
    out["V"] = V
    return out


# --------------------------------------------------------------------------------------
# EllipticSolver.train restatement (reference solver.py:628-826): diffusion / BSDE loss, exit-time problems
# --------------------------------------------------------------------------------------
@dataclass
class EllipticConfig:
    K: int
    N: int
    delta_t: float
    lr: float = 0.001
    L: int = 1
    seed: int = 42
    K_boundary: int = 50
    alpha: tuple = (1.0, 1.0)
    loss_method: str = "diffusion"
    adaptive_forward_process: bool = False
    detach_forward: bool = True
    boundary_type: str = "Dirichlet"
    uniform_square: bool = False
    loss_with_stopped: bool = False
    K_test_log: Optional[int] = None
    sample_center: bool = False


def elliptic_build(problem: OracleProblem, cfg: EllipticConfig, arch=None, net=None):
    torch.manual_seed(cfg.seed)                                      # :604
    return value_net(problem.d, cfg.lr, cfg.seed, net=net, arch=arch)    # :606 (or the net the caller swaps in)


def elliptic_train(problem: OracleProblem, cfg: EllipticConfig, V=None, trace=False):
    """Restates EllipticSolver.train for loss_method in {'diffusion','BSDE'} on boundary in {'sphere','two_spheres','square',
    'square-corner'}."""
    if V is None:
        V = elliptic_build(problem, cfg)
    dt32 = torch.tensor(cfg.delta_t)                                 # :576
    sq_dt32 = torch.sqrt(dt32)                                       # :577
    K, d, ex = cfg.K, problem.d, problem.extra
    out = dict(loss_log=[], K_log=[], V_L2_log=[], traces=[], V_test_L2=[])
    torch.manual_seed(cfg.seed)                                      # :630
    np.random.seed(cfg.seed)                                         # :631
    for l in range(cfg.L):
        loss = 0
        if cfg.sample_center:                                        # :643-645
            X_center = torch.zeros(1, 1)
            loss = loss + torch.mean((V(X_center).squeeze() - ex["v_true"](X_center).squeeze()) ** 2)
        X_boundary = sample_boundary(problem, cfg.K_boundary)        # :650-680
        if cfg.loss_method != "BSDE":                                # :683 (boundary_loss=True)
            if cfg.boundary_type == "Dirichlet":
                loss = loss + cfg.alpha[1] * torch.mean((V(X_boundary).squeeze() - problem.g(X_boundary)) ** 2)   # :685
            else:
                loss = loss + cfg.alpha[1] * neumann_residual(V, X_boundary, problem.g(X_boundary), d)           # :687-693
        if ex["boundary"] == "sphere":
            if cfg.uniform_square:
                X = torch.rand(K, d) * 2 - 1                         # :697
                X = ex["boundary_distance"] * X / torch.sqrt(torch.sum(X ** 2, 1)).unsqueeze(1) * (torch.rand(K).unsqueeze(1))
            else:
                X = torch.randn(K, d)                                # :700
                X = ex["boundary_distance"] * X / torch.sqrt(torch.sum(X ** 2, 1)).unsqueeze(1) \
                    * (torch.rand(K).unsqueeze(1) ** (1 / d))        # :701
        elif ex["boundary"] == "two_spheres":
            if cfg.uniform_square:
                X = torch.rand(K, d) * 2 - 1                         # :703
                X = X / torch.sqrt(torch.sum(X ** 2, 1)).unsqueeze(1) * (
                    torch.rand(K, d) * (ex["boundary_distance_2"] - ex["boundary_distance_1"]) + ex["boundary_distance_1"])   # :704
            else:
                X = torch.randn(cfg.K, d)                            # :706 (K_original draws)
                X = ex["boundary_distance_2"] * X / torch.sqrt(torch.sum(X ** 2, 1)).unsqueeze(1) \
                    * (torch.rand(cfg.K).unsqueeze(1) ** (1 / d))    # :707
                selection = torch.sqrt(torch.sum(X ** 2, 1)) > ex["boundary_distance_1"]     # :708
                X = X[selection, :]                                  # :709
                K = int(torch.sum(selection))                        # :710
        else:
            X = (ex["X_r"] - ex["X_l"]) * torch.rand(K, d) + ex["X_l"]       # :713 / :707 ('square-corner')
            if ex["boundary"] == "square-corner":
                corner = torch.all(X > ex["X_corner"], 1)
                X[corner, :] = -X[corner, :]                         # :708
        X = X.clone().requires_grad_(True)                           # :718
        Y = V(X).squeeze()                                           # :721
        stopped = torch.zeros(K).bool()                              # :724
        V_L2 = torch.zeros(K)
        K_count = 0
        tr = dict(X0=X.detach().clone(), xi=[]) if trace else None
        if trace:
            tr["X_boundary"] = X_boundary.clone()
        for n in range(cfg.N):
            Y_ = V(X)                                                # :733
            Y_eval = Y_.squeeze().sum()
            Z, = torch.autograd.grad(Y_eval, X, create_graph=True)   # :736
            Z = torch.mm(problem.sigma(X).t(), Z.t()).t()            # :737
            xi = torch.randn(K, d)                                   # :739  (drawn BEFORE the all-stopped test)
            selection = ~stopped
            if torch.sum(selection) == 0:                            # :742-744
                break
            if trace:
                tr["xi"].append(xi.clone())
            V_L2[selection] += ((V(X[selection]).squeeze() - ex["v_true"](X[selection].detach()).float().squeeze()) ** 2
                                ).detach() * cfg.delta_t             # :746
            c = torch.zeros(d, K)                                    # :748
            if cfg.adaptive_forward_process:
                c = -Z.t()
            if cfg.detach_forward:
                c = c.detach()
            sel = selection.float().unsqueeze(1).repeat(1, d)
            X_prop = (X + ((problem.b(X) + torch.mm(problem.sigma(X), c).t()) * dt32
                           + torch.mm(problem.sigma(X), xi.t()).t() * sq_dt32) * sel)    # :754-755
            new_sel = exit_test(problem, X, X_prop, elliptic=True)   # :758-767
            act = new_sel & ~stopped
            Y = (Y + ((-problem.h(X, Y_.squeeze(), Z) + torch.sum(Z * c.t(), 1)) * dt32
                      + torch.sum(Z * xi, 1) * sq_dt32) * act.float())        # :776-777
            X = (X * (~new_sel | stopped).float().unsqueeze(1).repeat(1, d)
                 + X_prop * act.float().unsqueeze(1).repeat(1, d))   # :780-781
            K_count = K_count + torch.sum(act)                       # :784
            if trace:
                tr["steps"] = tr.get("steps", 0) + act.long()
            stopped = stopped | (~new_sel & ~stopped)                # :786-787
        if cfg.loss_method == "diffusion":
            loss = loss + cfg.alpha[0] * torch.mean((V(X).squeeze() - Y) ** 2)   # :799
        out["K_log"].append(int(K_count))                            # :803
        if cfg.loss_method == "BSDE":
            loss = loss + torch.mean((problem.g(X) - Y) ** 2)        # :808
        if cfg.loss_with_stopped:                                    # :803-804
            loss = loss + torch.mean((problem.g(X[stopped, :]) - Y[stopped]) ** 2)
        V.zero_grad()                                                # :813
        loss.backward()                                              # :814
        if trace:
            tr["grads"] = [p.grad.detach().clone() for p in V.parameters()]
            with torch.no_grad():
                tr.update(Y_N=Y.detach().clone(), X_N=X.detach().clone(), V_N=V(X).squeeze(1).clone())
        V.optim.step()                                               # :815
        out["loss_log"].append(loss.item())                          # :819
        out["V_L2_log"].append(torch.mean(V_L2).item())              # :820
        if cfg.K_test_log is not None:                               # :821-825
            out["V_test_L2"].append(compute_test_error(V, problem, cfg.K_test_log, "elliptic")[0])
        if trace:
            out["traces"].append(tr)
    out["V"] = V
    return out


def fingerprint(module):
    res = []
    for name, p in module.named_parameters():
        q = p.detach().to(torch.float64)
        res.append(dict(name=name, shape=list(p.shape), sum=float(q.sum()), abs_sum=float(q.abs().sum()),
                        head=[float(v) for v in p.detach().reshape(-1)[:4].tolist()]))
    return res
