"""Float64 statement of the h kinds and closed-form solutions of the exit-time and box problems (include/psp.h PSP_GH_AFFINE_EXP,
PSP_GH_SINE_SOURCE, PSP_GH_SINNORM2; PSP_VTRUE_LOGQ / _SINPROD / _SINSUM / _SINR2), written from the header's formulas and a
problem's ``general_native_spec()`` / ``native_vtrue_spec()`` alone -- not from the class's ``h`` / ``v_true`` -- and one training
iteration of EllipticSolver on them in float64 through tests/ref64_general.py's ``iteration``.

  h64(spec)            h(t, x, y, z) in float64 from (h, h_par)
  vtrue64(vt)          v_true(x) in float64 from (kind, par)
  coeffs64(prob)       what ref64_general.iteration asks of a problem: d, B, drift, h, f, g
  draws(case)          the host draws of the first iteration in the order EllipticSolver.train makes them (boundary batch, domain
                       batch, N times xi), from a CPU twin of the solver
  iteration(...)       ref64_general.iteration on these coefficients

pi is the fp32 value the classes hold (``torch.tensor(np.pi)``) and the kernels' constant, and the source coefficients built
from it -- (a pi)^2, (a pi)^2 0.1, 4 pi^2, 2 d pi -- are the fp32 numbers the classes form as zero-dimensional fp32 tensors
before they meet the data (``_f32mul``): they are constants of the problem, so both sides differ from this statement by the
rounding of their own arithmetic alone."""
import types

import numpy as np
import torch

import ref64_general as r64
from util_cases import psp

F64 = torch.float64
PI32 = float(np.float32(np.pi))
nat = psp.native


def _f32mul(*vs):
    """The product of the values as fp32 arithmetic forms it, left to right."""
    out = np.float32(vs[0])
    for v in vs[1:]:
        out = np.float32(out * np.float32(v))
    return float(out)


def h64(spec):
    kind, p = spec["h"], [float(v) for v in spec.get("h_par", (0.0, 0.0, 0.0, 0.0))]
    if kind == nat.GH_AFFINE_EXP:
        return lambda t, x, y, z: p[0] + p[1] * y + p[2] * (z ** 2).sum(1) + p[3] * torch.exp(-y)
    if kind == nat.GH_SINE_SOURCE:
        if p[0] == 0.0:
            def helm(t, x, y, z):
                S = torch.sin(p[1] * x[:, 0]) * torch.sin(p[2] * x[:, 1])
                return p[3] * y + (_f32mul(p[1], p[1]) + _f32mul(p[2], p[2]) - p[3]) * S
            return helm
        return lambda t, x, y, z: (_f32mul(p[1], p[1]) * torch.sin(p[1] * x[:, 0])
                                   + _f32mul(p[2], p[2], p[3]) * torch.sin(p[2] * x[:, 0]))
    if kind == nat.GH_SINNORM2:
        al, d, linear = p[0], p[1], p[2] != 0.0

        def sn(t, x, y, z):
            r2, sx = (x ** 2).sum(1), x.sum(1)
            fp2 = 4 * _f32mul(PI32, PI32)
            src = -_f32mul(2 * d, PI32) * torch.cos(PI32 * r2)
            if linear:
                return al ** 2 * (fp2 * torch.sin(PI32 * r2) * sx ** 2 + src)
            return al ** 2 * (fp2 * y * sx ** 2 + src + torch.sin(PI32 * r2) ** 2 - y ** 2)
        return sn
    if kind == nat.GH_QUAD:
        return lambda t, x, y, z: -0.5 * (z ** 2).sum(1)
    if kind == nat.GH_ZERO:
        return lambda t, x, y, z: torch.zeros(x.shape[0], dtype=F64)
    raise ValueError("h kind %r is stated in ref64_general.py" % kind)


def vtrue64(vt):
    kind, p = vt["kind"], [float(v) for v in vt["par"]]
    if kind == nat.VTRUE_LOGQ:
        return lambda x: torch.log(((x ** 2).sum(1) + 1.0) / p[0])
    if kind == nat.VTRUE_SINPROD:
        return lambda x: torch.sin(p[0] * x[:, 0]) * torch.sin(p[1] * x[:, 1])
    if kind == nat.VTRUE_SINSUM:
        return lambda x: torch.sin(p[0] * x[:, 0]) + p[2] * torch.sin(p[1] * x[:, 0])
    if kind == nat.VTRUE_SINR2:
        return lambda x: torch.sin(PI32 * (x ** 2).sum(1))
    raise ValueError("v_true kind %r" % kind)


def coeffs64(prob):
    spec = prob.general_native_spec()
    d = prob.d
    B = spec["sigma"] if spec.get("sigma") is not None else float(spec["sigma_scale"]) * torch.eye(d)
    co = dict(d=d, B=torch.as_tensor(B).detach().cpu().to(F64), drift=None, h=h64(spec),
              f=lambda x: torch.zeros(x.shape[0], dtype=F64), g=lambda x, t=None: prob.g(x).to(F64))
    if spec["drift"][0] == nat.DRIFT_DOUBLE_WELL:
        kappa = spec["drift"][1].detach().cpu().to(F64)
        co["drift"] = lambda x: -4.0 * kappa * x * (x ** 2 - 1.0)
    else:
        assert spec["drift"][0] == nat.DRIFT_ZERO
    return co


def shim(prob):
    """The attributes ref64_general.iteration reads off an oracle problem."""
    extra = dict(boundary=prob.boundary)
    for k in ("boundary_distance", "X_l", "X_r", "one_boundary"):
        if hasattr(prob, k):
            extra[k] = getattr(prob, k)
    return types.SimpleNamespace(kind=type(prob).__name__, d=prob.d, extra=extra, B=prob.B.detach().cpu(), T=None)


def draws(model):
    """The first iteration's host draws of a (CPU) EllipticSolver, in the order train() makes them."""
    torch.manual_seed(model.seed)
    np.random.seed(model.seed)
    Xb = model._sample_boundary()
    X0 = model.sample_domain()
    xi = [torch.randn(model.K, model.d) for _ in range(model.N)]
    return dict(X_boundary=Xb.detach().clone(), X0=X0.detach().clone(), xi=xi)


def iteration(case, prob, net, dr):
    co = coeffs64(prob)
    case = dict(case, solver=dict(dict(alpha=[1.0, 1.0]), **case["solver"]))      # EllipticSolver's default weights
    keep = r64.coeffs64
    r64.coeffs64 = lambda case_, oprob_: co           # (iteration() asks the module for the coefficients of its oracle problem)
    try:
        return r64.iteration(case, shim(prob), net, dr)
    finally:
        r64.coeffs64 = keep
