"""Float64 restatements for the tests of utilities.loss_relative_errors and of psp_loss_stats_*:

  numpy_statistics   every statistic of the function's table in numpy float64 on fp32 (Y, D), with the scale each bound is
                     stated in (the mean absolute value of the centred terms that were summed);
  assert_statistics  |got - ref| <= 1e-10 s for every output;
  rollout64          the update rule of the function's docstring in float64 torch on given draws, for every control kind.
"""
import copy

import numpy as np
import torch

KEYS = ("terminal", "cross_entropy", "cross_entropy_detach", "cross_entropy_detach_selection", "log_variance", "moment")
# A sequential double sum of n terms is wrong by at most n 2^-53 sum|terms| = 1.1e-11 s at n = 1e5, with s the mean absolute
# term; a double exp adds a few ulp.  1e-10 leaves a factor of about 9.
BOUND = 1e-10


def numpy_statistics(Y32, D32):
    """({key: (mean, variance, relative error)}, the selection's count, {key: (s of the mean, s of the variance)})."""
    y, D = np.asarray(Y32).astype(np.float64), np.asarray(D32).astype(np.float64)
    g = y - D
    n = y.size
    with np.errstate(all="ignore"):
        v = {"terminal": np.exp(-g), "cross_entropy": y * np.exp(-g), "cross_entropy_detach": y * np.exp(-g + y), "moment": D * D}
        v["cross_entropy_detach_selection"] = v["cross_entropy_detach"][np.abs(v["cross_entropy_detach"]) < 100.0]
        out, scale = {}, {}
        for key, s in v.items():
            m = s.mean() if s.size else np.nan
            c2 = (s - m) ** 2
            var = c2.sum() / (s.size - 1.0)
            out[key] = (m, var, np.sqrt(var) / abs(m))
            scale[key] = (np.abs(s).mean() if s.size else 0.0, c2.mean() if s.size else 0.0)
        c = D - D.mean()
        var = (c ** 2).sum() / (n - 1.0)
        vv = (c ** 4).mean() - var ** 2
        out["log_variance"] = (var, vv, np.sqrt(vv) / abs(var))
        scale["log_variance"] = ((c ** 2).mean(), (c ** 4).mean())
    return out, int(v["cross_entropy_detach_selection"].size), scale


def _close(got, ref, tol):
    if not np.isfinite(ref):                 # a non-finite sample is not filtered: NaN stays NaN, an infinite mean keeps its sign
        return np.isnan(got) if np.isnan(ref) else got == ref
    return abs(got - ref) <= tol


def assert_statistics(got, ref, scale, tag="", other=None):
    """got: {key: (mean, variance, ..)} against numpy_statistics' ref under BOUND * s.  `other`: a second result (another split
    of the same samples) that may differ from `got` by rounding only -- twice the bound.  Returns the worst error / s."""
    worst = 0.0
    for key in KEYS:
        for j, what in enumerate(("mean", "variance")):
            s = scale[key][j]
            assert _close(got[key][j], ref[key][j], BOUND * s), (tag, key, what, got[key][j], ref[key][j], s)
            if other is not None:
                assert _close(other[key][j], got[key][j], 2 * BOUND * s), (tag, key, what, other[key][j], got[key][j], s)
            if s > 0 and np.isfinite(s) and np.isfinite(ref[key][j]):
                worst = max(worst, abs(got[key][j] - ref[key][j]) / s)
        # r = sqrt(variance) / |mean| of two numbers held to the bound: |dr| <= r (dvar / (2 var) + dmean / |mean|), and an ulp or two
        m_ref, v_ref, r_ref = ref[key]
        if np.isnan(r_ref):
            assert np.isnan(got[key][2]), (tag, key, got[key][2])
        elif np.isfinite(r_ref) and v_ref > 0:
            tol = r_ref * (BOUND * scale[key][1] / (2 * v_ref) + BOUND * scale[key][0] / abs(m_ref) + 1e-15)
            assert abs(got[key][2] - r_ref) <= tol, (tag, key, "relative_error", got[key][2], r_ref, tol)
    return worst


def rollout64(problem, control, xi, delta_t, adaptive):
    """(Y_N, D = Y_N - g(X_N)) in float64 for draws xi (N, K, d): per step Z = control(t_n, X_n) with the fp32 time feature
    n * delta_t, c = -Z or 0, X += (b(X) + sigma c) dt + sigma xi sqrt(dt), Y += (|Z|^2 / 2 + f(X_{n+1}) + Z . c) dt + Z . xi sqrt(dt).
    dt and sqrt(dt) are the fp32 numbers the kernels are handed, in double."""
    N, K, d = xi.shape
    xi = xi.double().cpu()
    dt32 = torch.tensor(delta_t, dtype=torch.float32)
    dt, sq = float(dt32), float(torch.sqrt(dt32))
    if hasattr(control, "z_n"):
        z, outer = control.z_n, control.time_approx == "outer"
    else:
        z, outer = control, isinstance(control, (list, tuple))
    nets = [copy.deepcopy(m).cpu().double() for m in (z if outer else [z])]
    prob = copy.copy(problem)
    for name in ("A", "B", "alpha", "X_0", "P", "Q", "R"):
        if hasattr(prob, name) and torch.is_tensor(getattr(prob, name)):
            setattr(prob, name, getattr(prob, name).detach().cpu().double())
    X = prob.X_0.repeat(K, 1)
    Y = torch.zeros(K, dtype=torch.float64)
    with torch.no_grad():
        for n in range(N):
            tn = float(torch.tensor(float(n), dtype=torch.float32) * dt32)
            Z = nets[n](X) if outer else nets[0](torch.cat([torch.full((K, 1), tn, dtype=torch.float64), X], 1))
            c = -Z if adaptive else torch.zeros_like(Z)
            B = prob.sigma(X)
            X = X + (prob.b(X) + c @ B.t()) * dt + (xi[n] @ B.t()) * sq
            Y = Y + (0.5 * (Z * Z).sum(1) + prob.f(X, tn).double() + (Z * c).sum(1)) * dt + (Z * xi[n]).sum(1) * sq
        D = Y - prob.g(X)
    return Y, D
