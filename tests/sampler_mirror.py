"""float64 numpy mirror of the device test log's point sampler (include/psp.h, psp_genl_eval_config), written from the counter
definition: Philox4x32-7, key (seed & 0xffffffff, (seed >> 32) ^ 0x54455354), counter (k_offset + k, c1, c2, iter);
c1 = 0, c2 = 4 b + q gives features 16 b + 4 r + q (normals for the ball kinds, 24-bit uniforms for the box), c1 = 1, c2 = 0
gives the radial uniform (output 0) and the time uniform (output 1).  Shared by the CPU and the GPU tests of the test log;
also the float64 closed forms of v_true by kind."""
import numpy as np

from oracle import philox_oracle as ph

BALL, ANNULUS, BOX = 1, 2, 3
VT_EXP, VT_QUAD, VT_COMMITTOR = 0, 1, 2
KEY_XOR = 0x54455354


def _uniform(r):
    return ((r >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def sample(kind, d, K, bound_a, bound_b, T=1.0, seed=42, iteration=0, k_offset=0):
    """dict(x (K, d), t (K), keep (K) bool, gnorm (K) |g| of the normals (ball kinds), radius (K) |x|)."""
    k0 = seed & 0xFFFFFFFF
    k1 = ((seed >> 32) & 0xFFFFFFFF) ^ KEY_XOR
    k = ((np.arange(K, dtype=np.uint64) + np.uint64(k_offset)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    nb = (d + 15) // 16
    feat = np.zeros((K, 16 * nb))
    for b in range(nb):
        for q in range(4):
            r = ph.philox4x32(k, np.uint32(0), np.uint32(4 * b + q), np.uint32(iteration), k0, k1)
            vals = [_uniform(ri) for ri in r] if kind == BOX else ph.normal4(*r)
            for rr in range(4):
                feat[:, 16 * b + 4 * rr + q] = vals[rr]
    g = feat[:, :d]
    ru = ph.philox4x32(k, np.uint32(1), np.uint32(0), np.uint32(iteration), k0, k1)
    u, ut = _uniform(ru[0]), _uniform(ru[1])
    gnorm = np.sqrt(np.sum(g ** 2, 1))
    if kind == BOX:
        x = (bound_b - bound_a) * g + bound_a
    else:
        x = bound_b * g / gnorm[:, None] * (u ** (1.0 / d))[:, None]
    radius = np.sqrt(np.sum(x ** 2, 1))
    keep = radius > bound_a if kind == ANNULUS else np.ones(K, dtype=bool)
    return dict(x=x, t=ut * T, keep=keep, gnorm=gnorm, radius=radius)


def v_true(kind, par, x, t=None):
    """The closed forms of PSP_VTRUE_* in float64."""
    x = np.asarray(x, dtype=np.float64)
    r2 = np.sum(x ** 2, 1)
    t = np.zeros(x.shape[0]) if t is None else np.asarray(t, dtype=np.float64)
    p = [float(v) for v in par]
    if kind == VT_EXP:
        return np.exp(p[0] * r2 + p[1] * t)
    if kind == VT_QUAD:
        return r2 + p[0] * (p[1] - t)
    a, c, d = p[0], p[1], p[2]
    return (a ** 2 - np.sqrt(r2) ** (2 - d) * a ** d) / (a ** 2 - c ** (2 - d) * a ** d)
