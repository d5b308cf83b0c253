"""tests/ref64_gradvar.py, the float64 reference of the gradient-variance diagnostic: its streamed pre-activation-gradient form
equals the literal definition (K separate autograd.grad calls per step, row-0 Gg), and the regime of tests/dense_block_cases.py
leaves every block of every parameter set with a non-zero variance -- so the per-block GPU tests compare signal, not zeros."""
import pytest
import torch

import dense_block_cases as dc
import gradvar_cases as gc
import ref64_gradvar as r64


def _rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


@pytest.mark.parametrize("loss", ["moment", "log-variance"])
@pytest.mark.parametrize("adaptive", [False, True], ids=["nonadaptive", "attached"])
def test_streamed_moments_equal_the_literal_definition(loss, adaptive):
    d, H, K, N = 3, 4, 5, 3
    c = gc.block_case(d, H, K, N, (16, 32), loss=loss, adaptive=adaptive)
    oprob, ocfg, nets = dc.scaled_oracle(c)
    noise = dc.host_noise(42, K, d, N)
    w = torch.randn(K, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    got = r64.moments(oprob, ocfg, nets, noise, weights=[w])
    lit = r64.literal(oprob, ocfg, nets, noise)
    assert float(lit["grads_var"].abs().max()) > 0 and float(lit["grads_mean"].abs().max()) > 0
    assert _rel(got["grads_mean"], lit["grads_mean"]) <= 1e-12
    assert _rel(got["grads_var"], lit["grads_var"]) <= 1e-12
    if adaptive:
        assert float(lit["Gg"].abs().max()) > 0 and _rel(got["Gg"], lit["Gg"]) <= 1e-12
    else:
        assert float(got["Gg"].abs().max()) == 0.0 and float(lit["Gg"].abs().max()) == 0.0
    # S[c], Q[c] against per-trajectory gradients from autograd
    ro = r64.rollout(oprob, ocfg, nets, noise)
    for n in range(N):
        G = torch.stack([torch.cat([g.reshape(-1) for g in torch.autograd.grad(ro["Y"][k], ro["sets"][n], retain_graph=True)])
                         for k in range(K)])
        assert _rel(got["S"][0][n], (w[:, None] * G).sum(0)) <= 1e-12
        assert _rel(got["Q"][0][n], ((w[:, None] * G) ** 2).sum(0)) <= 1e-12


# (the K = 9001 shape is used by the kernel test only: non-adaptive images)
REGIME = [(s, a) for s in gc.KERNEL_SHAPES for a in (False, True) if not (a and s[2] > 1000)]


@pytest.mark.parametrize("shape,adaptive", REGIME,
                         ids=["d%d-H%d-K%d-N%d-%s" % (s[:4] + ("attached" if a else "nonadaptive",)) for s, a in REGIME])
def test_every_block_has_variance(shape, adaptive):
    d, H, K, N, expect = shape
    for loss in ("moment", "log-variance"):
        c = gc.block_case(d, H, K, N, expect, loss=loss, adaptive=adaptive)
        oprob, ocfg, nets = dc.scaled_oracle(c)
        ref = r64.moments(oprob, ocfg, nets, dc.host_noise(42, K, d, N))
        assert gc.variance_blocks_alive(ref["grads_var"], d, H, N), (loss, adaptive)
