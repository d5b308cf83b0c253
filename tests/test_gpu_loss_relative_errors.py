"""utilities.loss_relative_errors on the GPU: per-trajectory parity of the chunked native plan with the update rule restated in
float64 (ref64_loss_relerr.rollout64) on the same draws, the statistics against float64 numpy on the returned samples, and
the chunking.

Parity bound: max|delta| <= 1e-4 max(1, max|ref|), the project's bar for the forward kernels.
Statistics bound: that of tests/test_gpu_loss_stats.py, 1e-10 of the mean absolute centred term.
The nets are the untrained nets with their weights scaled up and random biases, so that Z is O(1) and the relu(.)**2 / tanh
layers leave their linear regime (the untrained DenseNet's Z is ~1e-3)."""
import numpy as np
import pytest
import torch

import ref64_loss_relerr as r64
from util_cases import psp

U = psp.utilities
pytestmark = pytest.mark.gpu

DELTA_T, N, K = 0.125, 8, 256
PARITY = 1e-4                 # measured worst over the 32 cases below on an MI355X: 5.2e-7


def dev():
    return torch.device("cuda:0")


def boost_dense(net, seed, scale):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for w in net.W:
            if w.dim() == 2:
                w.mul_(scale)
            else:
                w.copy_(0.3 * torch.randn(w.shape, generator=gen))
    return net


def make_control(kind, problem, d, scale=1.5):
    if kind == "dense_inner":
        return boost_dense(psp.DenseNet(d + 1, d, lr=0.05, seed=11), 12, scale).to(dev())
    if kind == "mlp":
        net = psp.MySequential(d + 1, d, lr=0.05, seed=5)
        gen = torch.Generator().manual_seed(6)
        with torch.no_grad():
            for p in net.parameters():
                p.copy_((0.3 if p.dim() == 2 else 0.1) * torch.randn(p.shape, generator=gen))
        return net.to(dev())
    if kind == "dense_outer":
        return [boost_dense(psp.DenseNet(d, d, lr=0.05, seed=40 + n), 60 + n, scale).to(dev()) for n in range(N)]
    model = psp.Solver("lre", problem, lr=1e-3, L=1, K=16, delta_t=DELTA_T, time_approx="outer", u_l2_error_flag=False,
                       verbose=False, seed=3, device=dev())
    assert len(model.z_n) == N
    for n, net in enumerate(model.z_n):
        boost_dense(net, 80 + n, scale)
    return model


@pytest.mark.parametrize("kind", ["dense_inner", "mlp", "dense_outer", "solver"])
@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("d", [1, 3, 15, 16])
def test_native_rollout_matches_float64_per_trajectory(d, adaptive, kind):
    problem = psp.LLGC(d=d, off_diag=0.1, T=1, seed=7, device=dev())
    control = make_control(kind, problem, d)
    out = U.loss_relative_errors(problem, control, K, delta_t=DELTA_T, adaptive_forward_process=adaptive, noise="reference",
                                 seed=21, backend="native", chunk=96, return_samples=True)
    assert out["plan"] == "native" and out["plan_reason"] is None and out["K"] == K and out["N"] == N and out["chunk"] == 96
    torch.manual_seed(21)                                               # the draws the call made
    xi = torch.stack([torch.randn(K, d) for _ in range(N)])
    Yr, Dr = r64.rollout64(problem, control, xi, DELTA_T, adaptive)
    Y, D = out["Y"].double().cpu(), out["D"].double().cpu()
    assert float(Dr.abs().max()) < 100.0 and float(Yr.abs().max()) > 0.05    # a conditioned case that does exercise the control
    gy = float((Y - Yr).abs().max()) / max(1.0, float(Yr.abs().max()))
    gd = float((D - Dr).abs().max()) / max(1.0, float(Dr.abs().max()))
    print("d=%d adaptive=%s %s: max|dY| %.2e  max|dD| %.2e of max(1, max|ref|)  (bound %.0e)" % (d, adaptive, kind, gy, gd, PARITY))
    assert gy <= PARITY and gd <= PARITY
    # the same call's statistics are the float64 statistics of the samples it returned
    ref, count, scale = r64.numpy_statistics(out["Y"].cpu().numpy(), out["D"].cpu().numpy())
    assert out["cross_entropy_detach_selection"][3] == count
    r64.assert_statistics(out, ref, scale, tag="%s d=%d" % (kind, d))


def test_chunking_does_not_change_a_trajectory():
    """noise='philox', K = 1000 (62.5 tiles), d = 3: the smallest chunk, about K / 3 and one chunk give the same samples bit for
    bit and statistics within the bound; exactly K trajectories are counted, and the selection's count is that of the samples."""
    d, Kc = 3, 1000
    problem = psp.LLGC(d=d, off_diag=0.1, T=1, seed=7, device=dev())
    net = make_control("dense_inner", problem, d, scale=2.5)                 # spreads |Y exp(-g + Y)| to either side of 100
    runs = [U.loss_relative_errors(problem, net, Kc, delta_t=DELTA_T, noise="philox", seed=5, backend="native", chunk=c,
                                   return_samples=True) for c in (None, 16, Kc // 3)]
    assert [r["chunk"] for r in runs] == [1008, 16, 336] and all(r["K"] == Kc and r["plan"] == "native" for r in runs)
    ref, count, scale = r64.numpy_statistics(runs[0]["Y"].cpu().numpy(), runs[0]["D"].cpu().numpy())
    v = np.abs(runs[0]["Y"].double().cpu().numpy() * np.exp(runs[0]["D"].double().cpu().numpy()))
    print("selected %d of %d, nearest to 100: %.3g" % (count, Kc, np.abs(v - 100.0).min()))
    assert 0 < count < Kc and np.abs(v - 100.0).min() > 1e-6
    for r in runs:
        assert r["Y"].shape == (Kc,) and torch.equal(r["Y"], runs[0]["Y"]) and torch.equal(r["D"], runs[0]["D"])
        assert r["cross_entropy_detach_selection"][3] == count
        r64.assert_statistics(r, ref, scale, tag="chunk %s" % r["chunk"], other=runs[0])
    again = U.loss_relative_errors(problem, net, Kc, delta_t=DELTA_T, noise="philox", seed=5, backend="native", chunk=16)
    assert all(again[key] == runs[1][key] for key in U.LRE_KEYS)             # equal calls, equal bits
    other = U.loss_relative_errors(problem, net, Kc, delta_t=DELTA_T, noise="philox", seed=6, backend="native", return_samples=True)
    assert not torch.equal(other["Y"], runs[0]["Y"])                         # the seed does key the noise


def test_composite_plan_on_the_gpu_sees_the_kernels_noise():
    """backend='torch' on the GPU draws the kernels' Philox stream (psp_philox_normal_fill), so it is the native plan's rollout in
    fp32 torch: per trajectory within the parity bar, statistics from the same device kernels."""
    d, Kc = 3, 1000
    problem = psp.LLGC(d=d, off_diag=0.1, T=1, seed=7, device=dev())
    net = make_control("dense_inner", problem, d)
    kw = dict(delta_t=DELTA_T, adaptive_forward_process=True, noise="philox", seed=9, return_samples=True)
    nat_run = U.loss_relative_errors(problem, net, Kc, backend="native", **kw)
    tor_run = U.loss_relative_errors(problem, net, Kc, backend="torch", chunk=300, **kw)
    assert tor_run["plan"] == "torch" and tor_run["plan_reason"] == "backend='torch' requested" and tor_run["chunk"] == 304
    for key in ("Y", "D"):
        gap = float((nat_run[key] - tor_run[key]).abs().max()) / max(1.0, float(tor_run[key].abs().max()))
        print("%s: native against fp32 torch %.2e" % (key, gap))
        assert gap <= PARITY
    ref, count, scale = r64.numpy_statistics(tor_run["Y"].cpu().numpy(), tor_run["D"].cpu().numpy())
    r64.assert_statistics(tor_run, ref, scale, tag="torch plan")
