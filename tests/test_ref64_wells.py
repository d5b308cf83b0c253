"""tests/ref64_wells.py without a GPU: its coefficient closures against the classes they restate, the Jacobian formulas the adjoint
kernel uses against autograd, and the regime of every case of tests/wells_cases.py -- every gradient block of every per-step net
carries signal, and on the attached cases the gradient moves by at least 100 x BLOCK_TOL when the drift Jacobian is dropped (an
attached case whose gradient ignores b' would prove nothing about it).  Every case of the table is checked (the float64 reference
is cached per shape and flags: the matrix mode costs nothing).  The Philox cases are checked on the host stream of the same seed:
the device stream cannot be materialised without a GPU, and the regime is a property of the problem, the nets and the flags, with
N(0, 1) increments of either stream."""
import pytest
import torch

import dense_block_cases as dc
import ref64_wells as rw
import wells_cases as wc
from test_gpu_dense_block_gradients import BLOCK_TOL          # (its tests are marked gpu; the module itself imports without one)
from util_cases import dense_block_errors, dense_grad_blocks, psp

F64 = torch.float64


@pytest.mark.parametrize("make", [lambda: psp.DoubleWell_OU(d=6, T=0.2, alpha=0.7, kappa=1.5, device="cpu"),
                                  lambda: psp.DoubleWell_multidim_2(d=5, T=0.2, alpha=0.7, kappa=1.5, device="cpu"),
                                  lambda: psp.DoubleWell_multidim_3(d=4, T=0.2, eta=0.7, kappa=1.5, device="cpu")])
def test_closures_restate_the_classes(make):
    pb = make()
    b, g = rw.coefficients(pb.native_spec(), pb.d)
    x = 1.5 * torch.randn(40, pb.d, generator=torch.Generator().manual_seed(2))
    eb = (b(x.double()) - pb.b(x).double()).abs().max() / pb.b(x).abs().max()
    eg = (g(x.double()) - pb.g(x).double()).abs().max() / pb.g(x).abs().max()
    assert float(eb) < 2e-6 and float(eg) < 2e-6, (float(eb), float(eg))


def test_radial_jacobian_formula():
    """b'^T l = -(phi / r) l - ((phi' - phi / r) / r^2) (x . l) x with phi' = 4 kappa (3 (r - r0)^2 - w): what hjbd_adj_kernel forms."""
    pb = psp.DoubleWell_multidim_2(d=7, T=0.2, alpha=1.0, kappa=0.8, device="cpu")
    b, _ = rw.coefficients(pb.native_spec(), pb.d)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(9, 7, generator=gen, dtype=F64).requires_grad_(True)
    lam = torch.randn(9, 7, generator=gen, dtype=F64)
    (auto,) = torch.autograd.grad((b(x) * lam).sum(), x)
    kappa, r0, w = (float(v) for v in pb.native_spec()["drift"][1])      # (kappa as the fp32 number the kernels get)
    xd = x.detach()
    r = xd.norm(dim=1, keepdim=True)
    s = r - r0
    phi, dphi = 4 * kappa * s * (s ** 2 - w), 4 * kappa * (3 * s ** 2 - w)
    want = -(phi / r) * lam - ((dphi - phi / r) / r ** 2) * (xd * lam).sum(1, keepdim=True) * xd
    assert torch.allclose(auto, want, rtol=1e-10, atol=1e-10)      # float64 rounding of two orders of evaluation


def test_well_diag_jacobian_formula():
    spec = dict(drift=(psp.native.DRIFT_WELL_DIAG, torch.tensor([0.7, 1.3, -2.0, -5.0])), sigma=(psp.native.SIGMA_IDENTITY, None, 1.0),
                runcost=(psp.native.RUNCOST_ZERO, None), term=(psp.native.TERM_QUAD_LINEAR, torch.ones(4)), split=2)
    b, g = rw.coefficients(spec, 4)
    x = torch.randn(5, 4, generator=torch.Generator().manual_seed(1), dtype=F64).requires_grad_(True)
    (auto,) = torch.autograd.grad(b(x).sum(), x)
    xd, c = x.detach(), spec["drift"][1].double()
    want = torch.cat([-4 * c[:2] * (3 * xd[:, :2] ** 2 - 1), c[2:].expand(5, 2)], 1)
    assert torch.allclose(auto, want, rtol=1e-10, atol=1e-10)      # float64 rounding of two orders of evaluation
    (gg,) = torch.autograd.grad(g(x).sum(), x)
    assert torch.allclose(gg, torch.cat([2 * (xd[:, :2] - 1), torch.ones(5, 2, dtype=F64)], 1))


@pytest.mark.parametrize("c", wc.CASES, ids=wc.IDS)
def test_regime_of_the_gpu_cases(c):
    noise = lambda: dc.host_noise(42, c["K"], c["d"], c["N"])
    ref = wc.reference(c, noise, stream="host-stand-in")
    assert bool(torch.isfinite(ref["grad"]).all()) and bool(torch.isfinite(ref["D"]).all())
    assert float(ref["r"].min()) > 0.05                       # (radial kinds: no trajectory near the origin)
    for s, blocks in enumerate(dense_grad_blocks(ref["grad"], c["d"], c["H"], c["N"], False)):
        top = max(float(b.abs().max()) for b in blocks)
        assert top > 0
        for b in blocks:                                       # every block above the floor that dense_block_errors would apply
            assert float(b.abs().max()) > 1e-3 * top, (c["id"], s)
    if c["adaptive"] and not c["detach"] and c["N"] > 1:       # (N = 1: X_0 is fixed, so b'(X_0) never meets a gradient)
        dropped = wc.reference(c, noise, jacobian=False, stream="host-stand-in")
        errs = dense_block_errors(dropped["grad"], ref["grad"], c["d"], c["H"], c["N"], False)
        worst = max(max(es) for es in errs[:-1])               # (the last step's net sees no later drift)
        assert worst >= 100 * BLOCK_TOL, (c["id"], worst)
