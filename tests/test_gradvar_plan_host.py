"""Host side of the native gradient-variance diagnostic (plan_dense_native.py), no GPU: the combination psp_gradvar_finish applies
(its torch mirror gradvar_combine, which the GPU test holds the kernel to) and the eligibility table of compute_gradient_variance > 0."""
import math

import pytest
import torch

from util_cases import psp

pdn = psp.plan_dense_native
F64 = torch.float64


def _sums(G, c):
    return (c[:, None] * G).sum(0), ((c[:, None] * G) ** 2).sum(0), ((c * c)[:, None] * G).sum(0), G.sum(0)


@pytest.mark.parametrize("loss,with_gg", [("moment", False), ("moment", True), ("log-variance", True)])
def test_combination_reproduces_the_per_sample_definition(loss, with_gg):
    gen = torch.Generator().manual_seed(5)
    K, p = 23, 40
    G = torch.randn(K, p, generator=gen, dtype=F64)
    r = torch.randn(K, generator=gen, dtype=F64) + 0.3
    Gg = torch.randn(p, generator=gen, dtype=F64) if with_gg else torch.zeros(p, dtype=F64)
    if loss == "moment":
        c = r
        f = 2 * r[:, None] * (G - Gg)
    else:
        c = r - r.mean()
        A = G - Gg
        f = 2 * c[:, None] * (A - A.mean(0, keepdim=True))
    S, Q, S2, S1 = _sums(G, c)
    mean, var, rel, scalar = pdn.gradvar_combine(S, Q, S2 if (with_gg or loss != "moment") else None, S1,
                                                 Gg if (with_gg and loss == "moment") else None, K, loss, float(c.sum()),
                                                 float((c * c).sum()))
    assert mean.dtype == var.dtype == rel.dtype == torch.float32
    assert torch.allclose(mean.double(), f.mean(0), rtol=1e-6, atol=0)
    assert torch.allclose(var.double(), f.var(0), rtol=1e-6, atol=0)
    want = torch.sqrt(f.var(0)) / f.mean(0)
    assert torch.allclose(rel.double(), want, rtol=1e-5, atol=0)
    assert math.isclose(float(scalar), float(rel.double().mean()), rel_tol=1e-6)


def test_combination_special_values():
    K = 4.0
    # entry 0: a dead unit, every sum 0 -> 0 / 0 = NaN -> 0
    # entry 1: mean exactly 0 with a positive variance -> inf, kept
    # entry 2: a negative mean stays negative
    # entry 3: raw moments that round to a slightly NEGATIVE variance (sum f^2 < (sum f)^2 / K): clamped to 0 before the root
    S = torch.tensor([0.0, 0.0, -2.0, 2.0], dtype=F64)
    Q = torch.tensor([0.0, 3.0, 5.0, 4.0 / K * (1 - 1e-9)], dtype=F64)
    mean, var, rel, scalar = pdn.gradvar_combine(S, Q, None, None, None, K, "moment", 1.0, 1.0)
    assert float(rel[0]) == 0.0 and float(var[0]) == 0.0 and float(mean[0]) == 0.0
    assert math.isinf(float(rel[1])) and float(rel[1]) > 0 and float(var[1]) > 0
    assert float(mean[2]) < 0 and float(rel[2]) < 0 and math.isfinite(float(rel[2]))
    raw3 = (4 * float(Q[3]) - (2 * 2.0) ** 2 / K) / (K - 1)
    assert raw3 < 0                                                  # the raw-moment result is negative ...
    assert float(var[3]) == 0.0 and float(rel[3]) == 0.0             # ... and is clamped: a zero, not a NaN the NaN -> 0 rule hides
    assert math.isinf(float(scalar))                                 # inf is not filtered out of the logged mean either
    # the reference's rule applied to the same mean / var: identical where var >= 0
    want = torch.sqrt(var) / mean
    want[want != want] = 0
    assert torch.equal(rel, want)


def _solver(loss="log-variance", adaptive=True, detach=False, d=3, time_approx="outer", H=8, **kw):
    pb = psp.LLGC(d=d, off_diag=0.1, T=0.2, seed=42, device="cpu")
    m = psp.Solver("gv", pb, L=1, K=16, delta_t=0.05, lr=0.01, loss_method=loss, time_approx=time_approx,
                   adaptive_forward_process=adaptive, detach_forward=detach, compute_gradient_variance=1, u_l2_error_flag=False,
                   verbose=False, device="cpu", **kw)
    if time_approx == "outer":
        m.z_n = [psp.DenseNet(d_in=d, d_out=d, lr=0.01, arch=[H, H], seed=42) for _ in range(m.N)]
    else:
        m.z_n = psp.DenseNet(d_in=d + 1, d_out=d, lr=0.01, arch=[H, H], seed=42)
    m.update_Phis()
    m.device = torch.device("cuda")              # only its type is read by the eligibility functions; nothing runs on it
    return m


@pytest.mark.parametrize("loss", ["moment", "log-variance"])
@pytest.mark.parametrize("adaptive,detach", [(False, True), (False, False), (True, False)])
def test_in_scope_configurations_are_native(loss, adaptive, detach, monkeypatch):
    monkeypatch.delenv("PSP_DENSE_BWD", raising=False)
    assert pdn.dense_eligibility(_solver(loss, adaptive, detach)) is None
    assert pdn.dense_eligibility(_solver(loss, adaptive, detach, learn_Y_0=True, random_X_0=True)) is None


def test_out_of_scope_configurations_name_their_reason(monkeypatch):
    monkeypatch.delenv("PSP_DENSE_BWD", raising=False)
    r = pdn.dense_eligibility(_solver(time_approx="inner"))
    assert r is not None and "time_approx='outer'" in r
    r = pdn.dense_eligibility(_solver(loss="variance"))
    assert r is not None and "'moment'" in r and "'log-variance'" in r
    r = pdn.dense_eligibility(_solver(adaptive=True, detach=True))
    assert r is not None and "detach_forward=True" in r
    r = pdn.dense_eligibility(_solver(d=130))
    assert r is not None and "d <= 128" in r
    assert pdn.dense_eligibility(_solver(d=100)) is None
    monkeypatch.setenv("PSP_DENSE_BWD", "gemm")
    r = pdn.dense_eligibility(_solver())
    assert r is not None and "PSP_DENSE_BWD=gemm" in r
    monkeypatch.delenv("PSP_DENSE_BWD")
    r = pdn.gradient_variance_unsupported(_solver(), (16, 32), world=2)
    assert r is not None and "single-rank" in r
    # without the diagnostic none of this is consulted
    m = _solver(adaptive=True, detach=True)
    m.compute_gradient_variance = 0
    assert pdn.dense_eligibility(m) is None


def test_reasons_without_the_library():
    """The reason function itself needs no library: the same table on an explicit instance."""
    f = pdn.gradient_variance_unsupported
    assert f(_solver("moment", False, True), (16, 32), world=1) is None
    assert f(_solver("log-variance", True, False), (128, 64), world=1) is None
    assert "d <= 128" in f(_solver(), (256, 32), world=1)
    assert "detach_forward=True" in f(_solver(adaptive=True, detach=True), (16, 32), world=1)
    assert "'moment'" in f(_solver(loss="cross_entropy"), (16, 32), world=1)


def test_the_other_native_plans_keep_their_refusal():
    """The tanh-MLP plan and the linear-control plan still decline the keyword; the composite plan serves them."""
    pb = psp.LLGC(d=3, off_diag=0.1, T=0.2, seed=42, device="cpu")
    kw = dict(L=1, K=16, delta_t=0.05, compute_gradient_variance=1, u_l2_error_flag=False, verbose=False, device="cpu")
    m = psp.Solver("gv", pb, time_approx="inner", detach_forward=True, **kw)
    m.device = torch.device("cuda")
    assert psp.plan_native.native_eligibility(m) is not None
    a = psp.Solver("gv", pb, time_approx="outer", detach_forward=True, **kw)
    eye = torch.eye(3)
    a.z_n = [psp.Linear(d=3, B=eye, Q=eye, lr=a.lr, seed=42) for _ in range(a.N)]
    a.update_Phis()
    a.device = torch.device("cuda")
    assert psp.plan_affine_native.affine_eligibility(a) is not None
    a.compute_gradient_variance = 0
    assert psp.plan_affine_native.affine_eligibility(a) is None
