"""GPU: the naive and reference-control importance-sampling estimators on psp_is_rollout (csrc/hjbe_kernels.h) against the
reference's goldens, the composite plan on the same device and noise, the learned-control kernel and closed forms."""
import math
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from util_cases import make_pkg_problem, make_pkg_solver, psp

pytestmark = pytest.mark.gpu
GOLDEN = ["is_naive_dw1d_true", "is_naive_dw4_true", "is_naive_llgc6_true", "is_naive_lqgc3_true", "is_naive_llgc20_approx"]
KEYS = ["mean_naive", "variance_naive", "rel_error_naive", "mean_IS", "variance_IS", "rel_error_IS"]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _call(model, K, control, delta_t, cross, seed, **kw):
    torch.manual_seed(seed)
    return psp.do_importance_sampling_me(model.problem, model, K, control=control, simulate_naive=True, delta_t=delta_t,
                                         cross_statistics=cross, **kw)


def _crossed(capsys):
    return [int(m) for m in re.findall(r"crossed: (\d+)/", capsys.readouterr().out)]


@pytest.mark.parametrize("name", GOLDEN)
def test_native_matches_reference_golden(name, capsys):
    rec = load_golden(name)
    case, exp = rec["case"], rec["expected"]
    model = make_pkg_solver(case, dev(), backend="native")
    model.train()
    # (learned control: crossing counts only on the composite plan)
    cross = torch.tensor(case["cross"]) if case["control"] == "true" else None
    out = _call(model, case["is_K"], case["control"], case["is_delta_t"], cross, case["is_seed"], verbose=True)
    for k, got in zip(KEYS, out):
        tol = 2e-4 if k.startswith("mean") else 2e-3
        assert math.isclose(got, exp[k], rel_tol=tol), (k, got, exp[k])
    if cross is not None:
        assert _crossed(capsys) == [exp["crossed_naive"], exp["crossed_IS"]]


COMPARE = [
    ("dw1d", dict(kind="DoubleWell", kwargs=dict(d=1, T=1, eta=3.0, kappa=5.0), calls=[["compute_reference_solution", {}]])),
    ("dw10", dict(kind="DoubleWell_multidim", kwargs=dict(d=10, d_1=4, d_2=6, T=0.5, eta=2.0, kappa=3.0),
                  calls=[["compute_reference_solution", {}], ["compute_reference_solution_2", {}]])),
    ("llgc20_dense", dict(kind="LLGC", kwargs=dict(d=20, off_diag=0.1, T=0.5, seed=42))),
    ("llgc64_dense", dict(kind="LLGC", kwargs=dict(d=64, off_diag=0.05, T=0.3, seed=42))),
    ("llgc64_diag", dict(kind="LLGC", kwargs=dict(d=64, off_diag=0.0, T=0.3, seed=42))),
    ("lqgc10_dense", dict(kind="LQGC", kwargs=dict(d=10, off_diag=0.1, T=0.5, seed=42, delta_t=0.005))),
    ("lqgc64_dense", dict(kind="LQGC", kwargs=dict(d=64, off_diag=0.05, T=0.2, seed=42, delta_t=0.005))),
]


@pytest.mark.parametrize("label,pspec", COMPARE, ids=[c[0] for c in COMPARE])
def test_native_matches_composite_on_the_same_noise(label, pspec):
    res = {}
    for backend in ("native", "torch"):
        prob = make_pkg_problem(pspec, dev())
        model = psp.Solver("c", prob, L=0, K=16, delta_t=0.01, time_approx="inner", verbose=False, device=dev(), backend=backend)
        res[backend] = _call(model, 65536, "true", 0.01, None, 11)
    for k, a, b in zip(KEYS, res["native"], res["torch"]):
        assert math.isclose(a, b, rel_tol=1e-5 if k.startswith("mean") else 1e-4), (label, k, a, b)


def _learned(noise, d=6):
    prob = psp.LLGC(d=d, off_diag=0.1, T=0.3, seed=42, device=dev())
    model = psp.Solver("l", prob, lr=2e-3, L=2, K=256, delta_t=0.01, loss_method="log-variance", time_approx="inner",
                       adaptive_forward_process=True, detach_forward=True, u_l2_error_flag=False, verbose=False, seed=42,
                       device=dev(), backend="native", noise=noise)
    model.train()
    return prob, model


def test_both_kernels_draw_the_same_philox_noise():
    """Learned control set to zero (W3 = b3 = 0): the IS path of psp_hjb_rollout_eval IS the naive path of psp_is_rollout."""
    prob, model = _learned("philox")
    with torch.no_grad():
        model.z_n.linears[-1].weight.zero_()
        model.z_n.linears[-1].bias.zero_()
    out = psp.do_importance_sampling_me(prob, model, 1 << 16, simulate_naive=True)
    assert abs(out[0] - out[3]) <= 1e-6 * abs(out[3]), out


@pytest.mark.parametrize("noise", ["reference", "philox"])
def test_learned_control_IS_result_unchanged(noise):
    prob, model = _learned(noise)
    calls = getattr(model, "_is_calls", 0)
    torch.manual_seed(5)
    a = psp.do_importance_sampling_me(prob, model, 4096)
    model._is_calls = calls
    torch.manual_seed(5)
    b = psp.do_importance_sampling_me(prob, model, 4096, simulate_naive=True)
    assert model._is_calls == calls + 1
    assert tuple(b[3:]) == tuple(a)


def test_closed_form_of_the_euler_scheme():
    """LLGC(d = 20): IS under u* is exactly unbiased for E exp(-alpha.X_N) = exp(alpha' Sigma_N alpha / 2) of the Euler chain
    (discrete Girsanov), Sigma_N = sum_k Phi^k B B' Phi^k' dt, Phi = I + A dt."""
    prob = psp.LLGC(d=20, off_diag=0.1, T=1.0, seed=42, device=dev())
    model = psp.Solver("cf", prob, L=0, K=16, delta_t=0.01, time_approx="inner", verbose=False, device=dev(), backend="native",
                       noise="philox")
    K = 1 << 20
    mn, vn, rn, mi, vi, ri = psp.do_importance_sampling_me(prob, model, K, control="true", simulate_naive=True)
    A, B = prob.A.double().cpu(), prob.B.double().cpu()
    Phi = torch.eye(20, dtype=torch.float64) + 0.01 * A
    S = torch.zeros(20, 20, dtype=torch.float64)
    P = torch.eye(20, dtype=torch.float64)
    for _ in range(100):
        S += P @ B @ B.t() @ P.t() * 0.01
        P = Phi @ P
    al = prob.alpha.double().cpu()[:, 0]
    want = math.exp(0.5 * float(al @ S @ al))
    assert abs(mi - want) <= 5 * math.sqrt(vi / K) + 1e-4 * want, (mi, want)
    assert abs(mn - want) <= 5 * math.sqrt(vn / K) + 1e-4 * want, (mn, want)
    # calibrated on the CPU composite plan (K = 2^16, torch.manual_seed(0)): RE_IS = 0.0273, RE_naive = 97.0 (heavy-tailed naive
    # weights); the bound asks for a factor 20
    assert ri * 20 <= rn, (ri, rn)


def test_notebook_at_full_size(capsys):
    """The paper notebook's call at K = 1e7 on device noise, against its recorded output (5 combined standard errors)."""
    rec = load_golden("dw1d_notebook_is_record")
    prob = make_pkg_problem(rec["problem"], dev())
    model = psp.Solver("nb", prob, L=0, K=16, delta_t=0.01, time_approx="inner", verbose=False, device=dev(), backend="native",
                       noise="philox")
    K = rec["K"]
    mn, vn, rn, mi, vi, ri = psp.do_importance_sampling_me(prob, model, K, control="true", simulate_naive=True, verbose=True,
                                                           delta_t=rec["delta_t"], cross_statistics=torch.tensor([[0]]))
    cn, ci = _crossed(capsys)
    se_i = math.sqrt((rec["variance_IS"] + vi) / K)
    se_n = math.sqrt((rec["variance_naive"] + vn) / K)
    assert abs(mi - rec["mean_IS"]) <= 5 * se_i, (mi, rec["mean_IS"])
    assert abs(mn - rec["mean_naive"]) <= 5 * se_n, (mn, rec["mean_naive"])
    pn, pi = rec["crossed_naive"] / K, rec["crossed_IS"] / K
    assert abs(cn - rec["crossed_naive"]) <= 5 * math.sqrt(2 * K * pn * (1 - pn)), cn
    assert abs(ci - rec["crossed_IS"]) <= 5 * math.sqrt(2 * K * pi * (1 - pi)), ci
    # RE_IS within 10 % of the recorded 1.9394; calibrated on the CPU composite plan at K = 1e6 (seeds 0 / 1: 2.0316 / 2.0315,
    # +4.8 %) and measured natively at K = 1e7 (1.9136, -1.3 %)
    assert abs(ri - rec["rel_error_IS"]) <= 0.1 * rec["rel_error_IS"], ri


def test_outside_the_native_range_falls_back():
    prob = psp.LLGC(d=70, off_diag=0.0, T=0.05, seed=42, device=dev())
    model = psp.Solver("fb", prob, L=0, K=16, delta_t=0.01, time_approx="inner", verbose=False, device=dev())
    out = psp.do_importance_sampling_me(prob, model, 256, control="true", simulate_naive=True)
    assert len(out) == 6 and all(np.isfinite(out))
    model.backend = "native"
    with pytest.raises(NotImplementedError) as e:
        psp.do_importance_sampling_me(prob, model, 256, control="true", simulate_naive=True)
    assert "native range" in str(e.value)
