"""GPU: the naive and reference-control importance-sampling estimators above d = 64 on psp_isw_rollout (csrc/hjbew_kernels.h,
do_importance_sampling_me(..., wide_states='native')) against the composite plan on the same device and noise, the
learned-control kernel and a closed form -- the tests of tests/test_gpu_is_estimators.py at d > 64, with their tolerances.

The problems of the comparison were chosen on the CPU beforehand: on one noise stream of K = 65 536 the composite plan in fp32
agrees with itself in float64 to 1.1e-6 in every one of the six numbers (LLGC d = 80 dense / diagonal and LQGC d = 72 at T = 0.2;
DoubleWell_multidim d = 66 with d_1 = 64, eta = 0.05, kappa = 0.5, where exp(-g) stays an fp32 number, started 0.00127 off the
cell edge X_0 = -1 of its u* tables as tests/test_ref64_is.py does).
"""
import math
import re

import pytest
import torch

from affine_cases import build_modules
from util_cases import make_pkg_problem, psp

pytestmark = pytest.mark.gpu
nat = psp.native
KEYS = ["mean_naive", "variance_naive", "rel_error_naive", "mean_IS", "variance_IS", "rel_error_IS"]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _problem(pspec):
    prob = make_pkg_problem(pspec, dev())
    if hasattr(prob, "u_true_tables"):
        prob.X_0 = prob.X_0 + 0.00127
    return prob


def _solver(prob, backend, **kw):
    return psp.Solver("w", prob, L=0, K=16, delta_t=0.01, time_approx="inner", verbose=False, device=dev(), backend=backend, **kw)


COMPARE = [
    ("llgc80_dense", dict(kind="LLGC", kwargs=dict(d=80, off_diag=0.05, T=0.2, seed=42))),
    ("llgc80_diag", dict(kind="LLGC", kwargs=dict(d=80, off_diag=0.0, T=0.2, seed=42))),
    ("lqgc72_dense", dict(kind="LQGC", kwargs=dict(d=72, off_diag=0.05, T=0.2, seed=42, delta_t=0.005))),
    ("dw66", dict(kind="DoubleWell_multidim", kwargs=dict(d=66, d_1=64, d_2=2, T=0.2, eta=0.05, kappa=0.5),
                  calls=[["compute_reference_solution", {}], ["compute_reference_solution_2", {}]])),
]


@pytest.mark.parametrize("label,pspec", COMPARE, ids=[c[0] for c in COMPARE])
def test_native_matches_composite_on_the_same_noise(label, pspec):
    res = {}
    for backend in ("native", "torch"):
        prob = _problem(pspec)
        assert prob.d > nat.IS_MAX_D
        model = _solver(prob, backend)
        torch.manual_seed(11)
        res[backend] = psp.do_importance_sampling_me(prob, model, 65536, control="true", simulate_naive=True, delta_t=0.01,
                                                     wide_states="native")
    print(label, res)
    for k, a, b in zip(KEYS, res["native"], res["torch"]):
        assert math.isfinite(a) and a != 0.0
        assert math.isclose(a, b, rel_tol=1e-5 if k.startswith("mean") else 1e-4), (label, k, a, b)


def test_torch_default_is_unchanged_above_the_narrow_range():
    """wide_states='torch' (the default) keeps the refusal of the narrow kernel; 'native' lifts it up to ISW_MAX_D, where the
    library's own reason is raised."""
    prob = psp.LLGC(d=70, off_diag=0.0, T=0.05, seed=42, device=dev())
    model = _solver(prob, "native")
    with pytest.raises(NotImplementedError) as e:
        psp.do_importance_sampling_me(prob, model, 256, control="true", simulate_naive=True)
    assert "native range d <= 64 of psp_is_rollout" in str(e.value)
    out = psp.do_importance_sampling_me(prob, model, 256, control="true", simulate_naive=True, wide_states="native")
    assert len(out) == 6 and all(math.isfinite(v) for v in out)
    prob = psp.LLGC(d=nat.ISW_MAX_D + 4, off_diag=0.0, T=0.02, seed=42, device=dev())
    model = _solver(prob, "native")
    with pytest.raises(NotImplementedError) as e:
        psp.do_importance_sampling_me(prob, model, 64, control="true", simulate_naive=True, wide_states="native")
    assert "outside the native range d <= 256" in str(e.value)
    model.backend = "auto"                                                # ... and 'auto' falls back to the composite plan
    out = psp.do_importance_sampling_me(prob, model, 64, control="true", simulate_naive=True, wide_states="native")
    assert len(out) == 6 and all(math.isfinite(v) for v in out)


@pytest.mark.parametrize("label", ["dw66", "llgc80_diag"])
def test_cross_statistics_counts_agree(label, capsys):
    pspec = dict(COMPARE)[label]
    counts = {}
    for backend in ("native", "torch"):
        prob = _problem(pspec)
        model = _solver(prob, backend)
        torch.manual_seed(7)
        psp.do_importance_sampling_me(prob, model, 4096, control="true", simulate_naive=True, verbose=True, delta_t=0.01,
                                      cross_statistics=torch.tensor([[0.0]]), wide_states="native")
        counts[backend] = [int(m) for m in re.findall(r"crossed: (\d+)/4096", capsys.readouterr().out)]
    assert len(counts["native"]) == 2 and counts["native"] == counts["torch"], counts
    assert 0 < counts["native"][1]


def test_wide_kernel_and_learned_control_kernel_draw_the_same_philox_noise():
    """Learned control set to zero (W3 = b3 = 0): the IS path of psp_hjb_rollout_eval IS the naive path of psp_isw_rollout."""
    prob = psp.LLGC(d=80, off_diag=0.1, T=0.1, seed=42, device=dev())
    model = psp.Solver("l", prob, lr=2e-3, L=2, K=256, delta_t=0.01, loss_method="log-variance", time_approx="inner",
                       adaptive_forward_process=True, detach_forward=True, u_l2_error_flag=False, verbose=False, seed=42,
                       device=dev(), backend="native", noise="philox")
    model.train()
    with torch.no_grad():
        model.z_n.linears[-1].weight.zero_()
        model.z_n.linears[-1].bias.zero_()
    calls = getattr(model, "_is_calls", 0)
    out = psp.do_importance_sampling_me(prob, model, 1 << 16, simulate_naive=True, wide_states="native")
    assert model._is_calls == calls + 1                                   # one Philox key for both paths
    assert math.isfinite(out[0]) and out[0] > 0.0
    assert abs(out[0] - out[3]) <= 1e-6 * abs(out[3]), out


def test_closed_form_of_the_euler_scheme():
    """LLGC(d = 80): IS under u* is exactly unbiased for E exp(-alpha.X_N) = exp(s^2 / 2) of the Euler chain (discrete Girsanov),
    s^2 = alpha' Sigma_N alpha, Sigma_N = sum_k Phi^k B B' Phi^k' dt, Phi = I + A dt.  T = 0.05: s^2 = 6.10, so the naive
    weights are lognormal with relative error sqrt(exp(s^2) - 1) = 21.1 and K = 2^20 of them resolve their mean (at T = 1 as in
    the d = 20 test s^2 would be 44).  Calibrated on the CPU composite plan (K = 2^16, torch.manual_seed(0)): RE_IS = 0.0311,
    RE_naive = 15.2; the bound asks for a factor 20 as the d = 20 test does."""
    d, N = 80, 5
    prob = psp.LLGC(d=d, off_diag=0.1, T=0.05, seed=42, device=dev())
    model = _solver(prob, "native", noise="philox")
    K = 1 << 20
    mn, vn, rn, mi, vi, ri = psp.do_importance_sampling_me(prob, model, K, control="true", simulate_naive=True, wide_states="native")
    A, B = prob.A.double().cpu(), prob.B.double().cpu()
    Phi = torch.eye(d, dtype=torch.float64) + 0.01 * A
    S = torch.zeros(d, d, dtype=torch.float64)
    P = torch.eye(d, dtype=torch.float64)
    for _ in range(N):
        S += P @ B @ B.t() @ P.t() * 0.01
        P = Phi @ P
    al = prob.alpha.double().cpu()[:, 0]
    want = math.exp(0.5 * float(al @ S @ al))
    print("closed form %.6f  IS %.6f (RE %.4f)  naive %.6f (RE %.3f)" % (want, mi, ri, mn, rn))
    assert abs(mi - want) <= 5 * math.sqrt(vi / K) + 1e-4 * want, (mi, want)
    assert abs(mn - want) <= 5 * math.sqrt(vn / K) + 1e-4 * want, (mn, want)
    assert ri * 20 <= rn, (ri, rn)


def test_constant_list_above_the_narrow_range(monkeypatch):
    """A Constant list at d = 70 (approx_method='control', time_approx='outer'): psp_isw_rollout with the rows -c_idx(n) as a
    PSP_ISC_TABLE control, against the composite sweep on the same host noise, with the tolerance of
    tests/test_gpu_affine_control.py::test_importance_sampling_evaluation_is_native.  The evaluation grid (0.004) differs from the
    list's grid (0.01), so the step map is exercised."""
    d = 70
    prob = psp.LLGC(d=d, off_diag=0.05, T=0.1, seed=42, device=dev())
    model = psp.Solver(name="const", problem=prob, loss_method="log-variance", time_approx="outer", L=0, lr=0.1, seed=42,
                       delta_t=0.01, K=64, adaptive_forward_process=True, detach_forward=True, u_l2_error_flag=False,
                       verbose=False, device=dev(), backend="native")
    model.z_n = build_modules(dict(kind="Constant", init=dict(scale=0.1, seed0=9)), d, model.N, 0.1, 42, dev())
    model.update_Phis()
    ut = psp.utilities
    assert ut._affine_is_reason(prob, model) is not None and ut._affine_is_reason(prob, model, True) is None
    with pytest.raises(NotImplementedError):                              # (the default keeps today's refusal)
        ut.do_importance_sampling_me(prob, model, 400, delta_t=0.004)
    calls = []
    real = ut._is_rollout
    monkeypatch.setattr(ut, "_is_rollout", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    torch.manual_seed(11)
    got = ut.do_importance_sampling_me(prob, model, 400, delta_t=0.004, wide_states="native")
    assert calls == [1]
    torch.manual_seed(11)
    want = ut._is_composite(prob, model, 400, 0.004)
    print(got, want)
    for a, b in zip(got, want):
        assert math.isfinite(a) and math.isclose(a, b, rel_tol=2e-4), (got, want)
    model.backend = "auto"                                                # 'auto' takes the native path too where the library accepts
    torch.manual_seed(11)
    assert ut.do_importance_sampling_me(prob, model, 400, delta_t=0.004, wide_states="native") == got
