"""Host side of the sigma-basis rollout (plan_native.py: state_basis_decision, sigma_basis_problem).

With a constant invertible sigma = B the state may be carried as X~ = B^-1 X:
    X~_{n+1} = X~_n + dt (B^-1 A B) X~_n + v_n,   W1x X = (W1x B) X~,   g = (B^T alpha) . X~_N,   dW1x = dW~1x B^T.
No GPU here: the eligibility rule, the fp64 identities of the transformed problem, and the CPU oracle run on the transformed
problem against the original one with the same supplied noise.
"""
import copy

import numpy as np
import pytest
import torch

from util_cases import orc, psp

from path_space_pde_solver_amd import plan_native  # noqa: E402
CPU = torch.device("cpu")


def solver(problem, **over):
    kw = dict(lr=1e-3, L=1, K=64, delta_t=0.01, loss_method="log-variance", time_approx="inner", adaptive_forward_process=True,
              detach_forward=True, u_l2_error_flag=False, verbose=False, seed=42, device=CPU, backend="torch", widths=(64, 64))
    kw.update(over)
    return psp.Solver("basis-host", problem, **kw)


# ---- eligibility ------------------------------------------------------------------------------------------------------------
def test_headline_problem_rolls_out_in_the_sigma_basis(monkeypatch):
    monkeypatch.delenv("PSP_STATE_BASIS", raising=False)
    s = solver(psp.LLGC(d=100, off_diag=0.01, T=0.1, seed=42, device=CPU))
    basis, why = plan_native.state_basis_decision(s)
    assert basis == "sigma", why
    monkeypatch.setenv("PSP_STATE_BASIS", "0")
    assert plan_native.state_basis_decision(s) == ("x", "PSP_STATE_BASIS=0")


def test_ill_conditioned_sigma_stays_in_the_x_basis(monkeypatch):
    monkeypatch.delenv("PSP_STATE_BASIS", raising=False)
    pb = psp.LLGC(d=20, off_diag=0.3, T=0.1, seed=42, device=CPU)
    cond = np.linalg.cond(pb.B.double().numpy(), 2)
    assert 30.0 < cond < 60.0, cond                                  # the cond_2 ~ 41 matrix of DESIGN's table
    basis, why = plan_native.state_basis_decision(solver(pb, widths=(30, 30)))
    assert basis == "x" and "cond_2" in why and "exceeds" in why, why


@pytest.mark.parametrize("what", ["lqgc", "random_X_0", "attached", "u_l2_from_path", "wide"])
def test_ineligible_configurations_stay_in_the_x_basis_and_sigma_raises(what, monkeypatch):
    monkeypatch.delenv("PSP_STATE_BASIS", raising=False)
    llgc = psp.LLGC(d=12, off_diag=0.1, T=0.1, seed=42, device=CPU)
    if what == "lqgc":
        pb, kw, word = psp.LQGC(d=12, off_diag=0.1, T=0.1, delta_t=0.01, seed=42, device=CPU), {}, "cost"
    elif what == "random_X_0":
        pb, kw, word = llgc, dict(random_X_0=True), "random_X_0"
    elif what == "attached":
        pb, kw, word = llgc, dict(detach_forward=False), "attached"
    elif what == "u_l2_from_path":
        class XDependentReference(psp.LLGC):             # an LLGC whose reference control is NOT declared x-independent
            u_true_x_independent = False
        pb, kw, word = XDependentReference(d=12, off_diag=0.1, T=0.1, seed=42, device=CPU), dict(u_l2_error_flag=True), "u_L2"
    else:
        pb, kw, word = psp.LLGC(d=128, off_diag=0.01, T=0.1, seed=42, device=CPU), {}, "wide"
    basis, why = plan_native.state_basis_decision(solver(pb, widths=(30, 30), **kw))
    assert basis == "x" and word in why, why
    with pytest.raises(ValueError) as e:                 # (not PlanUnsupported: backend='auto' would swallow that)
        plan_native.state_basis_decision(solver(pb, widths=(30, 30), state_basis="sigma", **kw))
    assert not isinstance(e.value, plan_native.PlanUnsupported) and word in str(e.value)
    assert plan_native.state_basis_decision(solver(pb, widths=(30, 30), state_basis="x", **kw))[0] == "x"


def test_auto_declines_a_start_vector_with_one_huge_component(monkeypatch):
    """an fp32 B^-1 X resolves every component of X to eps ||B|| max |X~|: 'auto' keeps such a plan in the x basis, 'sigma' insists"""
    monkeypatch.delenv("PSP_STATE_BASIS", raising=False)
    s = solver(psp.LLGC(d=12, off_diag=0.1, T=0.1, seed=42, device=CPU), widths=(30, 30))
    x0 = 0.5 * torch.cos(torch.arange(12, dtype=torch.float32))
    s.X_0 = x0.clone()
    assert plan_native.state_basis_decision(s)[0] == "sigma"
    x0[3] = 7.0e4
    s.X_0 = x0
    basis, why = plan_native.state_basis_decision(s)
    assert basis == "x" and "X_0" in why, why
    s.state_basis = "sigma"
    assert plan_native.state_basis_decision(s)[0] == "sigma"


def test_a_decided_basis_does_not_look_at_the_matrix(monkeypatch):
    monkeypatch.setattr(plan_native.np.linalg, "svd", lambda *a, **k: (_ for _ in ()).throw(AssertionError("svd called")))
    pb = psp.LLGC(d=12, off_diag=0.1, T=0.1, seed=42, device=CPU)
    assert plan_native.state_basis_decision(solver(pb, widths=(30, 30), state_basis="x"))[0] == "x"
    monkeypatch.setenv("PSP_STATE_BASIS", "0")
    assert plan_native.state_basis_decision(solver(pb, widths=(30, 30)))[0] == "x"


def test_state_basis_keyword_is_validated():
    with pytest.raises(ValueError):
        solver(psp.LLGC(d=12, off_diag=0.1, T=0.1, seed=42, device=CPU), state_basis="B")


# ---- identities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,off", [(100, 0.01), (12, 0.1), (100, 0.03)])
def test_transformed_problem_identities_in_fp64(d, off):
    pb = psp.LLGC(d=d, off_diag=off, T=0.1, seed=42, device=CPU)
    A, B = pb.A.double().numpy(), pb.B.double().numpy()
    alpha = pb.alpha[:, 0].double().numpy()
    x0 = np.linspace(-1.0, 1.0, d)
    M, al, x0t = plan_native.sigma_basis_problem(A, B, alpha, x0)
    assert M.dtype == np.float64 and al.dtype == np.float64 and x0t.dtype == np.float64
    assert np.abs(B @ M - A @ B).max() <= 1e-12                      # B M = A B
    assert np.abs(al - B.T @ alpha).max() <= 1e-12                   # alpha' = B^T alpha  (g = alpha . X = alpha' . X~)
    assert np.abs(B @ x0t - x0).max() <= 1e-12                       # B x~0 = x0


# ---- the oracle on the transformed problem ----------------------------------------------------------------------------------
D_, K_, N_, DT_ = 12, 64, 10, 0.01


def _oracle_problem(A, B, alpha, x0, dtype):
    A, B, alpha, x0 = (torch.as_tensor(t, dtype=dtype) for t in (A, B, alpha.reshape(-1, 1), x0))
    return orc.OracleProblem(kind="LLGC", d=D_, T=N_ * DT_, X_0=x0, B=B, b=lambda x: torch.mm(A, x.t()).t(), sigma=lambda x: B,
                             h=lambda t, x, y, z: -0.5 * torch.sum(z ** 2, dim=1), f=lambda x, t: torch.zeros(x.shape[0], dtype=dtype),
                             g=lambda x: torch.mm(x, alpha)[:, 0], extra=dict(A=A, alpha=alpha))


def _two_iterations(dtype, basis, scale=1.0):
    """Two training iterations of the oracle (Adam in the ORIGINAL basis both times): per iteration the loss and the flat
    gradient in the original basis.  basis='sigma' evaluates each iteration on the transformed problem -- A' = M, B' = I, alpha',
    x~0, W1x' = W1x B -- and takes dW1x = dW~1x B^T."""
    # (problem and net are drawn in fp32 whatever `dtype`: the fp64 run starts from the same matrices and weights)
    pb = psp.LLGC(d=D_, off_diag=0.1, T=N_ * DT_, seed=42, device=CPU)
    z32 = orc.TanhMLP(D_ + 1, D_, 1e-3, seed=123, widths=(64, 64))
    keep = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        A, B, alpha = pb.A.double().numpy(), pb.B.double().numpy(), pb.alpha[:, 0].double().numpy()
        x0 = 0.5 * np.cos(np.arange(D_))
        M, al, x0t = plan_native.sigma_basis_problem(A, B, alpha, x0)
        Bt = torch.as_tensor(B, dtype=dtype)
        orig = _oracle_problem(A, B, alpha, x0, dtype)
        tran = _oracle_problem(M, np.eye(D_), al, x0t, dtype)
        cfg = orc.HJBConfig(K=K_, delta_t=DT_, lr=1e-3, L=1, seed=42, adaptive_forward_process=True, detach_forward=True)
        z = z32.to(dtype)
        with torch.no_grad():
            for p in z.parameters():
                p.mul_(scale)
        z.optim = torch.optim.Adam(z.parameters(), lr=1e-3)
        _, y0, N = orc.hjb_build(orig, cfg)
        assert N == N_
        g = torch.Generator().manual_seed(7)
        noise = [torch.randn(K_, D_, N_ + 1, generator=g, dtype=torch.float64).to(dtype) for _ in range(2)]
        losses, grads = [], []
        for l in range(2):
            if basis == "sigma":
                zt = copy.deepcopy(z)
                zt.optim = torch.optim.Adam(zt.parameters(), lr=1e-3)
                with torch.no_grad():
                    zt.linears[0].weight[:, 1:] = z.linears[0].weight[:, 1:] @ Bt
                out = orc.hjb_train(tran, cfg, step_models=(zt, y0, N), noise=[noise[l]], trace=True)
                gr = [t.clone() for t in out["traces"][0]["grads"]]
                gr[0][:, 1:] = gr[0][:, 1:] @ Bt.t()
                # the same Adam step as the x-basis run takes: on the original parameters with the back-transformed gradient
                z.optim.zero_grad()
                for p, t in zip(z.parameters(), gr):
                    p.grad = t.clone()
                z.optim.step()
            else:
                out = orc.hjb_train(orig, cfg, step_models=(z, y0, N), noise=[noise[l]], trace=True)
                gr = out["traces"][0]["grads"]
            losses.append(out["loss_log"][0])
            grads.append(torch.cat([t.reshape(-1) for t in gr]).double())
        return losses, grads
    finally:
        torch.set_default_dtype(keep)


def _errors(a, b):
    """max over the two iterations of (relative loss difference, gradient difference / max |gradient|)"""
    el = max(abs(x - y) / abs(y) for x, y in zip(a[0], b[0]))
    eg = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(a[1], b[1]))
    return el, eg


# The bound is the oracle's own reformulation error: its fp32 run of the ORIGINAL problem against its fp64 run of the same problem
# (same matrices, weights, noise and two Adam steps).  Measured once (CPU, d = 12, K = 64, N = 10, cond_2(B) = 2.2, weights x 30 so
# that the control is O(1)): MEASURED_X_VS_FP64 below (the sigma-basis run measured 5.9e-7 / 3.7e-7 against fp64 and 2.6e-7 / 2.4e-7
# against the fp32 x-basis run at the same time); the sigma-basis run must stay within four times the reference's own error, of the
# x-basis run and of fp64.
MEASURED_X_VS_FP64 = (3.3e-7, 3.2e-7)      # (relative loss error, gradient error / max |gradient|), max over the two iterations
BOUND_LOSS, BOUND_GRAD = 4 * MEASURED_X_VS_FP64[0], 4 * MEASURED_X_VS_FP64[1]


def test_oracle_on_the_transformed_problem_matches_the_original():
    scale = 30.0
    x32, s32 = _two_iterations(torch.float32, "x", scale), _two_iterations(torch.float32, "sigma", scale)
    x64, s64 = _two_iterations(torch.float64, "x", scale), _two_iterations(torch.float64, "sigma", scale)
    exact = _errors(s64, x64)
    print("fp64 sigma vs x (the algebra):", exact)
    print("fp32 x vs fp64:", _errors(x32, x64), " fp32 sigma vs fp64:", _errors(s32, x64), " fp32 sigma vs fp32 x:", _errors(s32, x32))
    assert exact[0] <= 1e-12 and exact[1] <= 1e-12                   # the transformation is exact
    assert float(x64[1][0].abs().max()) > 0 and x64[0][0] != x64[0][1]
    el, eg = _errors(s32, x32)
    assert el <= BOUND_LOSS and eg <= BOUND_GRAD, (el, eg)
    el, eg = _errors(s32, x64)
    assert el <= BOUND_LOSS and eg <= BOUND_GRAD, (el, eg)
