"""EigenvalueSolver on the GPU: the native plan against the reference's notebooks (tests/golden/eig_*.json) with the bounds
tests/test_gpu_elliptic_catalogue.py applies to the same quantities -- K_log exact after asserting the recorded margins, loss 5e-5
relative on the first iteration and 1e-4 after, V_L2_log 1e-4, the first-iteration gradient within 5e-4 of max |g| of the float64
statement --, lambda_log as a coarse check (after three Adam steps it mostly shows the gradient's sign: a quarter of a step),
and a short noise='philox' run of the Schroedinger problem."""
import math

import pytest
import torch

import eigen_kernel_cases as ec
import ref64_eigenvalue as r64
from eigen_cases import GOLDENS, LOSS_LOGS, build, kind_of
from util_cases import psp

pytestmark = pytest.mark.gpu
MIN_MARGIN = 1e-5


def dev():
    return torch.device("cuda:0")


def float64_first_iteration(name, rec):
    """The float64 statement of the golden's first iteration, on the draws its seed gives."""
    case, exp = rec["case"], rec["expected"]
    kind = kind_of(name)
    net = exp["net"]
    c = ec._c(name, "fp" if kind == "fp" else "nls", case["d"], case["K"], (net["act"], net["dims"][1:-1], net["linear"]),
              exp["settings"]["delta_t"] if case["delta_t"] is None else case["delta_t"], "init", lam=exp["lambda_init"],
              seed=case["seed"])
    assert case["N"] == ec.N and case["K_boundary"] == ec.KB and exp["settings"]["alpha"] == ec.ALPHA
    return ec.runs(c)["full"]


@pytest.mark.parametrize("name", GOLDENS)
def test_native_matches_notebook(name):
    rec, prob, model = build(name, device=dev(), backend="native")
    exp = rec["expected"]
    assert exp["min_exit_margin"] >= MIN_MARGIN and exp["min_gate_margin"] >= MIN_MARGIN
    plan = model._choose_plan()
    assert model.plan_name == "native", model.plan_reason
    assert type(plan).__name__ == "EigenDeepPlan"
    assert plan.cfg.h_kind == (psp.native.GH_EIG_FP if kind_of(name) == "fp" else psp.native.GH_EIG_NLS)
    plan.path.fill_(float("nan"))
    seen = []
    step = plan.iteration

    def iteration(l):
        out = step(l)
        seen.append(plan.grad.detach().cpu().clone())
        return out
    plan.iteration = iteration
    model.train()
    assert model._gen_plan is plan
    print("%s: K_log %s" % (name, model.K_log))
    assert model.K_log == exp["K_log"]
    for log in LOSS_LOGS:
        got, want = getattr(model, log), exp[log]
        errs = [abs(a - b) / max(abs(b), 1e-12) for a, b in zip(got, want)]
        print("  %s rel err per iteration %s" % (log, ["%.1e" % e for e in errs]))
        assert len(got) == len(want)
        for l, (a, b) in enumerate(zip(got, want)):
            # the domain part is mean(D^2) with D = V(X_N) - V(X_0) - Y a difference of O(1) numbers summed over N fp32 steps: D is
            # known to ~1e-6 absolute (8 ulp of 1), so mean(D^2) to 2 sqrt(mean(D^2)) 1e-6 -- the fp32 reference itself is 2.4e-5
            # relative off float64 there (eig_fp_d5); the other parts get the relative bounds alone
            abs_tol = 2e-6 * math.sqrt(b) if log == "loss_log_domain" else 1e-12
            assert math.isclose(a, b, rel_tol=5e-5 if l == 0 else 1e-4, abs_tol=abs_tol), (log, l, got, want)
    for a, b in zip(model.V_L2_log, exp["V_L2_log"]):
        assert math.isclose(a, b, rel_tol=1e-4, abs_tol=1e-9), (model.V_L2_log, exp["V_L2_log"])
    lr = exp["settings"]["lambda_lr"]
    print("  lambda_log %s reference %s" % (model.lambda_log, exp["lambda_log"]))
    for a, b in zip(model.lambda_log, exp["lambda_log"]):
        assert abs(a - b) <= 0.25 * lr, (model.lambda_log, exp["lambda_log"])
    assert model.lambda_.Y_0.item() == pytest.approx(model.lambda_log[-1])
    full = float64_first_iteration(name, rec)
    g64 = full["grad"]
    eg = float((seen[0].double() - g64).abs().max()) / max(float(g64.abs().max()), 1e-300)
    print("  first-iteration gradient err %.1e of max|g| = %.3e" % (eg, float(g64.abs().max())))
    assert abs(model.loss_log[0] - full["loss"]) <= 5e-5 * abs(full["loss"])
    assert eg <= 5e-4 or float(g64.abs().max()) == 0.0


def test_philox_schroedinger_run_moves_lambda_and_lowers_the_error():
    """300 iterations at d = 5, K = 512 with on-device noise: lambda leaves -2 toward -3 and V_L2_log falls.  Direction and the
    monotone trend of a moving average only; no rate is promised.
    lambda moves by at most lambda_lr = 1e-3 per iteration, so 300 iterations cover at most 0.3 of the way; its 50-iteration means
    must fall one after the other.  V_L2_log is a Monte-Carlo figure over K = 512 trajectories; its average is taken over the two
    halves of the run (150 iterations each).  Measured on an MI355X: lambda -2.001 -> -2.283, 50-iteration means -2.024, -2.071,
    -2.120, -2.168, -2.215, -2.261; V_L2 50-iteration means 7.43e-3, 5.95e-3, 5.62e-3, 5.64e-3, 5.70e-3, 5.68e-3 -- the error
    falls over the first hundred iterations and then stays within its sampling noise while lambda is still far from -3, which is
    why no finer monotone claim is made for it."""
    d = 5
    prob = psp.SchroedingerEigenvalue(d=d, device=dev())
    model = psp.EigenvalueSolver(prob, "nls_philox", L=300, K=512, lambda_init=-2.0, lambda_lr=0.001, normalisation="l2",
                                 verbose=False, device=dev(), backend="native", noise="philox")
    model.V = psp.DenseNet_tanh(d, 1, lr=0.001, arch=[15] * 4, output_relu=True).to(dev())
    model.train()
    assert model.plan_name == "native", model.plan_reason
    lam, err = torch.tensor(model.lambda_log), torch.tensor(model.V_L2_log)
    assert len(lam) == 300 and bool(torch.isfinite(lam).all()) and bool(torch.isfinite(err).all())
    la, ea = lam.reshape(6, 50).mean(1), err.reshape(6, 50).mean(1)
    print("lambda: first %.5f last %.5f, 50-iteration means %s" % (lam[0], lam[-1], ["%.5f" % v for v in la]))
    print("V_L2: first %.4e last %.4e, 50-iteration means %s" % (err[0], err[-1], ["%.4e" % v for v in ea]))
    assert lam[-1] < -2.0 and lam[-1] > -3.0 and bool((la[1:] < la[:-1]).all())
    halves = err.reshape(2, 150).mean(1)
    assert halves[1] < halves[0], halves
