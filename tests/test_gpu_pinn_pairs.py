"""The pair kernels of the native PINN plan (csrc/pinn_kernels.h, psp_pinn_pairs_*) on the GPU: through the C ABI against the
float64 statement of the (K, K) residual (ref64_pinn_pairs.py), and at solver level -- GeneralSolver(pinn_time_h='native') --
against the reference's goldens of ExponentialOnSphereNonlinearParabolic.

One bound, the one of every PINN kernel test: e_native <= 8 e_torch32 + 1e-6 with e(v) = max|v - v64| / max|v64|, for A, rho, nu,
the scalar loss and every named block of the gradient.  The chain is the plan's: the reduce reads the kernels' own A, the
backward the kernels' own rho and nu; the fp32 statement runs the same chain in torch.  Solver level: 1e-4 relative per
iteration of the loss log, as test_gpu_pinn.py asks of every golden."""
import ctypes as C
import math

import pytest
import torch

import ref64_pinn_pairs as rp
from conftest import load_golden
from pinn_cases import COMPOSITE_ONLY, GPU_SHAPES, build, probe_values, ref_case, seed_like_reference_train
from pinn_kernel_cases import Native, assert_rows, check_padding, pinn_config, table
from util_cases import psp
import ref64_pinn as r64

pytestmark = pytest.mark.gpu
nat = psp.native
PAD = 5
READS_T = ("pinn_expsphere_par_d3", "pinn_expsphere_par_d3_neumann")


def dev():
    return torch.device("cuda:0")


class PairsNative:
    """One case through psp_pinn_pairs_query / _residual / _reduce / _backward.  Every output buffer is PAD entries longer than
    the call needs and filled with NaN before it."""

    def __init__(self, case, alpha0=rp.ALPHA0):
        self.lib, d, f32 = nat.load(), dev(), torch.float32
        self.case, self.K, self.alpha0 = case, case["K"], alpha0
        self.cfg, self.sz, work = pinn_config(case), nat.PinnSizes(), C.c_int64()
        nat.check(self.lib.psp_pinn_pairs_query(C.byref(self.cfg), C.byref(self.sz), C.byref(work)), "psp_pinn_pairs_query")
        self.params = torch.cat([p.reshape(-1) for p in case["params"]]).to(d, f32).contiguous()
        assert self.params.numel() == self.sz.n_params
        self.x, self.t = case["x"].to(d, f32).contiguous(), case["t"].to(d, f32).contiguous()
        self.scratch = torch.empty(self.sz.scratch_bytes // 4 + PAD, dtype=f32, device=d)
        self.partial = torch.empty(self.sz.grad_partial_bytes // 4, dtype=f32, device=d)
        self.A, self.rho, self.nu = (torch.empty(self.K + PAD, dtype=f32, device=d) for _ in range(3))
        self.loss = torch.empty(1 + PAD, dtype=f32, device=d)
        self.work = torch.empty(work.value // 8 + PAD, dtype=torch.float64, device=d)
        self.grad = torch.empty(self.sz.n_params + PAD, dtype=f32, device=d)

    def run(self):
        p, cfg, K = nat.ptr, C.byref(self.cfg), self.K
        for buf in (self.scratch, self.partial, self.A, self.rho, self.nu, self.loss, self.work, self.grad):
            buf.fill_(float("nan"))
        nat.check(self.lib.psp_pinn_pairs_residual(cfg, p(self.params), p(self.x), p(self.t), p(self.scratch), p(self.A), None),
                  "psp_pinn_pairs_residual")
        nat.check(self.lib.psp_pinn_pairs_reduce(cfg, p(self.x), p(self.t), p(self.scratch), p(self.A), self.alpha0, p(self.work),
                                                 p(self.loss), p(self.rho), p(self.nu), None), "psp_pinn_pairs_reduce")
        nat.check(self.lib.psp_pinn_pairs_backward(cfg, p(self.params), p(self.x), p(self.t), p(self.scratch), p(self.rho),
                                                   p(self.nu), p(self.partial), p(self.grad), None), "psp_pinn_pairs_backward")
        torch.cuda.synchronize()
        return dict(A=self.A[:K], rho=self.rho[:K], nu=self.nu[:K], loss=self.loss[:1], grad=self.grad[:self.sz.n_params])

    def check_padding(self):
        K = self.K
        for label, buf, used in (("A", self.A, K), ("rho", self.rho, K), ("nu", self.nu, K), ("loss", self.loss, 1),
                                 ("pair_work", self.work, K), ("scratch", self.scratch, self.sz.scratch_bytes // 4),
                                 ("grad", self.grad, self.sz.n_params)):
            check_padding(label, buf[used:])
            assert bool(torch.isfinite(buf[:used]).all()), label


@pytest.mark.parametrize("name", sorted(rp.CASES))
def test_pair_kernels_match_float64(name):
    """Every shape of ref64_pinn_pairs.CASES: K = 1; 63 / 64 / 65 around a wave over the times; 257 (five trips of a wave, 65
    workgroups of four samples); 521 with 16 inputs (the time column alone in the second direction block, the backward's grid
    stride, tau = 0.5, e != 0, the identity); tanh^2 in two layers; the golden's shape with al = 0.7, T = 0.5."""
    ref = rp.reference(name)
    run = PairsNative(ref["case"])
    rows = rp.evaluate(ref, run.run())
    print("%s\n%s" % (name, table(rows)))
    assert_rows(rows)
    run.check_padding()


@pytest.mark.parametrize("name", ["k257_sin", "k521_sq_tau"])
def test_pair_kernels_are_deterministic(name):
    run = PairsNative(rp.reference(name)["case"])
    first = {k: v.clone() for k, v in run.run().items()}
    second = run.run()
    for k, v in first.items():
        assert torch.equal(v, second[k]), k


def test_backward_without_vadd_is_psp_pinn_backward_bit_for_bit():
    case = r64.make_case(**GPU_SHAPES["d16_par_a24_40_8"])        # has_time = 1, h does not read t
    run = Native(case)
    R = run.residual()
    rbar = ((2.0 / case["K"]) * R).contiguous()
    want = run.backward(rbar).clone()
    run.partial.fill_(float("nan"))
    run.grad.fill_(float("nan"))
    p = nat.ptr
    nat.check(run.lib.psp_pinn_pairs_backward(C.byref(run.cfg), p(run.params), p(run.x), p(run.t), p(run.scratch), p(rbar), None,
                                              p(run.partial), p(run.grad), None), "psp_pinn_pairs_backward")
    torch.cuda.synchronize()
    assert torch.equal(run.grad, want)


def first_iteration(case, model):
    """(X, t) of the first train_PINN() iteration, drawn in the plan's order."""
    seed_like_reference_train(case, model)
    if model.bounded:
        model._sample_boundary()
    X = model.sample_domain()
    return X, torch.rand(model.K, 1).to(model.device) * model.problem.T


@pytest.mark.parametrize("name", READS_T)
def test_solver_with_native_time_h_matches_the_reference_golden(name):
    rec = load_golden(name)
    case, exp = rec["case"], rec["expected"]
    prob, model = build(case, device=dev(), pinn_time_h="native")
    seed_like_reference_train(case, model)
    model.train_PINN()
    assert model.plan_name == "native", model.plan_reason
    errs = [abs(a - b) / abs(b) for a, b in zip(model.loss_log, exp["loss_log"])]
    print("%s: loss rel err per iteration %s" % (name, ["%.1e" % e for e in errs]))
    assert len(model.loss_log) == len(exp["loss_log"]) and max(errs) <= 1e-4, (model.loss_log, exp["loss_log"])
    assert model.K == exp["K"] and model.K_log == []
    for key in ("V_L2_log", "loss_log_domain", "loss_log_boundary", "V_test_L2"):
        got = getattr(model, key)
        assert len(got) == len(exp[key])
        for a, b in zip(got, exp[key]):
            assert abs(a - b) <= 1e-4 * abs(b) + 1e-12, (key, got, exp[key])
    v, want = probe_values(case, exp, prob, model), torch.tensor(exp["probe_V"])
    assert float((v - want).abs().max()) <= 1e-4 * max(1e-2, float(want.abs().max()))


@pytest.mark.parametrize("name", READS_T)
def test_first_iteration_gradient_of_the_plan_matches_float64(name):
    case = load_golden(name)["case"]
    _, model = build(case, device=dev(), pinn_time_h="native")
    X, t = first_iteration(case, model)
    plan = model._choose_pinn_plan()
    assert model.plan_name == "native" and plan.pairs
    a0 = model.alpha[0]
    loss = plan.pairs_loss_and_grad(X, t, a0)
    torch.cuda.synchronize()
    rcase = ref_case(model, X, t)
    ref = dict(case=rcase, f64=rp.statement(rcase, a0), f32=rp.statement(rcase, a0, torch.float32))
    K = model.K
    rows = rp.evaluate(ref, dict(A=plan.R[:K], rho=plan.rbar[:K], nu=plan.nu[:K], loss=loss.reshape(1), grad=plan.grad))
    print("%s\n%s" % (name, table(rows)))
    assert_rows(rows)


@pytest.mark.parametrize("name", READS_T)
def test_default_keyword_still_plans_torch_on_the_gpu(name):
    _, model = build(load_golden(name)["case"], device=dev(), L=1)
    with pytest.warns(UserWarning, match="composite torch plan"):
        model.train_PINN()
    assert model.plan_name == "torch" and COMPOSITE_ONLY[name] in model.plan_reason and "pinn_time_h" in model.plan_reason


def test_device_test_log_runs_behind_the_pair_plan():
    """K_test_log with test_log='device' on the plan's stream; the first loss is drawn before any test point."""
    rec = load_golden(READS_T[0])
    _, model = build(rec["case"], device=dev(), pinn_time_h="native", K_test_log=16, test_log="device")
    seed_like_reference_train(rec["case"], model)
    model.train_PINN()
    assert model.plan_name == "native"
    assert abs(model.loss_log[0] - rec["expected"]["loss_log"][0]) <= 1e-4 * rec["expected"]["loss_log"][0]
    for log in (model.V_test_L2, model.V_test_abs, model.V_test_rel_abs):
        assert len(log) == 3 and all(math.isfinite(v) and v > 0.0 for v in log)
