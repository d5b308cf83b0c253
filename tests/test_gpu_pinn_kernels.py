"""The PINN kernels (csrc/pinn_kernels.h) on the GPU past one tile per workgroup, through the C ABI: every case of
pinn_kernel_cases.py against its float64 statement, per named parameter block, per column of grad V and per vector of samples,
with fp32 torch autograd on the CPU as the yardstick (e_native <= 8 e_torch32 + 1e-6, the bound of test_gpu_pinn.py).  The
intermediates V, grad V and the Laplacian parts are read from the scratch by its documented layout (include/psp.h)."""
import pytest
import torch

import pinn_kernel_cases as kc
import ref64_pinn as r64
from conftest import load_golden
from pinn_cases import build, ref_case, seed_like_reference_train

pytestmark = pytest.mark.gpu
NAN = float("nan")


def show(name, rows):
    print("%s:\n%s" % (name, kc.table([r for r in rows if r[0].startswith("grad[")])))
    for kind, (e, e32, label) in kc.summary(rows).items():
        print("  %s worst of %-22s e_native %.2e  e_torch32 %.2e  (%s)" % (name, kind, e, e32, label))


def all_numbers(run, weights, twice=()):
    """One residual call and one backward call per entry of ``weights`` on ``run``, with the finite and padding checks after
    each; a key in ``twice`` is run again and must give the same bits."""
    R = run.residual()
    n_scratch, n_partial = run.used()
    kc.check_finite(R, R, R)
    kc.check_padding("R", run.R_buf[run.K:])
    kc.check_padding("scratch", run.scratch[n_scratch:])
    assert bool(torch.isfinite(run.scratch[:n_scratch]).all())
    got = {k: v.clone() for k, v in run.scratch_parts().items()}
    got["R"], got["grads"] = R.clone(), {}
    before = run.scratch.clone()
    for key, rbar in weights.items():
        g = run.backward(rbar).clone()
        kc.check_finite(R, g, run.partial[:n_partial])
        kc.check_padding("grad_partial", run.partial[n_partial:])
        if key in twice:
            assert torch.equal(run.backward(rbar), g), "two backward calls differ"
        got["grads"][key] = g
    assert torch.equal(run.scratch.nan_to_num(1e30), before.nan_to_num(1e30)) and torch.equal(run.R, got["R"])
    return got


@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_case_matches_float64_per_block(name):
    ref = kc.reference(name)
    case = ref["case"]
    if case["act"] == "relu2":                                   # phi'' jumps at 0: no comparison across a sign flip
        assert r64.preact_margin(case) >= 1e-5
    run = kc.Native(case, capacity=case["K"] + 3)                # three samples of room: what lies behind K stays untouched
    assert (run.sz.dir_blocks, run.sz.tiles, run.sz.bwd_workgroups) == kc.CASES[name][2]
    got = all_numbers(run, ref["rbar"], twice=("loss", "random") if name in kc.DETERMINISM else ())
    rows = kc.evaluate(ref, got)
    show(name, rows)
    kc.assert_rows(rows)


def test_capacity_beyond_the_batch_changes_no_bit():
    """stride_bwd's first 97 samples (291 tiles on 256 workgroups) in buffers sized for all 173, against buffers sized for 97."""
    ref = kc.reference("stride_bwd")
    case, K = ref["case"], 97
    w = {"random": kc.random_rbar(K), "loss": ref["rbar"]["loss"][:K]}
    roomy = all_numbers(kc.Native(case, capacity=case["K"], K=K), w)
    tight = all_numbers(kc.Native(case, K=K), w)
    for key in ("R", "V", "gradV", "lap_parts", "cV", "cG"):
        assert torch.equal(roomy[key], tight[key]), key
    for key in w:
        assert torch.equal(roomy["grads"][key], tight["grads"][key]), key
    assert kc.err(roomy["R"], ref["f64"]["R"][:K]) <= kc.bound(kc.err(ref["f32"]["R"][:K], ref["f64"]["R"][:K]))


def plan_numbers(plan, X, t, weights):
    for buf in (plan.scratch, plan.grad_partial, plan.R, plan.grad):
        buf.fill_(NAN)
    K = X.shape[0]
    R = plan.residual(X, t).clone()
    torch.cuda.synchronize()
    sz = plan.sizes
    got = {k: v.clone() for k, v in kc.scratch_parts(plan.scratch, K, sz.dir_blocks, X.shape[1] + (0 if t is None else 1)).items()}
    got["R"], got["grads"] = R, {}
    for key, w in weights.items():
        g = plan.backward(w.to(R.device, torch.float32)).clone()
        torch.cuda.synchronize()
        kc.check_finite(R, g, plan.grad_partial[:min(K * sz.dir_blocks, kc.MAX_BWD_WG) * plan.P])
        got["grads"][key] = g
    return got


def test_plan_residual_and_backward_per_block_and_below_capacity():
    """PinnNativePlan on the heat golden's net with K = 300: one block of 7 columns, 300 tiles on 256 workgroups."""
    case = load_golden("pinn_heat_d6")["case"]
    dev = torch.device("cuda:0")
    from path_space_pde_solver_amd.plan_pinn_native import PinnNativePlan

    def plan_of(K):
        prob, model = build(case, device=dev, L=1, boundary_loss=False, log_loss_parts=True, K_test_log=None, K=K)
        seed_like_reference_train(case, model)
        return prob, model, PinnNativePlan(model)

    prob, model, plan = plan_of(300)
    assert (plan.sizes.dir_blocks, plan.sizes.tiles, plan.sizes.bwd_workgroups) == (1, 300, 256)
    if model.bounded:
        model._sample_boundary()
    X = model.sample_domain()
    t = (torch.rand(model.K, 1) * prob.T).to(dev)
    rc = ref_case(model, X, t)
    ref = kc.build_reference(rc, alpha0=model.alpha[0])
    got = plan_numbers(plan, X, t, ref["rbar"])
    rows = kc.evaluate(ref, got)
    show("plan heat_d6 K=300", rows)
    kc.assert_rows(rows)
    # the first 200 points on the same plan, against a plan built for 200
    w200 = {"random": kc.random_rbar(200)}
    below = plan_numbers(plan, X[:200], t[:200], w200)
    kc.check_padding("scratch", plan.scratch[200 * (2 + 1 + 2 * 7):])
    _, _, fresh_plan = plan_of(200)
    assert torch.equal(fresh_plan.flat, plan.flat)
    fresh = plan_numbers(fresh_plan, X[:200], t[:200], w200)
    for key in ("R", "V", "gradV", "lap_parts"):
        assert torch.equal(below[key], fresh[key]), key
    assert torch.equal(below["grads"]["random"], fresh["grads"]["random"])
