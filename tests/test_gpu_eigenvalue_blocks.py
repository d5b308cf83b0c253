"""The eigenvalue kernels (psp_genl_rollout_fwd_eig: the EIG instances of genl_fwd_kernel, csrc/genl_kernels.h; psp_genl_rollout_bwd
unchanged) against the float64 restatement tests/ref64_eigenvalue.py on the same draws, in the style of
tests/test_gpu_general_block_gradients.py.  The first native iteration of EigenvalueSolver (backend='native', noise='reference', the
path store filled with NaN first) of every case of tests/eigen_kernel_cases.py:
  gradient       every block of the KERNELS' gradient (plan.grad as psp_genl_rollout_bwd leaves it, before the autograd terms are
                 added) and of the whole gradient, to BLOCK_TOL = 2e-4 of the block's own maximum (floored at 1e-4 of the whole);
  end points     Y_N, V(X_N), X_N per trajectory to D_TOL = 2e-5 max(1, max |.|);   S_k to 2e-5 of its maximum;
  loss           5e-5 relative, and its domain part alone;
  dLoss/dlambda  within 4 x DLAM_FP32_ERR of sum_k |w_k S_k| -- four times the fp32 composite plan's own error against float64,
                 measured on the CPU in tests/test_ref64_eigenvalue.py;
  discrete       K_log and the per-tile step counts exact (tests/test_ref64_eigenvalue.py asserts the margins on the CPU).
Measured on an MI355X over the thirteen cases (the one-, four- and eight-wave instances of the forward): whole-gradient blocks within
1.6e-5; blocks of the kernels' part within 4.6e-5 except the output bias of nls-d17-K40-relu15-drawn-dt05 at 1.6e-4 -- a cancelling
sum on which the fp32 composite plan's own domain-only gradient is 2.4e-4 off float64 on the CPU: the fp32 floor, close to the bound;
end points 1.1e-6, S_k 1.3e-6, loss 7.5e-7, its domain part 1.3e-5, dLoss/dlambda 9.0e-6.
Then: lambda is read from device memory by every launch; a NULL psp_genl_eig is psp_genl_rollout_fwd bit for bit on a scaled-sigma
and on a dense-sigma shape."""
import copy
import ctypes as C

import pytest
import torch

import eigen_kernel_cases as ec
from general_block_cases import assert_general_blocks
from test_ref64_eigenvalue import DLAM_FP32_ERR
from util_cases import psp

pytestmark = pytest.mark.gpu
nat = psp.native
BLOCK_TOL, D_TOL, LOSS_TOL, S_TOL = 2e-4, 2e-5, 5e-5, 2e-5


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def native_iteration(c, monkeypatch):
    run = ec.runs(c)
    if c["nw"] is None:
        monkeypatch.delenv("PSP_GENL_NW", raising=False)
    else:
        monkeypatch.setenv("PSP_GENL_NW", c["nw"])
    V = copy.deepcopy(run["V"]).to(dev())
    pb, model = ec.solver(c, V, device=dev(), backend="native")
    plan = model._choose_plan()
    assert model.plan_name == "native", model.plan_reason
    assert type(plan).__name__ == "EigenDeepPlan" and bool(plan.eig.output_relu) == c["relu"]
    assert int(plan.sizes.waves_per_tile) == c["waves"], (int(plan.sizes.waves_per_tile), c["waves"])
    plan.path.fill_(float("nan"))                                # a slot read without having been written fails here
    seen = {}
    launch = plan._launch_bwd

    def launch_bwd(flat, st):
        launch(flat, st)
        seen["kernel_grad"] = plan.grad.detach().clone()
    plan._launch_bwd = launch_bwd
    lam0 = float(model.lambda_.Y_0.item())
    model.train()
    torch.cuda.synchronize()
    return run, model, plan, seen["kernel_grad"].cpu(), lam0


@pytest.mark.parametrize("c", ec.CASES, ids=[c["id"] for c in ec.CASES])
def test_first_iteration_matches_the_float64_reference(c, monkeypatch):
    run, model, plan, gk, lam0 = native_iteration(c, monkeypatch)
    ref, full = run["ref"], run["full"]
    K = c["K"]
    assert lam0 == pytest.approx(c["lam"])
    assert model.K_log == [ref["K_count"]], (model.K_log, ref["K_count"])
    assert torch.equal(plan._tile_steps().cpu().long(), ref["tile_steps"]), (plan._tile_steps().cpu(), ref["tile_steps"])
    assert torch.equal(torch.round(plan.tN.double().cpu() / plan.cfg.dt).long(), ref["steps"])
    errs = {}
    for name, got in (("YN", plan.YN), ("VN", plan.VN), ("XN", plan.XN)):
        got, want = got.double().cpu(), ref[name]
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), name
        errs[name] = float((got - want).abs().max()) / max(1.0, float(want.abs().max()))
    S = plan._S[:K].double().cpu()
    errs["S"] = float((S - ref["S"]).abs().max()) / max(float(ref["S"].abs().max()), 1e-300)
    errs["loss"] = abs(model.loss_log[0] - full["loss"]) / abs(full["loss"])
    errs["domain"] = abs(model.loss_log_domain[0] - full["parts"]["domain"]) / abs(full["parts"]["domain"])
    dlam = float(plan.lam_grad.item())
    errs["dlam"] = abs(dlam - ref["dlam"]) / ref["dlam_scale"]
    print("%s [fwd<%d>]: %s" % (c["id"], int(plan.sizes.waves_per_tile), "  ".join("%s %.2e" % kv for kv in errs.items())))
    lay, kw = ec.layout(c)
    assert bool(torch.isfinite(gk).all())
    assert_general_blocks(gk, ref["grad_domain"], lay, BLOCK_TOL, tag=c["id"] + " kernels", **kw)
    assert_general_blocks(plan.grad.cpu(), full["grad"], lay, BLOCK_TOL, tag=c["id"] + " whole", **kw)
    assert all(errs[k] <= D_TOL for k in ("YN", "VN", "XN")), errs
    assert errs["S"] <= S_TOL, errs
    assert errs["loss"] <= LOSS_TOL and errs["domain"] <= LOSS_TOL, errs
    assert errs["dlam"] <= 4 * DLAM_FP32_ERR, (dlam, ref["dlam"], errs)
    for k in ("center", "boundary", "derivative_boundary"):
        got = getattr(model, "loss_log_" + k)[0] / (model.center_scale if k == "center" else 1.0)
        assert abs(got - full["parts"][k]) <= LOSS_TOL * max(abs(full["parts"][k]), 1e-6), (k, got, full["parts"][k])
    assert abs(model.V_L2_log[0] - full["V_L2"]) <= 1e-4 * abs(full["V_L2"]) + 1e-12


def _forward(plan, c, run):
    st = nat.stream_ptr(dev())
    x0 = run["draws"]["X0"].to(dev()).contiguous()
    xi = run["draws"]["xi"].to(dev()).contiguous()
    plan._set_batch(c["K"])
    plan.kcount.zero_()
    plan._launch_fwd(plan.flat, x0, torch.zeros(c["K"], device=dev()), xi, 0, st)
    torch.cuda.synchronize()
    return plan.YN.double().cpu().clone(), plan.VN.double().cpu().clone(), plan._S[:c["K"]].double().cpu().clone()


@pytest.mark.parametrize("c", [ec.CASES[1], ec.CASES[2]], ids=[ec.CASES[1]["id"], ec.CASES[2]["id"]])
def test_lambda_is_read_from_device_memory(c):
    """Two forwards whose lambda differs in device memory alone: Y_N moves by -dlambda S_k, V(X_N) and S_k do not move."""
    run = ec.runs(c)
    V = copy.deepcopy(run["V"]).to(dev())
    pb, model = ec.solver(c, V, device=dev(), backend="native")
    plan = model._choose_plan()
    assert model.plan_name == "native", model.plan_reason
    ptr = plan.lam.data_ptr()
    Y1, V1, S1 = _forward(plan, c, run)
    dl = 0.375
    plan.lam.add_(dl)                                            # in place: the same device word, no new plan, no new struct
    assert plan.lam.data_ptr() == ptr and plan.eig.lambda_ == ptr
    Y2, V2, S2 = _forward(plan, c, run)
    assert torch.equal(V1, V2) and torch.equal(S1, S2) and float(S1.abs().max()) > 0
    want = -dl * S1
    err = float((Y2 - Y1 - want).abs().max())
    # fp32 rounding of Y_N (|Y| = O(max |Y|)) over N steps
    bound = 20 * 2.0 ** -23 * max(1.0, float(Y1.abs().max()), float(Y2.abs().max()))
    print("%s: max |dY + dlambda S| = %.2e (bound %.2e), max |dlambda S| = %.2e" % (c["id"], err, bound, float(want.abs().max())))
    assert err <= bound and float(want.abs().max()) > 100 * bound


@pytest.mark.parametrize("name", ["expball_sin_d5_arch3_elliptic_diffusion", "cat_sinnorm2_lin_d4_diffusion"])
def test_null_struct_is_the_existing_entry_point(name):
    """psp_genl_rollout_fwd_eig(cfg, NULL, ..) against psp_genl_rollout_fwd(cfg, ..) on a sigma = s I shape and a dense-sigma
    shape: every output bit for bit."""
    from conftest import load_golden
    from test_general_composite_golden import build
    rec = load_golden(name)
    prob, model = build(rec["case"], device=dev(), backend="native")
    plan = model._choose_plan()
    assert type(plan).__name__ == "GeneralDeepPlan", (type(plan).__name__, model.plan_reason)
    assert (plan.gcfg.sigma_kind == nat.GENL_SIGMA_DENSE) == name.startswith("cat_sinnorm2")
    lib, st = nat.load(), nat.stream_ptr(dev())
    K, N, d = plan.K_local, model.N, prob.d
    g = torch.Generator().manual_seed(5)
    x0 = (0.4 * torch.randn(K, d, generator=g)).to(dev()).contiguous()
    xi = torch.randn(N, K, d, generator=g).to(dev()).contiguous()
    t0 = torch.zeros(K, device=dev())
    outs = []
    for which in ("plain", "null"):
        tables, path, ahat = torch.zeros_like(plan.tables), torch.full_like(plan.path, float("nan")), torch.zeros_like(plan.ahat)
        VN, YN, tN = (torch.zeros(K, device=dev()) for _ in range(3))
        XN = torch.zeros(K * d, device=dev())
        kc = torch.zeros(1, dtype=torch.int64, device=dev())
        tail = (nat.ptr(plan.flat), nat.ptr(x0), nat.ptr(t0), nat.ptr(xi), 42, 0, nat.ptr(tables), nat.ptr(path), nat.ptr(ahat),
                nat.ptr(VN), nat.ptr(YN), nat.ptr(XN), nat.ptr(tN), nat.ptr(kc), st)
        if which == "plain":
            nat.check(lib.psp_genl_rollout_fwd(C.byref(plan.gcfg), *tail), "psp_genl_rollout_fwd")
        else:
            nat.check(lib.psp_genl_rollout_fwd_eig(C.byref(plan.gcfg), None, *tail), "psp_genl_rollout_fwd_eig")
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in (VN, YN, XN, tN, kc, tables, ahat.view(torch.int32), path.view(torch.int32))])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert int(outs[0][4]) > 0
