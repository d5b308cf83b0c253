"""Solver(compute_gradient_variance=m) on the native DenseNet-control plan (plan_dense_native.DenseNativePlan.gradient_moments,
psp_dnet_rollout_bwd_sq, psp_gradvar_finish).

1. psp_gradvar_finish on hand-made partial buffers against its torch mirror (plan_dense_native.gradvar_combine, which
   tests/test_gradvar_plan_host.py holds to the per-sample definition): slices, gather, both loss kinds, NaN -> 0, inf kept, a
   negative mean kept, the clamp.
2. plan.gv_mean / plan.gv_var after the first iteration against tests/ref64_gradvar.py on the noise the kernels used, in the regime
   of tests/dense_block_cases.py: 'moment' and 'log-variance', non-adaptive / attached fp32 / attached with the f16x3 forward, on
   (12, 16, K 37, N 4) -> (16, 32), (20, 40, K 80, N 3) -> (32, 64), (70, 40, K 48, N 3) -> (112, 64), plus one learn_Y_0 case.  EACH of
   the 9 blocks of EACH set within 2e-4 of its own maximum.  The parameter gradient and the loss of that iteration are
   bit-identical to the same run with compute_gradient_variance=0 (the snapshot / restore of the images is clean).
3. End to end against the reference's recorded runs (tests/golden/gradvar_*.json) with noise='reference': plan_name 'native',
   loss_log within 1e-4, every rel matrix under the |rel| <= 30 filter (<= 15 % left out, exact zeros where the golden is 0).
   The filter's tolerance is 4x what the COMPOSITE plan attains on the same GPU against the same golden under the same filter
   (COMPOSITE_ON_GPU below, measured; the factor 4 is the raw-moment margin eps (1 + mean^2 / var) over the two-pass form).
4. Log plumbing: L = 5, m = 2 gives three entries, each the mean of plan.gv_rel of its iteration.

Measured on an MI355X.  Worst block of any set per route (instance / mode), grads_mean and grads_var, bound 2e-4:
  16x32/nonadaptive     mean 9.70e-07  var 1.50e-06      16x32/attached-fp32   mean 8.81e-07  var 1.40e-06      16x32/attached-f16x3  mean 8.98e-07  var 1.27e-06
  32x64/nonadaptive     mean 6.18e-07  var 9.16e-07      32x64/attached-fp32   mean 1.15e-06  var 2.26e-06      32x64/attached-f16x3  mean 7.34e-07  var 2.06e-06
  112x64/nonadaptive    mean 1.32e-06  var 2.62e-06      112x64/attached-fp32  mean 1.53e-06  var 3.22e-06      112x64/attached-f16x3 mean 9.65e-07  var 1.36e-06
i.e. the raw-moment combination in double costs nothing visible in this regime: every route is at the fp32-against-float64 floor.
End to end, worst relative error of a rel entry with golden |rel| <= 30 (K = 16: an entry with |rel| = 30 amplifies the fp32
rounding of the rollout thirtyfold, whichever plan computes it):
  golden                                   composite plan on the GPU   native plan
  gradvar_llgc2_moment_nonadaptive         3.338e-06                   1.862e-05
  gradvar_llgc2_moment_attached_learn_y0   3.386e-06                   1.726e-05
  gradvar_llgc2_logvar_nonadaptive         3.089e-06                   8.972e-06
  gradvar_llgc2_logvar_default_flags       4.198e-06                   1.587e-05
  gradvar_lqgc3_logvar_attached_cadence    6.632e-06                   2.357e-05
COMPOSITE_ON_GPU = 6.632e-06 is the composite plan's worst over the five goldens, the tolerance 4x that = 2.653e-05.  (The composite
plan repeats the reference's torch operations in the reference's order, so it stays closer to the CPU golden than a rollout with
another, equally valid, fp32 operation order can: the native figures are the rollout's rounding, not the moments' -- section 2.)
The whole file runs in 4 s.
"""
import ctypes as C
import math

import pytest
import torch

from conftest import load_golden
import dense_block_cases as dc
import gradvar_cases as gc
import ref64_gradvar as r64
from util_cases import assert_dense_blocks, dense_block_names, psp

pytestmark = pytest.mark.gpu
nat = psp.native
pdn = psp.plan_dense_native
BLOCK_TOL = 2e-4
# worst relative error of the composite plan's rel matrices on an MI355X against the goldens, entries with golden |rel| <= 30
COMPOSITE_ON_GPU = 6.632e-06
REL_TOL = 4 * COMPOSITE_ON_GPU
LOSS_TOL = 1e-4


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- 1. the finishing kernel ------------------------------------------------------------------------------------------------
def _finish(parts, gg, gidx, N, slices, PP, Pset, K, kind, csums):
    d = dev()
    bufs = [None if p is None else p.to(d).contiguous() for p in parts]
    ggd = None if gg is None else gg.to(d).contiguous()
    mean, var, rel = (torch.full((N, Pset), 7.0, dtype=torch.float32, device=d) for _ in range(3))
    step, scalar = torch.zeros(N, dtype=torch.float64, device=d), torch.zeros(1, dtype=torch.float32, device=d)
    cs, gi = csums.to(d), gidx.to(d)
    rc = nat.load().psp_gradvar_finish(nat.ptr(bufs[0]), nat.ptr(bufs[1]), nat.ptr(bufs[2]), nat.ptr(bufs[3]), nat.ptr(ggd), nat.ptr(gi),
                                       N, slices, PP, Pset, K, kind, nat.ptr(cs), nat.ptr(mean), nat.ptr(var), nat.ptr(rel),
                                       nat.ptr(step), nat.ptr(scalar), nat.stream_ptr(d))
    torch.cuda.synchronize()
    return rc, mean.cpu(), var.cpu(), rel.cpu(), scalar.cpu()


@pytest.mark.parametrize("loss,with_gg", [("moment", False), ("moment", True), ("log-variance", False)])
def test_finish_kernel_equals_its_mirror(loss, with_gg):
    gen = torch.Generator().manual_seed(9)
    N, slices, PP, Pset, K = 3, 4, 50, 31, 19
    gidx = torch.randperm(PP, generator=gen)[:Pset].to(torch.int64)
    parts = [torch.randn(N * slices, PP, generator=gen) for _ in range(4)]
    parts[1] = parts[1].abs() * 3 + parts[0] ** 2                        # Q: positive, above S^2 / K mostly
    parts[0][:, gidx[0]] = 0.0
    parts[1][:, gidx[0]] = 0.0                                           # a dead unit: NaN -> 0
    parts[0][:, gidx[1]] = 0.0                                           # mean exactly 0, var > 0: inf (moment without Gg)
    parts[1][:, gidx[2]] = 0.0                                           # sum f^2 = 0 < (sum f)^2 / K: the clamp
    gg = torch.randn(N, Pset, generator=gen) if with_gg else None
    csums = torch.tensor([1.7, 23.0], dtype=torch.float64)
    kind = nat.LOSS_MOMENT if loss == "moment" else nat.LOSS_LOG_VARIANCE
    use = [parts[0], parts[1], parts[2] if (with_gg or loss != "moment") else None, parts[3] if loss != "moment" else None]
    rc, mean, var, rel, scalar = _finish(use, gg, gidx, N, slices, PP, Pset, K, kind, csums)
    assert rc == 0
    red = lambda p: None if p is None else p.double().view(N, slices, PP).sum(1).index_select(1, gidx)
    wm, wv, wr, ws = pdn.gradvar_combine(red(use[0]), red(use[1]), red(use[2]), red(use[3]), gg, K, loss, float(csums[0]), float(csums[1]))
    assert torch.allclose(mean, wm, rtol=1e-6, atol=0) and torch.allclose(var, wv, rtol=1e-6, atol=0)
    fin = torch.isfinite(wr)
    assert torch.equal(torch.isfinite(rel), fin) and torch.equal(rel[~fin], wr[~fin])
    assert torch.allclose(rel[fin], wr[fin], rtol=1e-5, atol=0)
    if loss == "moment" and not with_gg:
        assert bool((rel[:, 0] == 0).all()) and bool((var[:, 0] == 0).all())          # NaN -> 0
        assert bool(torch.isinf(rel[:, 1]).all())                                     # inf kept
        assert bool((var[:, 2] == 0).all()) and bool((rel[:, 2] == 0).all())          # clamp
        assert bool((rel < 0).any()) and bool((mean[rel < 0] < 0).all())              # a negative mean stays negative
        assert math.isinf(float(scalar))
    else:
        assert math.isclose(float(scalar), float(ws), rel_tol=1e-5) or (math.isinf(float(scalar)) and math.isinf(float(ws)))


def test_finish_kernel_checks():
    z = torch.zeros(2, 8)
    gidx = torch.arange(4, dtype=torch.int64)
    cs = torch.zeros(2, dtype=torch.float64)
    assert _finish([z, z, None, None], None, gidx, 2, 1, 8, 4, 1, nat.LOSS_MOMENT, cs)[0] == -1             # K < 2
    assert _finish([z, z, None, None], None, gidx, 2, 1, 8, 4, 5, nat.LOSS_LOG_VARIANCE, cs)[0] == -1       # S[c^2], S[1] missing
    assert _finish([z, z, None, None], None, gidx, 2, 1, 8, 4, 5, nat.LOSS_WEIGHTS, cs)[0] == -1
    assert _finish([z, z, None, None], None, gidx, 2, 1, 8, 9, 5, nat.LOSS_MOMENT, cs)[0] == -1              # Pset > padded


# ---- 2. the plan against float64 --------------------------------------------------------------------------------------------
MODES = [("nonadaptive", False, "fp32"), ("attached-fp32", True, "fp32"), ("attached-f16x3", True, "f16x3")]
PLAN_CASES = [(s, loss, m) for s in gc.PLAN_SHAPES for loss in ("moment", "log-variance") for m in MODES]
WORST = {}


def _plan_case(shape, loss, mode, learn_y0=False):
    d, H, K, N, expect = shape
    tag, adaptive, mm = mode
    c = gc.block_case(d, H, K, N, expect, loss=loss, adaptive=adaptive, mode=mm)
    over = dict(learn_Y_0=True) if learn_y0 else {}
    model, plan, oprob, ocfg, onets = gc.forward_once(c, dev(), lr=0.001, compute_gradient_variance=1, **over)
    assert plan.matrix_mode == mm and plan.attached == adaptive and plan.gv_count == 1
    assert len(model.grads_rel_error_log) == 1
    gm, gv, gr = plan.gv_mean.cpu(), plan.gv_var.cpu(), plan.gv_rel.cpu()
    grad, loss_v = plan.grad.clone().cpu(), model.loss_log[0]
    base_model, base_plan, *_ = gc.forward_once(c, dev(), lr=0.001, compute_gradient_variance=0, **over)
    assert base_model.grads_rel_error_log == [] and base_plan.gv_count == 0
    assert torch.equal(base_plan.grad.cpu(), grad) and base_model.loss_log[0] == loss_v          # bit-identical training
    ref = r64.moments(oprob, ocfg, onets, dc.host_noise(int(model.seed), K, d, N), y0=0.0)
    name = "d%d-H%d-K%d-N%d-%s-%s%s" % (d, H, K, N, loss[:6], tag, "-y0" if learn_y0 else "")
    route = "%dx%d/%s" % (expect[0], expect[1], tag)
    assert bool(torch.isfinite(gm).all()) and bool(torch.isfinite(gv).all()) and bool((gv >= 0).all())
    try:
        em = assert_dense_blocks(gm.reshape(-1), ref["grads_mean"].reshape(-1), d, H, N, False, BLOCK_TOL, tag=name + " mean")
    finally:
        ev = assert_dense_blocks(gv.reshape(-1), ref["grads_var"].reshape(-1), d, H, N, False, BLOCK_TOL, tag=name + " var")
    for what, errs in (("mean", em), ("var", ev)):
        worst, s, blk = max((e, s, n) for s, es in enumerate(errs) for e, n in zip(es, dense_block_names(False)))
        if worst > WORST.get((route, what), (-1.0,))[0]:
            WORST[(route, what)] = (worst, blk, s, name)
    want = torch.sqrt(gv) / gm
    want[want != want] = 0
    # rel is the reference's rule applied to gv_mean, gv_var: the same zeros (NaN -> 0) and non-finite entries; the finite ones to
    # 1e-6 (the kernel's fp32 root and quotient are correctly rounded; a host library's may each be an ulp, 6e-8, off)
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(gr), fin) and torch.equal(gr[~fin], want[~fin]) and torch.equal(gr == 0, want == 0)
    assert torch.allclose(gr[fin], want[fin], rtol=1e-6, atol=0)
    return name


@pytest.mark.parametrize("shape,loss,mode", PLAN_CASES,
                         ids=["d%d-H%d-K%d-N%d-%s-%s" % (s[:4] + (l[:6], m[0])) for s, l, m in PLAN_CASES])
def test_plan_moments_match_float64(shape, loss, mode):
    try:
        _plan_case(shape, loss, mode)
    finally:
        if (shape, loss, mode) == PLAN_CASES[-1]:
            for (route, what), (e, blk, s, cid) in sorted(WORST.items()):
                print("worst block per route: %-26s %-4s %.2e (%s of set %d) %s" % (route, what, e, blk, s, cid))


def test_plan_moments_with_learn_y0():
    _plan_case(gc.PLAN_SHAPES[0], "moment", MODES[1], learn_y0=True)


# ---- 3. end to end against the reference's recorded runs ----------------------------------------------------------------------
def _golden_run(name, backend):
    rec = load_golden(name)
    torch.set_num_threads(1)
    model = gc.make_gradvar_solver(rec["case"], dev(), backend=backend, noise="reference")
    for z in model.z_n:
        z.to(dev())
    mats = []
    if backend == "torch":
        mats = gc.record_matrices(model)
    else:
        plan = model._choose_plan()
        inner = plan.gradient_moments

        def recording(out=None):
            r = inner(out=out)
            mats.append(plan.gv_rel.clone())            # a device copy: no sync
            return r

        plan.gradient_moments = recording
    model.train()
    torch.cuda.synchronize()
    return rec, model, [m.cpu() for m in mats]


def _worst_against_golden(rec, model, mats, rel_tol):
    exp = rec["expected"]
    assert len(model.loss_log) == len(exp["loss_log"])
    for got, want in zip(model.loss_log, exp["loss_log"]):
        assert math.isclose(got, want, rel_tol=LOSS_TOL), (got, want)
    assert len(mats) == len(exp["rel_matrices"]) == len(model.grads_rel_error_log)
    worst = 0.0
    for got, want in zip(mats, exp["rel_matrices"]):
        assert tuple(got.shape) == (exp["N"], exp["p"])
        w, left = gc.compare_rel(got, torch.tensor(want), rel_tol=rel_tol)
        worst = max(worst, w)
    return worst


@pytest.mark.parametrize("name", gc.RUN_CASES)
def test_native_plan_matches_the_reference_runs(name):
    rec, model, mats = _golden_run(name, "auto")
    assert model.plan_name == "native", model.plan_reason
    try:
        worst = _worst_against_golden(rec, model, mats, rel_tol=float("inf"))
        print("%s: native worst rel err %.3e (<= %.3e)" % (name, worst, REL_TOL))
    finally:
        _worst_against_golden(rec, model, mats, rel_tol=REL_TOL)


def composite_figures():
    """What COMPOSITE_ON_GPU is taken from: the composite plan (backend='torch') on this GPU against every golden."""
    for name in gc.RUN_CASES:
        rec, model, mats = _golden_run(name, "torch")
        assert model.plan_name == "torch"
        print("%s: composite-on-GPU worst rel err %.3e" % (name, _worst_against_golden(rec, model, mats, float("inf"))))


# ---- 4. log plumbing ----------------------------------------------------------------------------------------------------------
def test_log_plumbing():
    rec = load_golden("gradvar_lqgc3_logvar_attached_cadence")
    model = gc.make_gradvar_solver(rec["case"], dev(), noise="reference", L=5, compute_gradient_variance=2)
    plan = model._choose_plan()
    assert model.plan_name == "native"
    rels, inner = [], plan.gradient_moments

    def recording(out=None):
        r = inner(out=out)
        rels.append(plan.gv_rel.clone())
        return r

    plan.gradient_moments = recording
    model.train()
    torch.cuda.synchronize()
    assert len(model.loss_log) == 5 and len(model.grads_rel_error_log) == 3 and len(rels) == 3         # l = 0, 2, 4
    for got, rel in zip(model.grads_rel_error_log, rels):
        want = float(rel.double().mean())
        assert math.isclose(got, want, rel_tol=1e-6) or (math.isinf(got) and got == want), (got, want)


if __name__ == "__main__":
    composite_figures()
