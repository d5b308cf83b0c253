"""Per-trajectory float64 tests of the control-ansatz Solver's u_L2 log (u_l2_error_flag=True, the reference's default) on every
forward that can write it.  What checked the log before is the MEAN over K against the reference's recorded u_L2_loss at 1e-4
(tests/test_gpu_parity.py); at the initial N(0, 0.01) weights that number is 99.1 % (llgc_d8_logvar_ul2) and 99.84 %
(llgc_d40_moment_ul2) sum_n |u*(t_n)|^2 dt, so 1e-4 of it accepts an error of 1 % and 6 % in Z, and it cannot see one wrong
trajectory among K (tests/test_ref64_ul2.py plants one).

Here every case of tests/ul2_cases.py runs ONE iteration on weights scaled until Z is O(1), and
  * ul2_k of every trajectory is held to tests/ref64_ul2.py on the noise the kernels used (Philox noise materialised by
    psp_philox_normal_fill): |ul2_k - ul2_64,k| <= bound max(1, max ul2_64), bound = 8 E32 + 5e-7 with E32 the error of the fp32
    torch stand-in on the same noise (1.1e-6 .. 2.0e-6, table in tests/test_ref64_ul2.py); the bf16 mode by
    e_kernel <= BF16_C e_model + bound against ref64.iteration(operands='bf16'); grid kind: trajectories within delta of a cell
    edge are left out, at most K / 8 of them;
  * model.u_L2_loss[0] equals sum(ul2) / K to 1e-6;
  * D, the loss and each of the seven gradient blocks are held to the float64 reference with the bounds of
    tests/test_gpu_block_gradients.py -- the forward instances with the log on are not the ones that file launches;
  * a second run of the case gives bit-equal ul2;
  * the f16x3 cases of the wide family give the D of their fp32 sibling bit for bit (HjbwLaunch::fwd_x3 returns the fp32 LOGU forward).

Forward instance per route (asserted on the plan: family, instance, matrix mode, store_path, which of ul2 / ul2_gain / ul2_tab):
  table-narrow-v1, -small-d, -100x64 (fp32), -rounds, -attached, -relent, -nonadaptive   hjb_fwd_kernel<D, H, MODE 0, FAST 0>
  table-narrow-v2 / -v3                                hjbs_fwd_kernel / hjbq_fwd_kernel, non-FAST (u_ref set)
  table-f16x3, -100x64 (f16x3), -sigma-basis / table-bf16     hjb_fwd_kernel<D, H, MODE 2 / MODE 1, FAST 0>, on both noises
  table-wide-fp32 / -f16x3 / -rounds                   hjbw_fwd_kernel<D, H, LOGU = true>; fwd_coop_tiles == 0 on Philox noise
  gains-*, grid-*                                      no u_ref: the FAST instances on Philox noise; the log is decoded from the
                                                       path store by HjbNativePlan._ul2_rows_from_path
Measured on an MI355X (68 cases in 12 s), worst per route, ul2 error (its bound) / D / worst gradient block:
  table-narrow-v1 1.6e-7 (1.3e-6) / 1.6e-7 / 4.0e-7    table-narrow-v2 1.5e-7 (1.6e-6) / 2.4e-7 / 4.8e-7
  table-narrow-v3 1.6e-7 (1.3e-6) / 1.4e-7 / 3.1e-7    table-small-d   1.3e-7 (1.1e-6) / 1.7e-7 / 4.1e-7
  table-100x64    1.2e-7 (1.5e-6) / 3.7e-7 / 8.3e-7    table-rounds    2.1e-7 (2.0e-6) / 2.3e-7 / 3.1e-7
  table-f16x3     1.5e-7 (1.3e-6) / 1.8e-7 / 3.7e-7    table-attached  1.5e-7 (1.6e-6) / 2.4e-7 / 4.1e-7
  table-relent    1.5e-7 (1.6e-6) / 2.5e-7 / 1.7e-7    table-nonadaptive 1.9e-7 (1.4e-6) / 1.9e-7 / 3.0e-7
  table-sigma-basis 6.7e-8 (1.4e-6) / 1.9e-7 / 2.6e-7  table-wide-fp32 = table-wide-f16x3 2.2e-7 (1.5e-6) / 2.1e-6 / 3.1e-6
  table-wide-rounds 1.5e-7 (1.8e-6) / 6.0e-7 / 6.5e-7  gains-d2        1.3e-7 (1.1e-6) / 1.4e-7 / 4.3e-7
  gains-fp32      2.1e-7 (1.9e-6) / 2.9e-7 / 4.3e-7    gains-f16x3     2.4e-7 (1.5e-6) / 2.0e-7 / 4.1e-7
  gains-48x32     3.1e-7 (1.6e-6) / 3.5e-7 / 7.1e-7    gains-attached  2.1e-7 (1.9e-6) / 2.9e-7 / 3.9e-7
  gains-relent    2.4e-7 (1.5e-6) / 2.2e-7 / 1.7e-7    gains-store4    2.2e-7 (1.9e-6) / 2.0e-7 / 3.2e-7
  gains-wide      2.2e-7 (1.3e-6) / 4.1e-7 / 1.5e-6    grid-dw1d       8.0e-8 (9.7e-7) / 9.9e-8 / 1.5e-7
  grid-dw30       1.2e-7 (1.4e-6) / 1.1e-7 / 5.7e-7 (no trajectory near a cell edge on the Philox stream; 0 of 112 at d = 1)
  bf16, e_kernel / e_model of ul2: table-bf16 2.0e-4 / 1.3e-3 and 1.2e-4 / 1.8e-3 on supplied noise (one hidden unit on the other
  bf16 neighbour, as in tests/test_gpu_bf16_blocks.py), 6.7e-8 / 1.4e-3 and 1.8e-7 / 1.4e-3 on Philox noise; gains-bf16
  5.2e-4 / 2.3e-3 while its D agrees to 1.4e-7: the decode forms Z_n = W3 h2 + b3 in fp32 from the stored fp32 h2, the kernel
  from bf16 operands -- 0.22 e_model, inside the criterion.
i.e. every fp32-grade route logs each trajectory at the fp32-against-float64 floor, a factor 5 .. 10 inside its bound.  The decode
of the path store holds for both kernel families, the three matrix modes and store_path 1 .. 4 as it stands.  What the tests did
find: HjbNativePlan.sizes was queried before u_ref was set and reported the cooperative forward (fwd_coop_tiles = 2) for the wide
f16x3 plans on Philox noise, which the library never launches with the log on; the plan now queries again.

psp_hjb_sizes tells the quad forward apart (fwd_workgroups = 4 tiles) and, at K = 9001, the tile-per-wave one (fewer workgroups
than tiles); at K <= 16 CUs variants 1 and 2 both report one workgroup per tile, so there the variant is what PSP_FWD_VARIANT pins.
"""
import pytest
import torch

import block_cases as bc
import ul2_cases as uc
from test_gpu_block_gradients import BLOCK_TOL, D_TOL, SWITCHES, assert_route, dev, philox_noise
from util_cases import BLOCK_NAMES, assert_blocks, flat_params, make_pkg_solver, psp

pytestmark = pytest.mark.gpu
MEAN_TOL = 1e-6             # the logged mean against sum(ul2) / K
Plan = psp.plan_native.HjbNativePlan


def run_case(c, monkeypatch):
    """The first iteration of the case on the GPU: (model, plan, K, ul2 (K,) as the iteration logged it)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    seen = {}
    rows_of = Plan._ul2_rows_from_path

    def rows(self):                                                       # (the backward may reuse slots of the path store: keep
        seen["rows"] = rows_of(self)                                      # what the iteration itself decoded)
        return seen["rows"].clone()

    monkeypatch.setattr(Plan, "_ul2_rows_from_path", rows)
    K = bc.case_K(c, torch.cuda.get_device_properties(dev()).multi_processor_count)
    model = make_pkg_solver(uc.style(c, K), dev(), backend="native", noise=c["noise"], L=1, mlp_dtype=c["mode"], **uc.solver_kwargs(c))
    _, _, z = uc.scaled_oracle(c, K)
    with torch.no_grad():
        for p in model.z_n.parameters():
            p.mul_(c["scale"])
    assert torch.equal(flat_params(model.z_n), flat_params(z))            # the same scaled weights on both sides
    assert model.u_l2_error_flag
    model.train()
    assert model.plan_name == "native" and model.N == c["N"], (model.plan_name, model.N)
    torch.cuda.synchronize()
    plan = model._native_plan
    ul2 = plan.ul2 if c["ukind"] == "table" else seen["rows"]
    assert ul2.shape == (K,) and ul2.dtype == torch.float32
    return model, plan, K, ul2.detach().cpu().clone()


def assert_ul2_route(c, model, plan, K):
    assert_route(c, model, plan)
    kinds = dict(table=plan.ul2 is not None, gains=plan.ul2_gain is not None, grid=plan.ul2_tab is not None)
    assert kinds == {k: k == c["ukind"] for k in kinds}, kinds
    assert plan.state_basis == c["plan_basis"], (plan.state_basis, plan.state_basis_reason)
    assert bool(plan.cfg.adaptive) == c["adaptive"]
    nt = (K + 15) // 16
    wg = int(plan.sizes.fwd_workgroups)
    v = c["env"].get("PSP_FWD_VARIANT")
    if plan.family == 2:
        assert int(plan.sizes.fwd_coop_tiles) == 0                        # make_plan: no cooperative forward with u_ref set
    elif v == "3":
        assert wg == 4 * nt
    elif v == "2":
        assert wg == nt
    elif v == "1" or c["mode"] != "fp32":
        assert wg <= nt and (K < 9001 or wg < nt), (wg, nt)


def errors_of(ul2, ref_ul2, scale, keep):
    return float((ul2.double() - ref_ul2).abs()[keep].max()) / scale


WORST = {}                   # route -> (ul2 error, bound, D error, worst block error, block, case id)
FP32_D = {}                  # (d, H, K, noise) -> D of the wide fp32 case


def _wide_fp32_D(c, K, monkeypatch):
    key = (c["d"], c["H"], c["K"], c["noise"])
    if key not in FP32_D:
        sib = [o for o in uc.CASES if o["mode"] == "fp32" and o["expect"] == c["expect"] and (o["d"], o["H"], o["K"], o["noise"]) == key][0]
        FP32_D[key] = run_case(sib, monkeypatch)[1].D.cpu().clone()
    return FP32_D[key]


@pytest.mark.parametrize("c", uc.CASES, ids=uc.IDS)
def test_per_trajectory_log_matches_the_float64_reference(c, monkeypatch):
    model, plan, K, ul2 = run_case(c, monkeypatch)
    assert_ul2_route(c, model, plan, K)
    draw = philox_noise if c["noise"] == "philox" else bc.host_noise
    noise = lambda: draw(int(model.seed), K, c["d"], c["N"])
    R = uc.references(c, K, noise)
    ref, u64, keep = R["r64"], R["r64"]["ul2"], ~R["near"]
    scale = max(1.0, float(u64.max()))
    assert bool(torch.isfinite(ul2).all())
    # ---- the log, per trajectory
    n_near = int(R["near"].sum())
    assert n_near <= K // 8, (n_near, K)
    assert R["bound"] <= D_TOL
    e = errors_of(ul2, u64, scale, keep)
    bf16 = c["mode"] == "bf16"
    if bf16:
        model64 = uc.bf16_model(c, K, noise)
        e_k, e_m = errors_of(ul2, model64["ul2"], scale, keep), errors_of(model64["ul2"], u64, scale, keep)
        print("%s: ul2 e_kernel %.2e  e_model %.2e  (<= %.2g e_model + %.2e)" % (c["id"], e_k, e_m, bc.BF16_C, R["bound"]))
    else:
        print("%s: ul2 %.2e (<= %.2e; E32 %.2e)  mean %.6g  max %.4g  %d near of %d" % (c["id"], e, R["bound"], R["E32"], float(u64.mean()),
                                                                                    float(u64.max()), n_near, K))
    # ---- the logged mean
    mean = float(ul2.double().sum()) / K
    e_mean = abs(model.u_L2_loss[0] - mean) / mean
    print("%s: u_L2_loss[0] %.8g  sum(ul2) / K %.8g  (%.1e)" % (c["id"], model.u_L2_loss[0], mean, e_mean))
    # ---- D, loss and the gradient blocks of these forward instances
    g = plan.grad.cpu()
    assert g.shape == ref["grad"].shape
    if bf16:
        got = dict(D=plan.D, loss=float(model.loss_log[0]), grad=g)
        ek, _ = bc.assert_bf16(c, got, model64, ref, bc.BF16_C, D_TOL, BLOCK_TOL, tag=c["id"])
        eD, errs = ek["D"], ek["blocks"]
    else:
        D, D_ref = plan.D.double().cpu(), ref["D"]
        assert D.shape == D_ref.shape and bool(torch.isfinite(D).all())
        eD = float((D - D_ref).abs().max()) / max(1.0, float(D_ref.abs().max()))
        tol_l = bc.first_loss_tol(bc.loss_values(c["loss"], D_ref), ref["loss"])
        el = abs(model.loss_log[0] - ref["loss"]) / abs(ref["loss"])
        print("%s: D %.2e (<= %.1e)  loss %.2e (<= %.1e)" % (c["id"], eD, D_TOL, el, tol_l))
        errs = assert_blocks(g, ref["grad"], c["d"], c["H"], BLOCK_TOL, tag=c["id"])
        assert eD <= D_TOL, eD
        assert el <= tol_l, (model.loss_log[0], ref["loss"])
    if bf16:
        assert e_k <= bc.BF16_C * e_m + R["bound"], (e_k, e_m, R["bound"])
    else:
        assert e <= R["bound"], (e, R["bound"], int((ul2.double() - u64).abs().argmax()))
    assert e_mean <= MEAN_TOL, (model.u_L2_loss[0], mean)
    worst = max(errs)
    e = e_k if bf16 else e                                                # (bf16 routes: e_kernel, against the bf16-operand model)
    if e > WORST.get(c["route"], (-1.0,))[0]:
        WORST[c["route"]] = (e, R["bound"], eD, worst, BLOCK_NAMES[errs.index(worst)], c["id"])
    # ---- the wide f16x3 forward with the log on IS the fp32 LOGU forward
    if c["expect"][0] == 2 and c["ukind"] == "table":
        if c["mode"] == "fp32":
            FP32_D[(c["d"], c["H"], c["K"], c["noise"])] = plan.D.cpu().clone()
        else:
            assert torch.equal(plan.D.cpu(), _wide_fp32_D(c, K, monkeypatch)), "the f16x3 plan did not run the fp32 LOGU forward"
    # ---- determinism
    again = run_case(c, monkeypatch)[3]
    assert torch.equal(again, ul2), "a second run of the case changed ul2"
    if c is uc.CASES[-1]:
        for route, (eu, b, d_, w, blk, cid) in sorted(WORST.items()):
            print("worst per route: %-20s ul2 %.2e (bound %.2e)  D %.2e  block %.2e (%s)  %s" % (route, eu, b, d_, w, blk, cid))
