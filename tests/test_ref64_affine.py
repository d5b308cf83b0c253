"""tests/ref64_affine.py (the float64 statement of the linear-control kernels, csrc/aff_kernels.h) and the case table of
tests/affine_kernel_cases.py, checked on the CPU:

  a. the statement against the project's fp32 oracle (orc.hjb_train with the case's module list, trace) on the seven affine goldens'
     cases and the SWEEP table of tests/affine_cases.py, with the real losses: w / mu / nu / wT are formed from the loss as
     plan_affine_native.iteration forms them.  D within 2e-5 max(1, |D|), each of dM_n, dc_n within 2e-4 of its own maximum;
  b. every case of the table is in the regime: finite D, each block's maximum at least 1e-2 of the larger block of its step, each
     step's maximum at least 0.1 of the gradient's (the conditions of tests/test_ref64_dense.py); the fp32 run of the statement is
     printed next to it;
  c. six planted errors, made from the float64 numbers, each REJECTED by the checks the GPU test applies to the kernels;
  d. the launch shapes the cases were built for, from psp_aff_query (no GPU needed).
"""
import functools

import numpy as np
import pytest
import torch

import affine_kernel_cases as kc
import ref64_affine as r64
from affine_cases import GOLDEN, SWEEP, make_affine_oracle
from conftest import load_golden
from oracle import philox_oracle
from util_cases import make_pkg_problem, orc, psp

aff = psp.plan_affine_native
CPU = torch.device("cpu")


# ---- a. the statement against the fp32 oracle ------------------------------------------------------------------------------------
def _loss_numbers(s, D, Y, K):
    """(attached, relent, kwargs of the statement's loss) from the loss, as plan_affine_native.iteration does."""
    loss, adaptive = s["loss_method"], s["adaptive_forward_process"]
    attached, relent = bool(adaptive and not s["detach_forward"]), loss == "relative_entropy"
    if relent:
        return attached, True, (dict(nu=torch.full((K,), 1.0 / K, dtype=torch.float64)) if attached else
                                dict(w=torch.full((K,), -1.0 / K, dtype=torch.float64)))       # L = mean(Zsum + g) = -mean D
    if loss == "log-variance":
        w = (2.0 / K) * (D - D.mean())
    elif loss == "moment":
        w = (2.0 / K) * D
    elif loss == "variance":
        E = torch.exp(D)
        w = (2.0 / (K - 1.0)) * (E - E.mean()) * E
    else:
        w = (torch.exp(D) if adaptive else torch.exp(D - Y)) / K
    if not attached:
        return False, False, dict(w=w)
    return True, False, dict(mu=w, wT=-Y * w if loss == "cross_entropy" else None)


ORACLE_CASES = [("golden:" + n, n) for n in GOLDEN] + [("sweep:" + t, t) for t in sorted(SWEEP)]


@pytest.mark.parametrize("tag,name", ORACLE_CASES, ids=[t for t, _ in ORACLE_CASES])
def test_statement_matches_the_fp32_oracle(tag, name):
    case = load_golden(name)["case"] if tag.startswith("golden:") else SWEEP[name]
    s = case["solver"]
    oprob, ocfg, (z, y0m, N) = make_affine_oracle(case, L=1)
    prob = make_pkg_problem(case["problem"], CPU)
    spec = prob.native_spec()
    d, K = oprob.d, s["K"]
    g = torch.Generator().manual_seed(7)
    x0n = torch.randn(K, d, generator=g) if s.get("random_X_0", False) else None
    xi = torch.randn(K, d, N + 1, generator=g)
    kind = case["control"]["kind"]
    with torch.no_grad():
        G = aff.linear_gains(z, CPU) if kind == "Linear" else None
        M = aff.effective_map(G, torch.stack([m.F for m in z])) if kind == "Linear" else \
            torch.stack([m.A for m in z]) if kind == "Affine" else None
        c = torch.stack([m.b[0] for m in z]) if kind == "Affine" else torch.stack([m.c.reshape(-1) for m in z]) if kind == "Constant" \
            else None
        y0 = float(y0m(oprob.X_0.repeat(K, 1))[0]) if s.get("learn_Y_0", False) else 0.0
    dt32 = torch.tensor(s["delta_t"])
    args = (d, K, N, float(dt32), float(torch.sqrt(dt32)), M, c, spec["drift"], spec["sigma"][:2], spec["runcost"], spec["term"],
            float(spec["sigma"][2]), s["adaptive_forward_process"])
    x0 = x0n if x0n is not None else oprob.X_0
    noise = xi.permute(2, 0, 1).contiguous()
    first = r64.statement(*args, False, x0, noise, y0=y0, w=torch.zeros(K), relent=s["loss_method"] == "relative_entropy")
    attached, relent, loss = _loss_numbers(s, first["D"], first["Y"], K)
    ref = r64.statement(*args, attached, x0, noise, y0=y0, relent=relent, **loss)
    out = orc.hjb_train(oprob, ocfg, step_models=(z, y0m, N), noise=[xi], x0_noise=None if x0n is None else [x0n], trace=True)
    tr = out["traces"][0]
    D32 = (-tr["Zsum_g"] if relent else tr["D"]).double()
    eD = float((ref["D"] - D32).abs().max()) / max(1.0, float(ref["D"].abs().max()))
    grads = [g_.double() for g_ in tr["grads"]]
    per = 2 if kind == "Affine" else 1
    assert len(grads) == per * N
    blocks = []
    if kind == "Linear":
        blocks.append(("dM", aff.chain_rule(None if G is None else G.double(), ref["dM"]), torch.stack(grads)))
    elif kind == "Affine":
        blocks.append(("dM", ref["dM"], torch.stack(grads[0::2])))
        blocks.append(("dc", ref["dc"], torch.stack([g_.reshape(-1) for g_ in grads[1::2]])))
    else:
        blocks.append(("dc", ref["dc"], torch.stack([g_.reshape(-1) for g_ in grads])))
    errs = {}
    for nm, mine, theirs in blocks:
        assert mine.shape == theirs.shape
        for n in range(N):
            errs["%s_%d" % (nm, n)] = float((mine[n] - theirs[n]).abs().max()) / max(float(mine[n].abs().max()), 1e-300)
    worst = max(errs, key=errs.get)
    print("%s: D %.2e (<= 2e-5)  worst block %.2e (%s, <= 2e-4)" % (tag, eD, errs[worst], worst))
    assert bool(torch.isfinite(ref["D"]).all()) and eD <= 2e-5, eD
    assert errs[worst] <= 2e-4, (worst, errs[worst])


# ---- b. the regime of the table ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(cid):
    c = kc.BY_ID[cid]
    xi = None
    if c["noise"] == "philox":                              # the numpy restatement of the device stream, with the real d
        xi = torch.from_numpy(np.asarray(philox_oracle.normal_stream(c["N"], kc.K_of(c), c["d"], 0, kc.PHILOX_SEED,
                                                                     kc.PHILOX_ITER))).float()
    return kc.build_inputs(c, xi)


@functools.lru_cache(maxsize=None)
def reference(cid, sp):
    """float64 statement of one run of the table: computed once, never modified."""
    return kc.reference(kc.BY_ID[cid], inputs(cid), sp)


@pytest.mark.parametrize("cid,sp", kc.RUNS, ids=["%s-sp%d" % r for r in kc.RUNS])
def test_case_is_in_the_regime(cid, sp):
    c, inp, ref = kc.BY_ID[cid], inputs(cid), reference(cid, sp)
    ref32 = kc.reference(c, inp, sp, dtype=torch.float32)
    lo_block, lo_step = kc.regime(ref)
    eD = float((ref32["D"].double() - ref["D"]).abs().max()) / max(1.0, float(ref["D"].abs().max()))
    _, eg = yardstick_gradient(ref32, ref)
    eZ = max(kc.step_errors(ref32["dZ"], ref["dZ"]))
    print("%s sp%d [%s]: max |D| %.3g  smallest block %.2f of its step  smallest step %.2f of the gradient  | fp32 statement: D %.2e"
          "  worst block %.2e  dL/dZ %.2e" % (cid, sp, kc.route(c, sp), float(ref["D"].abs().max()), lo_block, lo_step, eD, eg, eZ))
    assert bool(torch.isfinite(ref["D"]).all()) and bool(torch.isfinite(ref["dZ"]).all())
    assert lo_block >= 1e-2, lo_block
    assert lo_step >= 0.1, lo_step


def yardstick_gradient(ref32, ref):
    worst = (0.0, "-")
    for nm in ("dM", "dc"):
        if ref[nm] is not None:
            e = kc.step_errors(ref32[nm], ref[nm])
            worst = max(worst, (max(e), nm))
    return worst[1], worst[0]


def test_the_route_list_is_covered_by_the_table():
    Cs = kc.CASES
    assert {kc.bucket(c["d"]) for c in Cs if c["d"] == kc.bucket(c["d"])} == {16, 32, 64}             # exact
    assert {kc.bucket(c["d"]) for c in Cs if c["d"] != kc.bucket(c["d"])} == {16, 32, 64}             # padded
    assert any(c["d"] == 1 for c in Cs) and any(c["N"] == 1 for c in Cs)
    for T in (64, 256):
        assert any(c["threads"] == T and kc.K_of(c) % T for c in Cs), T                               # ragged last workgroup
    assert any(not c["multi_stage"] for c in Cs) and any(c["multi_stage"] for c in Cs)
    assert {c["drift"] for c in Cs} == {0, 1, 2, 3} and {c["sigma"] for c in Cs} == {0, 1, 2}
    assert {c["run"] for c in Cs} == {0, 1} and {c["term"] for c in Cs} == {0, 1, 2}
    assert {(c["drift"] == r64.DRIFT_DENSE, c["sigma"] == r64.SIGMA_DENSE) for c in Cs} == {(a, b) for a in (0, 1) for b in (0, 1)}
    assert {c["control"] for c in Cs} == {"Linear", "Affine", "Constant"}
    assert {(sp, c["adaptive"]) for c in Cs for sp in c["paths"]} == {(1, True), (1, False), (2, True), (3, True)}
    assert {c["explicit_wT"] for c in Cs if 2 in c["paths"]} == {True, False}
    assert {c["x0_rows"] for c in Cs} == {True, False}
    assert any(c["ul2"] == r64.UL2_TABLE for c in Cs) and any(c["ul2"] == r64.UL2_LINEAR and kc.bucket(c["d"]) == 64 for c in Cs)
    assert {c["noise"] for c in Cs} == {"supplied", "philox"}
    # the adjoint sweep's own branches: s * lam, the diagonal Jacobian, the double well's, dense A without dense B and the reverse
    swept = {(c["drift"], c["sigma"]) for c in Cs if set(c["paths"]) & {2, 3}}
    assert {(r64.DRIFT_DIAG, r64.SIGMA_SCALED), (r64.DRIFT_DENSE, r64.SIGMA_IDENTITY), (r64.DRIFT_DWELL, r64.SIGMA_DENSE),
            (r64.DRIFT_DENSE, r64.SIGMA_DENSE)} <= swept


# ---- c. planted errors ------------------------------------------------------------------------------------------------------------
def _rejected(check, *a):
    try:
        check(*a)
    except AssertionError as e:
        return str(e.args[0][1] if isinstance(e.args[0], tuple) and len(e.args[0]) > 1 else e)[:60]
    return None


def _gradient_check(got, ref):
    kc.check_gradient(got["dM"], got["dc"], ref, "planted")


def _forward_check(c, inp, ref, sp, got):
    exp = kc.expected_forward(c, inp, ref, sp)
    kc.check_forward({k: got[k] for k in exp}, exp, c["d"], "planted")


def _planted():
    """(name, the check that has to reject it, its arguments); each starts from the float64 numbers rounded to fp32."""
    out = []
    # 1. the last valid trajectory left out of the K_big gradient sum
    cid, sp = "d5_big_relent", 3
    c, inp, ref = kc.BY_ID[cid], inputs(cid), reference(cid, sp)
    assert kc.K_of(c) == kc.k_big()
    got = kc.kernel_like(c, inp, ref, sp)
    got["dM"] = (ref["dM"] - torch.einsum("ni,nj->nij", ref["dZ"][:, -1], ref["X"][:-1, -1])).float()
    out.append(("last trajectory left out of the K_big sum", _gradient_check, (got, ref)))
    # 2. dM_n transposed, 3. dc of two steps exchanged
    cid, sp = "d64_big_attached", 2
    c, inp, ref = kc.BY_ID[cid], inputs(cid), reference(cid, sp)
    got = kc.kernel_like(c, inp, ref, sp)
    got["dM"] = got["dM"].transpose(1, 2).contiguous()
    out.append(("dM_n transposed", _gradient_check, (got, ref)))
    got = kc.kernel_like(c, inp, ref, sp)
    got["dc"] = got["dc"][[1, 0, 2]].contiguous()
    out.append(("dc of two steps exchanged", _gradient_check, (got, ref)))
    # 4. the u_L2 LINEAR reference evaluated at X_n instead of X_{n+1}
    cid, sp = "d64_big_detached", 1
    c, inp, ref = kc.BY_ID[cid], inputs(cid), reference(cid, sp)
    got = kc.kernel_like(c, inp, ref, sp)
    got["ul2"] = kc.reference(c, inp, sp, ul2_at_old_state=True)["ul2"].float()
    out.append(("u_L2 LINEAR reference at X_n", _forward_check, (c, inp, ref, sp, got)))
    # 5. the sweep's delta_n without B^T: delta = direct - dt B^T Lam, so Lam = B^-T (direct - delta) / dt
    cid, sp = "d33_relent", 3
    c, inp, ref = kc.BY_ID[cid], inputs(cid), reference(cid, sp)
    dt = inp["dt"]
    direct = inp["nu"].double()[None, :, None] * dt * ref["Z"]
    Lam = torch.linalg.solve(inp["sigma"].double().t(), ((direct - ref["dZ"]) / dt).reshape(-1, c["d"]).t()).t().reshape(ref["dZ"].shape)
    wrong = ((direct - dt * Lam) / inp["sqdt"]).float()
    out.append(("sweep without B^T", kc.check_sweep, (wrong, inp["sqdt"], ref["dZ"], "planted")))
    # 6. one X_N row taken from the neighbouring trajectory
    cid, sp = "d17_denseA_identB", 2
    c, inp, ref = kc.BY_ID[cid], inputs(cid), reference(cid, sp)
    got = kc.kernel_like(c, inp, ref, sp)
    got["XN"][5] = got["XN"][6]
    out.append(("X_N row of the neighbour", _forward_check, (c, inp, ref, sp, got)))
    return out


def test_planted_errors_are_rejected_and_the_float64_numbers_pass():
    # the unplanted numbers pass every check (so that a rejection below is the planted error's)
    for cid, sp in (("d5_big_relent", 3), ("d17_denseA_identB", 2), ("d64_big_detached", 1)):
        c, inp, ref = kc.BY_ID[cid], inputs(cid), reference(cid, sp)
        got = kc.kernel_like(c, inp, ref, sp)
        _forward_check(c, inp, ref, sp, got)
        _gradient_check(got, ref)
        kc.check_sweep(got["dZ"] / inp["sqdt"], inp["sqdt"], ref["dZ"])
    planted = _planted()
    assert len(planted) == 6
    for name, check, args in planted:
        why = _rejected(check, *args)
        print("planted: %-44s %s" % (name, "rejected by the %s check" % why if why else "ACCEPTED"))
        assert why is not None, name


# ---- d. launch shapes -------------------------------------------------------------------------------------------------------------
def test_launch_shapes_of_the_table():
    ragged = []
    for c in kc.CASES:
        sizes = kc.query(kc.make_config(c, c["paths"][0]))
        print(kc.assert_route(c, sizes))
        if c["multi_stage"] and kc.ragged_last_slice(c, sizes):
            ragged.append(c["id"])
    assert ragged, "no multi-stage case has a ragged last slice"
    assert kc.k_big() == 64 * 256 + 17 or torch.cuda.is_available()
