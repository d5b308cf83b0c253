"""tests/ref64.py::iteration_dense (the float64 reference of one Solver iteration with a DenseNet control) and the per-set block
comparison of tests/util_cases.py, checked on the CPU:

  a. the fp32 oracle (orc.hjb_train, trace) against iteration_dense on the same fp32 problem data, nets and noise, for every distinct
     reference of tests/dense_block_cases.py: every block of every parameter set to 1e-5 of that block's own maximum, D to
     1e-5 max(1, |D|) -- the bounds tests/test_ref64.py holds the tanh nets to.  Measured: worst block 3.8e-6 (W2h1, the non-adaptive
     double well at d = 115), D at most 3.4e-7, so no relu(.)**2 case needed a lower scale or a wider bound; the test prints the
     worst block of each case;
  b. every case of the table is in the regime it was built for (asserted on the float64 reference): every block at least 1e-2 of
     its set's maximum, every set's maximum at least 0.1 of the global one, max |D| <= 50, between 0.2 and 0.8 of the hidden units
     with z > 0 in both layers at step N // 2, and a mean relu(z) of the active units of at least 0.1;
  c. five planted errors, each ACCEPTED by the whole-gradient criterion of tests/test_gpu_dense_control.py (max |g - g_ref| <= 2e-4
     max |g_ref|) and REJECTED by assert_dense_blocks at the same 2e-4.

Which d the Philox counters see: none.  philox_block's counter is (global trajectory, step, 4 b + q, iteration) and call (b, q)
supplies features 16 b + 4 r + q (csrc/hjb_kernels.h, oracle/philox_oracle.py); hjbd_fwd_kernel walks the blocks of the PADDED d
and zeroes the features >= d_real, psp_philox_normal_fill(d) walks ceil(d / 16) blocks and keeps the features < d.  So the stream of
the real features is the same for every d >= d_real, and both this file (philox_oracle.normal_stream) and the GPU test
(psp_philox_normal_fill) materialise it with the REAL d.
"""
import math

import pytest
import torch

import dense_block_cases as dc
import ref64
from oracle import philox_oracle
from util_cases import (assert_dense_blocks, dense_block_errors, dense_block_names, dense_grad_blocks, make_oracle, orc)

BLOCK_TOL = 1e-5            # iteration_dense against the fp32 oracle, per block of every set
D_TOL = 1e-5
FLAT_TOL = 2e-4             # the whole-gradient criterion of tests/test_gpu_dense_control.py


def cpu_noise(c):
    """The stream the case's kernels draw from: the host generator, or the numpy restatement of the device Philox stream (real d)."""
    if c["noise"] == "philox":
        return torch.from_numpy(philox_oracle.normal_stream(c["N"], c["K"], c["d"], 0, 42, 0)).float().permute(1, 2, 0).contiguous()
    return dc.host_noise(42, c["K"], c["d"], c["N"])


def _distinct():
    seen, out = set(), []
    for c in dc.CASES:
        if dc.reference_key(c) not in seen:
            seen.add(dc.reference_key(c))
            out.append(c)
    return out


DISTINCT = _distinct()


def oracle_trace(oprob, ocfg, nets, xi):
    """The fp32 oracle's first iteration on the given nets and noise (it ends with an Adam step: take the float64 reference first)."""
    z = list(nets) if ocfg.time_approx == "outer" else nets[0]
    N = int(math.floor(oprob.T / ocfg.delta_t))
    ref = orc.hjb_train(oprob, ocfg, step_models=(z, orc.ScalarY0(ocfg.lr), N), noise=[xi], trace=True)
    return ref["traces"][0], ref["loss_log"][0]


@pytest.mark.parametrize("c", DISTINCT, ids=[c["id"] for c in DISTINCT])
def test_iteration_dense_matches_the_fp32_oracle_per_block(c):
    xi = cpu_noise(c)
    r64 = dc.reference(c, lambda: xi)
    oprob, ocfg, nets = dc.scaled_oracle(c)
    tr, loss32 = oracle_trace(oprob, ocfg, nets, xi)
    assert r64["N"] == c["N"] and len(r64["sets"]) == (c["N"] if c["tmode"] == "outer" else 1)
    assert [tuple(b.shape) for s in r64["sets"] for b in s] == [tuple(g.shape) for g in tr["grads"]]
    D32 = -tr["Zsum_g"] if c["loss"] == "relative_entropy" else tr["D"]
    assert bool(torch.isfinite(r64["D"]).all()) and bool(torch.isfinite(D32).all())
    eD = float((r64["D"] - D32.double()).abs().max()) / max(1.0, float(r64["D"].abs().max()))
    g32 = torch.cat([g.reshape(-1) for g in tr["grads"]])
    inner = c["tmode"] == "inner"
    errs = assert_dense_blocks(g32, r64["grad"], c["d"], c["H"], len(r64["sets"]), inner, BLOCK_TOL, tag="fp32 oracle vs ref64 " + c["id"])
    worst, s, n = max((e, s, n) for s, es in enumerate(errs) for e, n in zip(es, dense_block_names(inner)))
    print("%s: D %.2e (<= %.1e)  worst block %.2e (%s of set %d)  loss %.9g / %.9g" % (c["id"], eD, D_TOL, worst, n, s, r64["loss"], loss32))
    assert eD <= D_TOL, eD
    from block_cases import first_loss_tol, loss_values
    assert math.isclose(loss32, r64["loss"], rel_tol=first_loss_tol(loss_values(c["loss"], r64["D"]), r64["loss"])), (loss32, r64["loss"])


@pytest.mark.parametrize("c", dc.CASES, ids=[c["id"] for c in dc.CASES])
def test_gpu_cases_are_in_the_regime(c):
    r = dc.reference(c, lambda: cpu_noise(c))
    inner = c["tmode"] == "inner"
    names = dense_block_names(inner)
    sets = dense_grad_blocks(r["grad"], c["d"], c["H"], len(r["sets"]), inner)
    assert len(names) == (12 if inner else 9) and all(len(bl) == len(names) for bl in sets)
    gmax, Dmax = float(r["grad"].abs().max()), float(r["D"].abs().max())
    low = []
    for s, bl in enumerate(sets):
        m = [float(b.abs().max()) for b in bl]
        low.append((min(m) / max(m), names[m.index(min(m))], max(m) / gmax, s))
    a1, a2 = r["z1"] > 0, r["z2"] > 0
    s1, s2 = float(a1.double().mean()), float(a2.double().mean())
    m1, m2 = float(r["z1"][a1].mean()), float(r["z2"][a2].mean())
    print("%s: max |D| %.3g  active %.2f %.2f  mean relu %.2f %.2f  smallest block %.2e (%s of set %d)  smallest set %.2f" %
          (c["id"], Dmax, s1, s2, m1, m2, min(low)[0], min(low)[1], min(low)[3], min(x[2] for x in low)))
    assert all(x[0] >= 1e-2 for x in low), low
    assert all(x[2] >= 0.1 for x in low), low
    assert math.isfinite(Dmax) and Dmax <= 50.0, Dmax
    assert 0.2 <= s1 <= 0.8 and 0.2 <= s2 <= 0.8, (s1, s2)
    assert m1 >= 0.1 and m2 >= 0.1, (m1, m2)


def test_every_route_of_the_family_is_in_the_table():
    """Instances with their backward formulation, both matrix modes on each, the SPEC forward, Philox noise off it, the adjoint sweep,
    the relative entropy, generic trajectory weights, the non-adaptive image, several slices, N = 1."""
    C = dc.CASES
    have = {(c["expect"], c["bwd"]) for c in C}
    for inst, bwd in (((16, 32), "kernel1"), ((32, 64), "kernel1"), ((64, 64), "kernel1"), ((112, 32), "kernel1"), ((32, 32), "kernel1"),
                      ((128, 32), "kernel1"), ((112, 64), "kernel2"), ((128, 64), "kernel2"), ((256, 64), "gemm"), ((256, 32), "gemm"),
                      ((16, 32), "gemm"), ((32, 64), "gemm")):
        assert (inst, bwd) in have, (inst, bwd)
        assert {c["mode"] for c in C if c["expect"] == inst} == {"fp32", "f16x3"}, inst
    assert any(c["spec"] and c["detach"] for c in C) and any(c["spec"] and not c["detach"] for c in C)
    assert any(c["noise"] == "philox" and not c["spec"] and c["mode"] == m for c in C for m in ("f16x3",))
    assert any(c["noise"] == "philox" and c["mode"] == "fp32" for c in C)
    assert {c["loss"] for c in C} == set(ref64.LOSSES)
    assert any(not c["adaptive"] for c in C) and any(c["N"] == 1 for c in C) and sum(c["slices_gt1"] for c in C) >= 4
    assert {c["kind"] for c in C} == set(ref64.KINDS) and 45 <= len(C) <= 50


# ---- c. planted errors -------------------------------------------------------------------------------------------------------------
def old_sweep_reference(tmode, kind, d, H, K, dt, T, detach=True):
    """float64 reference of a case of tests/test_gpu_dense_control.py::test_dense_shape_sweep_matches_oracle at ITS weights: the
    DenseNets' own initial state (0.1 randn, zero biases), the problem's own X_0."""
    kwargs = dict(d=d, off_diag=0.05, T=T, seed=42, delta_t=dt) if kind == "LQGC" else dict(d=d, off_diag=0.3 / d ** 0.5, T=T, seed=42)
    solver = dict(loss_method="log-variance", time_approx=tmode, adaptive_forward_process=True, detach_forward=detach,
                  early_stopping_time=None, L=1, lr=0.002, seed=42, delta_t=dt, K=K, u_l2_error_flag=False)
    case = dict(name="dsweep", family="solver", problem=dict(kind=kind, kwargs=kwargs), solver=solver)
    if tmode == "inner":
        case["net"] = dict(kind="densenet", arch=[H, H], seed=5)
    oprob, ocfg, om = make_oracle(case, L=1)
    N = om[2]
    z = [orc.DenseNetOracle(d, d, 0.002, arch=[H, H], seed=5 + n) for n in range(N)] if tmode == "outer" else om[0]
    return ref64.iteration_dense(oprob, ocfg, z, dc.host_noise(42, K, d, N)), N


def flat_error(g, g_ref):
    return float((g - g_ref).abs().max()) / float(g_ref.abs().max())


def check_planted(what, g, g_ref, d, H, n_sets, inner, where):
    """`where` = {(set, block name)}: accepted by the flat criterion, rejected per block, and only there."""
    names = dense_block_names(inner)
    errs = dense_block_errors(g, g_ref, d, H, n_sets, inner)
    flat = flat_error(g, g_ref)
    hit = {(s, n) for s, es in enumerate(errs) for n, e in zip(names, es) if e > FLAT_TOL}
    print("%s: flat %.2e (<= %.1e passes), blocks %s" % (what, flat, FLAT_TOL,
          "  ".join("%s[%d] %.2e" % (n, s, errs[s][names.index(n)]) for s, n in sorted(where))))
    assert flat <= FLAT_TOL, (what, flat)
    assert hit == set(where), (what, hit, where)
    assert all(e == 0.0 for s, es in enumerate(errs) for n, e in zip(names, es) if (s, n) not in where), (what, errs)
    with pytest.raises(AssertionError):
        assert_dense_blocks(g, g_ref, d, H, n_sets, inner, FLAT_TOL, tag=what)


def set_views(g, d, H, n_sets, inner):
    """Per set (W1, b1, W2, b2, W3, b3) as writable views of the flat gradient."""
    di = d + (1 if inner else 0)
    sizes = [di * H, H, (di + H) * H, H, (di + 2 * H) * d, d]
    out = []
    for s in g.view(n_sets, sum(sizes)):
        W1, b1, W2, b2, W3, b3 = torch.split(s, sizes)
        out.append((W1.view(di, H), b1, W2.view(di + H, H), b2, W3.view(di + 2 * H, d), b3))
    return out


def test_planted_errors_at_the_old_tests_own_weights():
    """('outer', 'LLGC', 3, 5, 37) of test_dense_shape_sweep_matches_oracle at its initial weights: W2[h1] of set 1 is 2.7e-5 of the
    flat maximum, so the block set to ZERO passes the flat criterion.  W1[x] x 1.05: set 0's is exactly zero there (every hidden unit
    of the step-0 net is), so x 1.05 changes nothing; it is planted in the set whose W1[x] is the smallest non-zero one (set 2,
    4.0e-3 of the maximum: 0.05 x 4.0e-3 = 1.99e-4 still passes)."""
    d, H, K = 3, 5, 37
    r, N = old_sweep_reference("outer", "LLGC", d, H, K, 0.05, 0.2)
    g_ref = r["grad"]
    assert N == 4 and max(max(es) for es in dense_block_errors(g_ref, g_ref, d, H, N, False)) == 0.0
    assert_dense_blocks(g_ref.float(), g_ref, d, H, N, False, FLAT_TOL, tag="fp32 rounding of the reference")     # what is right passes
    blocks = dense_grad_blocks(g_ref, d, H, N, False)
    assert all(float(b.abs().max()) == 0.0 for b in blocks[0][:-1]) and float(blocks[0][-1].abs().max()) > 0.0    # set 0: b3 only
    g = g_ref.clone()
    set_views(g, d, H, N, False)[1][2][d:] = 0.0
    check_planted("W2h1 of set 1 zeroed", g, g_ref, d, H, N, False, {(1, "W2h1")})
    w1x = [float(bl[0].abs().max()) for bl in blocks]
    s = min((s for s in range(N) if w1x[s] > 0.0), key=lambda s: w1x[s])
    g = g_ref.clone()
    set_views(g, d, H, N, False)[s][0].mul_(1.05)
    check_planted("W1x of set %d x 1.05" % s, g, g_ref, d, H, N, False, {(s, "W1x")})


def test_planted_time_row_and_bias_exchange_at_a_short_step():
    """A block 5 % off, or two sets' blocks exchanged, passes the flat criterion only where the block is below 4e-3 (2e-4) of the flat
    maximum -- never in the regime of the case table, whose blocks are all above 1e-2 of it, and not at the old tests' step either
    (W2[t] of ('inner', 'LLGC', 64, 64, 100): 4.8e-3; b1 of the ('outer', 'LLGC', 3, 5, 37) sets: 2.8e-3 .. 5e-2).  Both are planted
    at those tests' own initial weights with a shorter step, where the time feature n dt and the states X_n ~ sqrt(n dt) are smaller:
    W2[t] x 1.05 at dt = 0.02, b1 of sets 1 and 2 exchanged at dt = 1e-5."""
    d, H, K = 64, 64, 100
    r, N = old_sweep_reference("inner", "LLGC", d, H, K, 0.02, 0.07)
    assert N == 3
    g = r["grad"].clone()
    set_views(g, d, H, 1, True)[0][2][0].mul_(1.05)
    check_planted("W2t x 1.05", g, r["grad"], d, H, 1, True, {(0, "W2t")})
    d, H, K = 3, 5, 37
    r, N = old_sweep_reference("outer", "LLGC", d, H, K, 1e-5, 4.5e-5)
    assert N == 4
    g = r["grad"].clone()
    v, v_ref = set_views(g, d, H, N, False), set_views(r["grad"], d, H, N, False)
    v[1][1].copy_(v_ref[2][1])
    v[2][1].copy_(v_ref[1][1])
    check_planted("b1 of sets 1 and 2 exchanged", g, r["grad"], d, H, N, False, {(1, "b1"), (2, "b1")})


def test_planted_element_moved_to_the_neighbouring_padded_row():
    """What an off-by-(H_pad - H) in DenseNativePlan._gather_index would produce in a regime case: one element of W3[h2] of the LAST
    set lands one row further down (its own place reads zero).  The largest element whose move the flat criterion cannot see (both
    touched entries change by at most 2e-4 of the flat maximum) but which is more than 2e-4 of its block -- on the (128, 64) case of
    the variance loss, H = 50, whose W3[h2] has such elements (33 of 5880; most cases of the table have none)."""
    c = [c for c in dc.CASES if c["loss"] == "variance" and c["tmode"] == "outer"][0]
    d, H, N = c["d"], c["H"], c["N"]
    g_ref = dc.reference(c, lambda: cpu_noise(c))["grad"]
    W3_ref = set_views(g_ref, d, H, N, False)[N - 1][4]
    gmax, bmax = float(g_ref.abs().max()), float(W3_ref[d + H:].abs().max())
    picks = [(i, j) for i in range(d + H, d + 2 * H - 1) for j in range(d)
             if FLAT_TOL * bmax < abs(float(W3_ref[i, j]))
             and max(abs(float(W3_ref[i, j])), abs(float(W3_ref[i, j] - W3_ref[i + 1, j]))) <= 0.9 * FLAT_TOL * gmax]
    assert picks, "no element of W3[h2] of the last set is small enough for the flat criterion to miss"
    i, j = max(picks, key=lambda ij: abs(float(W3_ref[ij])))
    g = g_ref.clone()
    W3 = set_views(g, d, H, N, False)[N - 1][4]
    W3[i + 1, j] = W3_ref[i, j]
    W3[i, j] = 0.0
    check_planted("W3h2[%d, %d] of set %d moved one row down" % (i - d - H, j, N - 1), g, g_ref, d, H, N, False, {(N - 1, "W3h2")})


def test_set_floor_keeps_a_zero_block_in_the_comparison():
    """A block that is zero in the reference is held to BLOCK_FLOOR (1e-4) of ITS SET's maximum -- not of the whole gradient's, so a
    large set cannot hide a small one -- and is neither skipped nor divided by."""
    d, H, n_sets = 3, 2, 2
    per = d * H + H + (d + H) * H + H + (d + 2 * H) * d + d
    g_ref = torch.zeros(n_sets * per, dtype=torch.float64)
    g_ref[per - 1] = 1.0                                          # b3 of set 0
    g_ref[2 * per - 1] = 1e-3                                     # b3 of set 1: a set 1000 x smaller
    g = g_ref.clone()
    g[per] = 3e-11                                                # W1x of set 1: 3e-11 / (1e-4 * 1e-3) = 3e-4
    errs = dense_block_errors(g, g_ref, d, H, n_sets, False)
    assert math.isclose(errs[1][0], 3e-4, rel_tol=1e-9) and all(e == 0.0 for e in errs[0] + errs[1][1:])
    assert [b.numel() for b in dense_grad_blocks(g, d, H, n_sets, False)[0]] == [d * H, H, d * H, H * H, H, d * d, H * d, H * d, d]
    assert [b.numel() for b in dense_grad_blocks(torch.zeros(per + H + H + d), d, H, 1, True)[0]][9:] == [H, H, d]
    with pytest.raises(AssertionError):
        assert_dense_blocks(g, g_ref, d, H, n_sets, False, 2e-4)
