"""The case table of the PINN kernel tests (pinn_kernel_cases.py) without a GPU: every route is claimed and psp_pinn_query confirms
the claim, every case lies in the regime where the bound 8 e_torch32 + 1e-6 means something, the float64 statement is consistent
with itself, and the checks reject nine planted errors, each made from the float64 numbers or a switch in the statement; the
first of them the one global norm they replace accepts."""
import ctypes as C

import pytest
import torch

import pinn_kernel_cases as kc
import ref64_pinn as r64

nat = kc.nat
NAMES = sorted(kc.CASES)


def query(case, K=None, **over):
    c = kc.pinn_config(case, K)
    keep = None
    if case["drift"] is not None:                                  # the query only asks that the pointer is there
        keep = (C.c_float * case["d"])()
        c.drift = C.cast(keep, C.c_void_p)
    for k, v in over.items():
        setattr(c, k, v)
    sz = nat.PinnSizes()
    return nat.load().psp_pinn_query(C.byref(c), C.byref(sz)), sz


def row_stride(tot):
    a = (tot + 3) & ~3
    while a & 63 != 4:
        a += 4
    return a


def lds_bytes(n_in, arch, backward):
    """pinn_lds_bytes (csrc/pinn_kernels.h): the concatenation image (and its adjoint), a pre-activation image per layer, 96 floats."""
    return 4 * ((2 if backward else 1) * 16 * row_stride(n_in + sum(arch)) + len(arch) * 16 * 132 + 96)


def derived_routes(name):
    """The routes a case's shape reaches, from its arguments and psp_pinn_query alone."""
    kw = kc.CASES[name][0]
    case = kc.make(name)
    rc, sz = query(case)
    assert rc == 0, nat.last_error()
    d, n_in, K, nblk, G = kw["d"], kc.n_in_of(case), kw["K"], sz.dir_blocks, sz.bwd_workgroups
    out = set()
    if sz.tiles > kc.MAX_FWD_WG:
        out.add("forward stride")
    if sz.tiles > G:
        out.add("backward stride")
        if G % nblk:                                               # tile g and tile g + G lie in different direction blocks
            out.add("mixed blocks in one workgroup")
        if sz.tiles % G:
            out.add("unequal tiles per workgroup")
    if n_in >= kc.DIRS:
        out.add("full block")
    if kw["parabolic"] and d % kc.DIRS == 0:
        out.add("time-only block")
    for w in (128, 1, 16, 17):
        if w in kw["arch"]:
            out.add("width %d" % w)
    if n_in in (112, 1):
        out.add("n_in %d" % n_in)
    out.add("K = 1" if K == 1 else "K = 64" if K == 64 else "K > 64" if K > 64 else "K < 64")
    out.add("h " + {r64.H_ZERO: "zero", r64.H_QUAD: "quad", r64.H_ALLEN_CAHN: "allen-cahn", r64.H_EXP_LIN: "exp-lin",
                    r64.H_EXP_SQ: "exp-sq", r64.H_EXP_SIN: "exp-sin"}[kw["h_kind"]])
    drift = kw.get("drift_kind", r64.DRIFT_ZERO)
    out.add("drift " + {r64.DRIFT_ZERO: "zero", r64.DRIFT_DIAG: "diag", r64.DRIFT_DWELL: "double-well"}[drift])
    out.add(kw["act"] + (" linear" if kw.get("linear") else ""))
    if kw["h_kind"] >= r64.H_EXP_LIN and kw["h_par"][2] != 0.0:
        out.add("e != 0")
    if kw["h_kind"] == r64.H_QUAD and case["s"] ** 2 != 1.0:
        out.add("s != 1")
    if kw.get("linear") and kw["arch"][0] == n_in:
        out.add("square first weight in the linear layout")
    if drift == r64.DRIFT_DWELL and kw["h_kind"] in (r64.H_ALLEN_CAHN, r64.H_EXP_SQ, r64.H_EXP_SIN):
        out.add("double-well with an h that reads V")
    if len(kw["arch"]) == 4:
        out.add("four layers")
    return out


def test_every_route_is_claimed_and_every_claim_holds():
    claimed = set()
    for name in NAMES:
        routes = set(kc.CASES[name][1])
        assert routes <= set(kc.ROUTES), (name, routes - set(kc.ROUTES))
        assert routes <= derived_routes(name), (name, routes - derived_routes(name))
        claimed |= routes
    assert claimed == set(kc.ROUTES), set(kc.ROUTES) - claimed


@pytest.mark.parametrize("name", NAMES)
def test_query_confirms_the_launch_shape(name):
    case = kc.make(name)
    rc, sz = query(case)
    assert rc == 0, nat.last_error()
    assert (sz.dir_blocks, sz.tiles, sz.bwd_workgroups) == kc.CASES[name][2]
    assert sz.tiles == case["K"] * kc.dir_blocks(case) and sz.bwd_workgroups == min(sz.tiles, kc.MAX_BWD_WG)
    assert sz.scratch_bytes == 4 * kc.scratch_floats(case)
    assert sz.grad_partial_bytes == 4 * sz.bwd_workgroups * sz.n_params
    assert sz.n_params == sum(p.numel() for p in case["params"])
    n_in = kc.n_in_of(case)
    assert sz.lds_fwd_bytes == lds_bytes(n_in, case["arch"], False) and sz.lds_bwd_bytes == lds_bytes(n_in, case["arch"], True)
    routes = kc.CASES[name][1]
    if "backward stride" in routes:
        assert sz.tiles > sz.bwd_workgroups
    if "forward stride" in routes:
        assert sz.tiles > 1024
    if name == "max_lds":                                          # the config range's largest net: nothing asks for more LDS
        rc, largest = query(dict(case, d=112, parabolic=False), K=8)
        assert rc == 0 and sz.lds_bwd_bytes == largest.lds_bwd_bytes == 116608 and sz.lds_bwd_bytes > 65536
        assert row_stride(112 + 4 * 128) == 644


def test_one_hot_samples_sit_where_the_table_says():
    for name, (last, second) in kc.ONE_HOT.items():
        nblk, tiles, G = kc.CASES[name][2]
        assert last == kc.CASES[name][0]["K"] - 1
        assert {(second * nblk + b) // G for b in range(nblk)} == {1}         # every tile of it is its workgroup's second
        assert (last * nblk) // G >= 2


def test_one_past_each_limit_is_refused():
    case = kc.make("d1_k1")
    assert query(dict(case, d=113))[0] == -2 and "112" in nat.last_error()
    assert query(dict(case, d=112, parabolic=True))[0] == -2
    assert query(dict(case, arch=[5, 129]))[0] == -2 and "128" in nat.last_error()
    assert query(dict(case, arch=[5, 3, 3, 3]), n_hidden=5)[0] == -2 and "hidden layers" in nat.last_error()
    assert query(dict(case, d=112, arch=[128, 128, 128, 128]))[0] == 0


@pytest.mark.parametrize("name", NAMES)
def test_regime_and_the_statements_pass_their_own_checks(name):
    ref = kc.reference(name)
    case, f64 = ref["case"], ref["f64"]
    if case["act"] == "relu2":                                     # phi'' jumps at 0: no comparison across a sign flip
        assert r64.preact_margin(case) >= 1e-5
    rows32 = kc.evaluate(ref, kc.as_native(ref["f32"], case))
    rows64 = kc.evaluate(ref, kc.as_native(f64, case))
    kc.assert_rows(rows32)
    kc.assert_rows(rows64)
    assert all(r[1] == 0.0 for r in rows64)
    for label, _, e32, bnd, _ in rows32:                           # the yardstick is sharp everywhere: the bound is never vacuous
        assert e32 <= kc.REGIME_CAP and bnd <= 4.1e-5, (label, e32)
    for key, g in f64["grads"].items():
        top = float(g.abs().max())
        assert top > 0.0
        for blk, v in r64.blocks(case, g).items():
            m = float(v.abs().max())
            assert m == 0.0 or m >= 1e-6 * top, (key, blk, m, top)
    assert sum(v.numel() for v in r64.blocks(case, f64["grads"]["loss"]).values()) == sum(p.numel() for p in case["params"])
    assert list(r64.blocks(case, f64["grads"]["loss"]))[-2:] == ["Wout", "bout"]


def test_output_bias_gradient_vanishes_exactly_where_h_does_not_read_v():
    """By the statement, not by a list: H_ZERO and H_QUAD leave the output bias out of R; H_EXP_LIN = -y lin does not."""
    zero = {n for n in NAMES if float(r64.blocks(kc.make(n), kc.reference(n)["f64"]["grads"]["random"])["bout"].abs().max()) == 0.0}
    assert zero == {"stride_fwd", "quad_diag"}


@pytest.mark.parametrize("name", ["odd_widths", "time_alone", "d1_k1"])
def test_weighted_grad_restates_loss_and_grad(name):
    case = kc.make(name)
    K = case["K"]
    for logvar in ((False, True) if K > 1 else (False,)):
        R, _, g = r64.loss_and_grad(case, alpha0=kc.ALPHA0, log_variance=logvar)
        rbar = (r64.variance_rbar if logvar else r64.mean_square_rbar)(kc.ALPHA0, K)(R)
        assert torch.allclose(r64.weighted_grad(case, rbar), g, rtol=1e-12, atol=1e-14)
        if K <= 20:
            each = sum(rbar[k] * r64.per_sample_grad(case, k) for k in range(K))
            assert torch.allclose(each, g, rtol=1e-12, atol=1e-14)
    V, gV, lap, Rp = r64.parts(case)
    assert torch.equal(Rp, r64.residual(case).detach()) and gV.shape == (K, kc.n_in_of(case)) and V.shape == lap.shape == (K,)


def test_the_existing_kernel_shapes_keep_their_tensors():
    """make_case and residual are what test_gpu_pinn.py has always used: the same draws in the same order."""
    from pinn_cases import GPU_SHAPES
    kw = GPU_SHAPES["d16_par_a24_40_8"]
    case = r64.make_case(**kw)
    g = torch.Generator().manual_seed(kw["seed"])
    W1 = torch.randn(17, 24, generator=g) / 17 ** 0.5
    assert torch.equal(case["params"][0], W1.double())
    R, _, grad = r64.loss_and_grad(case)
    assert torch.equal(r64.parts(case)[3], R) and torch.equal(r64.weighted_grad(case, (2.0 / kw["K"]) * R), grad)


# ---- planted errors: the checks must reject each, and the global norm is shown to accept those it was blind to ------------------
def rejected(ref, got):
    return not all(r[4] for r in kc.evaluate(ref, got))


def with_grad(ref, key, g):
    got = kc.as_native(ref["f64"], ref["case"])
    got["grads"][key] = g
    return got


def test_planted_1_smallest_block_off_by_one_percent():
    """The block check rejects 1 % in the smallest block.  What the global norm makes of such an error is its size times the
    block's share of the flat maximum: at this seed the smallest block (the width-1 layer's bias) is 3e-3 of it, so 1 % reads
    3e-5 there, and an error of 2e-4 -- five times the ceiling 4.1e-5 of the per-block bound -- reads 6e-7 and passes the
    constant 1e-6 of the global bound whatever the yardstick gives.  (A block that is smaller still only by cancellation over
    the samples would let 1 % through, but its fp32 statement is then off by more than the regime cap.)"""
    ref = kc.reference("odd_widths")
    case, f64, f32 = ref["case"], ref["f64"], ref["f32"]
    ratio, key, blk = min((float(v.abs().max()) / float(g.abs().max()), key, blk) for key, g in f64["grads"].items()
                          for blk, v in r64.blocks(case, g).items() if float(v.abs().max()) > 0.0)
    assert ratio <= 4.5e-3, (ratio, key, blk)
    for scale, passes_global in ((1.01, None), (1.0002, True)):
        g = f64["grads"][key].clone()
        r64.blocks(case, g)[blk].mul_(scale)
        assert rejected(ref, with_grad(ref, key, g))
        assert kc.err(g, f64["grads"][key]) <= 1.0001 * (scale - 1.0) * ratio
        if passes_global:
            assert kc.global_norm_ok(g, f64["grads"][key], f32["grads"][key]) and (scale - 1.0) * ratio < 1e-6 < 4.1e-5 < scale - 1.0


def test_planted_2_and_3_only_the_first_trip_or_the_first_trip_twice():
    ref = kc.reference("stride_bwd")
    case = ref["case"]
    nblk, _, G = kc.CASES["stride_bwd"][2]
    first_trip = torch.arange(case["K"]) <= (G - 1) // nblk       # the samples that own one of tiles 0 .. G - 1
    rbar = ref["rbar"]["loss"]
    only = r64.weighted_grad(case, rbar * first_trip)
    twice = r64.weighted_grad(case, rbar * (1.0 + first_trip.double()))
    assert rejected(ref, with_grad(ref, "loss", only)) and rejected(ref, with_grad(ref, "loss", twice))


def test_planted_4_laplacian_over_the_time_column_too():
    ref = kc.reference("time_alone")
    case = ref["case"]
    wrong = kc.statement(case, ref["rbar"], torch.float64, lap_cols=case["d"] + 1)
    assert rejected(ref, kc.as_native(wrong, case))
    got = kc.as_native(ref["f64"], case)                           # the right sum, but the time-only block holds a part of it
    got["lap_parts"][:, 1] = 1e-30
    assert rejected(ref, got)


def test_planted_5_e_dropped_from_lin():
    ref = kc.reference("time_alone")
    case = ref["case"]
    a, dd, e, tau = case["h_par"]
    assert e != 0.0
    wrong = kc.statement(dict(case, h_par=(a, dd, 0.0, tau)), ref["rbar"], torch.float64)
    assert rejected(ref, kc.as_native(wrong, case))


def test_planted_6_first_weight_transposed():
    ref = kc.reference("stride_fwd")
    case = ref["case"]
    W1 = case["params"][0]
    assert case["linear"] and W1.shape == (16, 16)
    wrong = kc.statement(dict(case, params=[W1.t().contiguous()] + case["params"][1:]), ref["rbar"], torch.float64)
    assert rejected(ref, kc.as_native(wrong, case))


def test_planted_7_value_seed_dropped():
    ref = kc.reference("relu2_linear")
    case = ref["case"]
    wrong = kc.statement(case, ref["rbar"], torch.float64, detach_y=True)
    assert torch.equal(wrong["R"], ref["f64"]["R"])                # only the adjoint's seed is wrong
    assert rejected(ref, kc.as_native(wrong, case))


def test_planted_8_one_hot_gradient_of_the_neighbouring_sample():
    ref = kc.reference("stride_bwd")
    K = ref["case"]["K"]
    assert rejected(ref, with_grad(ref, "one-hot last", r64.per_sample_grad(ref["case"], K - 2)))
    assert torch.equal(ref["f64"]["grads"]["one-hot last"], r64.per_sample_grad(ref["case"], K - 1))


def test_planted_9_one_nan_in_a_block():
    ref = kc.reference("one_block")
    g = ref["f64"]["grads"]["variance"].clone()
    r64.blocks(ref["case"], g)["b1"][3] = float("nan")
    assert rejected(ref, with_grad(ref, "variance", g))
    with pytest.raises(AssertionError):
        kc.check_finite(ref["f64"]["R"], g, g)
    with pytest.raises(AssertionError):
        kc.check_padding("scratch", torch.tensor([float("nan"), 0.0]))
    kc.check_padding("scratch", torch.full((3,), float("nan")))
