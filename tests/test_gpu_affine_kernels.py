"""The linear-control kernels (csrc/aff_kernels.h: aff_fwd_kernel, aff_adj_kernel, aff_bwd_kernel) through the C ABI against the
float64 statement of the same operation (tests/ref64_affine.py), at every launch shape make_aff_plan can produce: 64- and 256-thread
workgroups with a ragged last one, single- and multi-stage gradient slices with a ragged last slice, the three d buckets exact and
padded, the 132 096-byte LDS launch, every coefficient kind, store_path 1 / 2 / 3, both u_L2 kinds, supplied and Philox noise
(tests/affine_kernel_cases.py; the table's regime and six planted errors are checked on the CPU, tests/test_ref64_affine.py).

Per run (case, store_path), every output pre-filled with NaN:
  forward   D, Y_out, XN_out, the u_L2 sums, the path-store X_n rows and images: each within 2e-5 max(1, max |ref|); padded columns
            exactly zero; no NaN in the extents psp_aff_sizes names;
  partials  per workgroup (sum D, sum D^2) = the float64 lane-order sums of the kernel's own D (bit for bit / 1e-12);
            psp_aff_terminal_reduce = their sum within 1e-12;
  sweep     image slot * sqrt(dt) against dL/dZ_n, per step within 2e-4 of the step's maximum; the X_n half untouched bit for bit;
  gradient  dM_n and dc_n separately, per step within 2e-4 of the block's own maximum; padded rows / columns of every partial exactly
            zero; two calls give equal bits.
The bounds are the project's existing ones (tests/test_gpu_affine_control.py, tests/test_gpu_dense_block_gradients.py).

Measured on an MI355X, worst per route (kernel error | the fp32 CPU run of the statement as yardstick; the test prints this table;
route = bucket / workgroup / drift-sigma / control / store_path; fwd = the largest of the forward outputs):
  16/T64/A0-BI/Affine/sp1                         fwd 5.3e-8 | 5.3e-8                          block 1.7e-7 | 2.9e-7
  16/T64/Adiag-BsI/Affine/sp1                     fwd 1.1e-7 | 1.2e-7                          block 3.4e-7 | 3.2e-7
  16/T64/Adiag-BI/Constant/sp1-nonadaptive        fwd 5.6e-7 | 5.9e-7                          block 8.7e-7 | 3.6e-7
  16/T256/Adiag-BsI/Linear/sp3                    fwd 1.3e-7 | 1.3e-7    sweep 1.6e-7 | 2.0e-7   block 3.9e-7 | 1.9e-6
  32/T64/Adense-BI/Linear/sp2                     fwd 1.7e-7 | 1.4e-7    sweep 1.0e-7 | 1.2e-7   block 3.2e-7 | 3.5e-7
  32/T64/Adwell-Bdense/Affine/sp2                 fwd 2.2e-7 | 2.2e-7    sweep 2.3e-7 | 2.0e-7   block 3.4e-7 | 3.8e-7
  32/T256/Adense-Bdense/Constant/sp1-nonadaptive  fwd 1.8e-7 | 1.8e-7                          block 1.5e-7 | 2.3e-7
  64/T64/Adense-Bdense/Affine/sp3                 fwd 1.7e-7 | 1.6e-7    sweep 6.5e-7 | 1.9e-7   block 5.2e-7 | 4.9e-7
  64/T64/Adiag-BsI/Linear/sp1-philox              fwd 2.6e-7 | 1.3e-7                          block 2.2e-7 | 3.8e-7
  64/T64/Adiag-BsI/Linear/sp2-philox              fwd 2.6e-7 | 1.3e-7    sweep 1.2e-7 | 1.3e-7   block 2.9e-7 | 4.8e-7
  64/T256/Adense-Bdense/Affine/sp1                fwd 4.1e-7 | 4.1e-7                          block 3.6e-7 | 4.5e-7
  64/T256/Adense-Bdense/Affine/sp2                fwd 3.5e-7 | 3.0e-7    sweep 3.8e-7 | 1.9e-7   block 3.8e-7 | 5.1e-7
i.e. every route is at the fp32-against-float64 floor: none is more than 3.5 times above its yardstick, none within a factor 30 of
the forward bound or 200 of the block bound; the file runs in 4 s.
"""
import ctypes as C
import functools

import pytest
import torch

import affine_kernel_cases as kc
from util_cases import psp

pytestmark = pytest.mark.gpu
nat = psp.native

def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def philox_stream(c, k_offset=0):
    """The stream the Philox runs draw from, materialised by the library with the REAL d (the counters do not see the bucket)."""
    K = kc.K_of(c)
    xi = torch.full((c["N"] + 1, K, c["d"]), float("nan"), device=dev())
    nat.check(nat.load().psp_philox_normal_fill(nat.ptr(xi), c["N"], K, c["d"], k_offset, kc.PHILOX_SEED, kc.PHILOX_ITER, None),
              "psp_philox_normal_fill")
    torch.cuda.synchronize()
    return xi.cpu()


@functools.lru_cache(maxsize=None)
def inputs(cid):
    c = kc.BY_ID[cid]
    return kc.build_inputs(c, philox_stream(c) if c["noise"] == "philox" else None)


@functools.lru_cache(maxsize=None)
def reference(cid, sp):
    """(float64 statement, fp32 statement) of one run: computed once, never modified."""
    c = kc.BY_ID[cid]
    return kc.reference(c, inputs(cid), sp), kc.reference(c, inputs(cid), sp, dtype=torch.float32)


class Native:
    """One run of a case on the device through psp_aff_query and the four entry points.  Every output starts as NaN."""

    def __init__(self, c, inp, sp, noise=None, k_offset=0, K_global=None):
        self.lib, self.c, self.sp, d = nat.load(), c, sp, dev()
        self.DB, self.K, self.N, self.d = kc.bucket(c["d"]), inp["K"], inp["N"], c["d"]
        DB, K, N = self.DB, self.K, self.N
        f32, nan = torch.float32, float("nan")
        up = lambda t, square=False: None if t is None else kc.pad(t.to(f32), DB, square).to(d)
        self.philox = (c["noise"] if noise is None else noise) == "philox"
        self.t = dict(drift=up(inp["drift"], c["drift"] == kc.R.DRIFT_DENSE), sigma=up(inp["sigma"], True), run=up(inp["run"]),
                      term=up(inp["term"]), ul2=up(inp["ul2"], c["ul2"] == kc.R.UL2_LINEAR), M=up(inp["M"], True), c=up(inp["c"]),
                      x0=up(inp["x0"]), xi=None if self.philox else up(inp["xi"]))
        assert self.t["xi"] is None or self.t["xi"].shape == (N + 1, K, DB)
        self.w = {k: inp[k].to(f32).to(d) for k in ("w", "mu", "nu", "wT")}
        self.ul2 = torch.full((K,), nan, device=d) if c["ul2"] is not None else None
        self.cfg = kc.make_config(c, sp, self.t, k_offset, K_global, self.ul2, noise)
        self.sz = kc.query(self.cfg)
        sz = self.sz
        assert sz.path_bytes == N * K * 2 * DB * 4 and sz.padded_params == DB * DB + DB
        assert sz.partial_bytes == N * sz.slices * sz.padded_params * 4 and sz.fwd_partial_bytes == sz.fwd_workgroups * 16
        self.path = torch.full((N, K, 2 * DB), nan, device=d)
        self.D, self.Y, self.XN = torch.full((K,), nan, device=d), torch.full((K,), nan, device=d), torch.full((K, DB), nan, device=d)
        self.fwd_partial = torch.full((sz.fwd_workgroups, 2), nan, dtype=torch.float64, device=d)
        self.partial = torch.full((N * sz.slices, sz.padded_params), nan, device=d)
        self.sums = torch.full((2,), nan, dtype=torch.float64, device=d)

    def forward(self):
        t = self.t
        nat.check(self.lib.psp_aff_rollout_fwd(C.byref(self.cfg), nat.ptr(t["M"]), nat.ptr(t["c"]), nat.ptr(t["x0"]),
                                               self.DB if t["x0"].dim() == 2 else 0, None, nat.ptr(t["xi"]), kc.PHILOX_SEED,
                                               kc.PHILOX_ITER, nat.ptr(self.path), nat.ptr(self.D), nat.ptr(self.XN), nat.ptr(self.Y),
                                               nat.ptr(self.fwd_partial), None), "psp_aff_rollout_fwd")
        nat.check(self.lib.psp_aff_terminal_reduce(C.byref(self.cfg), nat.ptr(self.fwd_partial), nat.ptr(self.sums), None),
                  "psp_aff_terminal_reduce")
        torch.cuda.synchronize()
        path = self.path.cpu()
        out = dict(D=self.D.cpu(), Y=self.Y.cpu(), XN=self.XN.cpu(), X=path[..., :self.DB], image=path[..., self.DB:])
        if self.ul2 is not None:
            out["ul2"] = self.ul2.cpu()
        return out

    def sweep(self):
        w, z = self.w, torch.zeros(self.K, device=dev())
        mu, nu, wT = (w["mu"], None, w["wT"] if self.c["explicit_wT"] else None) if self.sp == 2 else (z, w["nu"], None)
        nat.check(self.lib.psp_aff_adjoint_sweep(C.byref(self.cfg), nat.ptr(self.t["M"]), nat.ptr(self.path), nat.ptr(self.XN),
                                                 nat.ptr(mu), nat.ptr(nu), nat.ptr(wT), None), "psp_aff_adjoint_sweep")
        torch.cuda.synchronize()
        path = self.path.cpu()
        return path[..., :self.DB], path[..., self.DB:]

    def backward(self):
        """(dM (N, DB, DB) or None, dc (N, DB) or None, the partials): the slices of a step summed as the plan sums them."""
        w = self.w["w"] if self.sp == 1 else torch.ones(self.K, device=dev())
        self.partial.fill_(float("nan"))
        nat.check(self.lib.psp_aff_rollout_bwd(C.byref(self.cfg), nat.ptr(self.path), nat.ptr(w), nat.ptr(self.partial), None),
                  "psp_aff_rollout_bwd")
        torch.cuda.synchronize()
        S, DB = int(self.sz.slices), self.DB
        g = self.partial.view(self.N, S, -1)
        g = (g.sum(1) if S > 1 else g[:, 0]).cpu()
        dM = g[:, :DB * DB].view(self.N, DB, DB) if self.c["control"] != "Constant" else None
        dc = g[:, DB * DB:] if self.c["control"] != "Linear" else None
        return dM, dc, self.partial.cpu()


WORST = {}                   # route -> dict of the largest errors and yardsticks: printed by the last run of the module


def _report(route, **pairs):
    slot = WORST.setdefault(route, {})
    for k, (e, y) in pairs.items():
        if e >= slot.get(k, (-1.0, 0.0))[0]:
            slot[k] = (e, y)


def _print_worst():
    print("worst per route (kernel | fp32 yardstick; bounds: forward %.0e, sweep and blocks %.0e)" % (kc.D_TOL, kc.BLOCK_TOL))
    for route, slot in sorted(WORST.items()):
        print("  %-46s %s" % (route, "  ".join("%s %.2e | %.2e" % (k, e, y) for k, (e, y) in slot.items())))
    # 6e-8: one fp32 rounding, for a yardstick that happens to be exact
    far = [(r, k, e, y) for r, slot in WORST.items() for k, (e, y) in slot.items() if e > 20.0 * max(y, 6e-8)]
    print("routes more than 20x above their yardstick: %s" % (far if far else "none"))


@pytest.mark.parametrize("cid,sp", kc.RUNS, ids=["%s-sp%d" % r for r in kc.RUNS])
def test_kernels_match_the_float64_statement(cid, sp):
    c, inp = kc.BY_ID[cid], inputs(cid)
    ref, ref32 = reference(cid, sp)
    run = Native(c, inp, sp)
    print(kc.assert_route(c, run.sz))
    d, DB, tag, route = c["d"], run.DB, "%s-sp%d" % (cid, sp), kc.route(c, sp)
    try:
        # ---- forward
        got = run.forward()
        exp = kc.expected_forward(c, inp, ref, sp)
        yard = kc.forward_errors({k: v.float() for k, v in kc.expected_forward(c, inp, ref32, sp).items()}, exp, d)
        errs = kc.forward_errors(got, exp, d)
        print("%s [%s] forward (kernel | fp32 yardstick, <= %.0e): %s" % (tag, route, kc.D_TOL,
              "  ".join("%s %.2e | %.2e" % (k, errs[k], yard[k]) for k in errs)))
        _report(route, D=(errs["D"], yard["D"]), fwd=(max(errs.values()), max(yard.values())))
        kc.check_forward(got, exp, d, tag)
        if c["noise"] == "philox" and sp == 1:
            assert torch.equal(got["image"][..., :d], inp["xi"][1:]), "the store_path 1 image is not the materialised Philox stream"
        # ---- (sum D, sum D^2)
        sums = kc.check_partials(run.fwd_partial, got["D"], int(run.sz.fwd_threads), tag)
        red = run.sums.cpu()
        assert float(((red - sums).abs() / sums.abs().clamp_min(1e-300)).max()) <= 1e-12, (tag, red, sums)
        # ---- sweep
        if sp in (2, 3):
            X_after, image = run.sweep()
            assert torch.equal(X_after, got["X"]), (tag, "the sweep changed the X_n half of the path store")
            assert bool(torch.isfinite(image).all()) and not bool(image[..., d:].any()), (tag, "image after the sweep")
            eZ, yZ = kc.check_sweep(image[..., :d], inp["sqdt"], ref["dZ"], tag), max(kc.step_errors(ref32["dZ"], ref["dZ"]))
            print("%s sweep: dL/dZ %.2e | %.2e (<= %.0e)" % (tag, eZ, yZ, kc.BLOCK_TOL))
            _report(route, sweep=(eZ, yZ))
        # ---- gradient
        dM, dc, partial = run.backward()
        assert bool(torch.isfinite(partial).all()), (tag, "a partial nobody wrote")
        pm = partial[:, :DB * DB].view(-1, DB, DB)
        assert not bool(pm[:, d:, :].any()) and not bool(pm[:, :, d:].any()) and not bool(partial[:, DB * DB + d:].any()), \
            (tag, "padded rows / columns of a partial are not exactly zero")
        if dM is None:
            assert not bool(pm.any()), (tag, "a Constant control has no outer products")
        eg, blk = kc.check_gradient(None if dM is None else dM[:, :d, :d], None if dc is None else dc[:, :d], ref, tag)
        yg = max(max(kc.step_errors(ref32[n], ref[n])) for n in ("dM", "dc") if ref[n] is not None)
        print("%s gradient: worst block %.2e (%s) | %.2e (<= %.0e)" % (tag, eg, blk, yg, kc.BLOCK_TOL))
        _report(route, block=(eg, yg))
        again = run.backward()[2]
        assert torch.equal(partial, again), (tag, "two gradient calls differ")
    finally:
        if (cid, sp) == kc.RUNS[-1]:
            _print_worst()


def test_launch_shapes_on_the_device():
    """The routes of the table with the device's own CU count: both workgroup sizes, multi-stage slices, a ragged last slice."""
    ragged = []
    for c in kc.CASES:
        sizes = kc.query(kc.make_config(c, c["paths"][0]))
        kc.assert_route(c, sizes)
        if c["multi_stage"] and kc.ragged_last_slice(c, sizes):
            ragged.append(c["id"])
    print("multi-stage cases with a ragged last slice: %s" % ragged)
    assert ragged
    assert kc.k_big() == 64 * torch.cuda.get_device_properties(0).multi_processor_count + 17


def test_philox_noise_is_the_library_stream_at_any_offset():
    """The store_path 1 image is psp_philox_normal_fill(N, K, d_real, k_offset, seed, iter) bit for bit, at k_offset = 0 and at a
    non-zero k_offset with K_global > K_local; a supplied-noise run on the materialised stream gives the same D, path and partials."""
    c = kc.BY_ID["d49_philox"]
    d, K = c["d"], kc.K_of(c)
    for k_offset, K_global in ((0, None), (37, K + 100)):
        stream = philox_stream(c, k_offset)
        assert bool(torch.isfinite(stream).all()) and not bool(stream[0].any())
        inp = dict(inputs("d49_philox"), xi=stream)
        dev_run = Native(c, inp, 1, k_offset=k_offset, K_global=K_global)
        got = dev_run.forward()
        assert torch.equal(got["image"][..., :d], stream[1:]), k_offset
        host_run = Native(c, inp, 1, noise="supplied", k_offset=k_offset, K_global=K_global)
        same = host_run.forward()
        for k in got:
            assert torch.equal(got[k], same[k]), (k_offset, k)
        assert torch.equal(dev_run.fwd_partial, host_run.fwd_partial) and torch.equal(dev_run.sums, host_run.sums)
        assert torch.equal(dev_run.backward()[2], host_run.backward()[2])
    assert not torch.equal(philox_stream(c, 0)[1:], philox_stream(c, 37)[1:])
