"""Per-block float64 tests of the PINN kernels (csrc/pinn_kernels.h) past one tile per workgroup: the case table, the float64 and
fp32 statements of every case, the device wrapper and the checks.

A tile is one sample times one block of 14 input columns.  psp_pinn_backward launches min(tiles, 256) workgroups and
psp_pinn_residual min(tiles, 1024); a workgroup that owns more than one tile walks them in a grid-stride loop, adds each into its
partial gradient and reuses its LDS images.  Every case below names the routes it is there for (ROUTES), and
test_pinn_kernel_cases.py asserts through psp_pinn_query that it reaches them.

The checks are plain functions of (native numbers, float64 numbers, fp32-statement numbers), so that the CPU tests can hand them
planted errors.  One bound throughout, the one of test_gpu_pinn.py: with e(v) = max|v - v64| / max|v64|, e_native <= 8 e_fp32 + 1e-6
(fp32 torch autograd on the CPU, same inputs, is the yardstick; 8 for another summation order, 1e-6 for a yardstick that happens
to be exact) -- applied per named parameter block, per column of grad V and per vector of K samples instead of once per tensor.
"""
import ctypes as C
import functools
import math

import torch

import ref64_pinn as r64
from util_cases import psp

nat = psp.native
ACT = {"relu2": nat.ACT_RELU2, "tanh2": nat.ACT_TANH2, "tanh": nat.ACT_TANH}
ALPHA0 = 1.3
DIRS, MAX_BWD_WG, MAX_FWD_WG = 14, 256, 1024        # kPinnDirs, kPinnMaxWg, the forward grid's cap (pinn_instance.hip)
REGIME_CAP = 5e-6                                    # e32 of every block: keeps 8 e32 + 1e-6 <= 4.1e-5 (checked on the CPU)

ROUTES = (
    "forward stride", "backward stride", "mixed blocks in one workgroup", "unequal tiles per workgroup", "full block",
    "time-only block", "width 128", "width 1", "width 16", "width 17", "n_in 112", "n_in 1", "K = 1", "K = 64", "K > 64",
    "h zero", "h quad", "h allen-cahn", "h exp-lin", "h exp-sq", "h exp-sin",
    "drift zero", "drift diag", "drift double-well",
    "relu2", "relu2 linear", "tanh2", "tanh2 linear", "tanh", "tanh linear",
    "e != 0", "s != 1", "square first weight in the linear layout", "double-well with an h that reads V", "four layers",
)

# name -> (make_case arguments, routes, what psp_pinn_query must answer: dir_blocks, tiles, bwd_workgroups)
CASES = {
    "stride_bwd": (dict(d=29, parabolic=False, arch=[16, 16], K=173, act="relu2", seed=0, h_kind=r64.H_ALLEN_CAHN),
                   ("backward stride", "mixed blocks in one workgroup", "unequal tiles per workgroup", "K > 64", "width 16",
                    "relu2", "drift zero", "h allen-cahn"), (3, 519, 256)),
    "stride_fwd": (dict(d=15, parabolic=True, arch=[16], K=521, act="tanh", seed=0, linear=True, h_kind=r64.H_ZERO,
                        drift_kind=r64.DRIFT_DIAG),
                   ("forward stride", "backward stride", "unequal tiles per workgroup", "K > 64", "tanh linear", "h zero",
                    "drift diag", "square first weight in the linear layout"), (2, 1042, 256)),
    "max_lds": (dict(d=111, parabolic=True, arch=[128, 128, 128, 128], K=40, act="tanh", seed=0, h_kind=r64.H_ALLEN_CAHN),
                ("backward stride", "full block", "width 128", "n_in 112", "four layers", "tanh"), (8, 320, 256)),
    "odd_widths": (dict(d=27, parabolic=True, arch=[128, 1, 17], K=65, act="tanh2", seed=3, linear=True, h_kind=r64.H_EXP_SQ,
                        h_par=(0.05, 27.0, 0.0, 0.0), drift_kind=r64.DRIFT_DWELL),
                   ("full block", "width 128", "width 1", "width 17", "K > 64", "tanh2 linear", "h exp-sq",
                    "drift double-well", "double-well with an h that reads V"), (2, 130, 130)),
    "time_alone": (dict(d=14, parabolic=True, arch=[16, 24], K=19, act="relu2", seed=8, h_kind=r64.H_EXP_LIN,
                        h_par=(0.5, -4.0, 0.75, 0.0), drift_kind=r64.DRIFT_DIAG),
                   ("time-only block", "full block", "h exp-lin", "e != 0", "relu2", "drift diag", "width 16"), (2, 38, 38)),
    "one_block": (dict(d=14, parabolic=False, arch=[20], K=64, act="tanh2", seed=0, h_kind=r64.H_EXP_SIN,
                       h_par=(0.05, 14.0, -0.5, 0.0)),
                  ("full block", "K = 64", "tanh2", "h exp-sin", "e != 0"), (1, 64, 64)),
    "d1_k1": (dict(d=1, parabolic=False, arch=[5, 3], K=1, act="tanh", seed=0, h_kind=r64.H_ALLEN_CAHN),
              ("n_in 1", "K = 1", "tanh"), (1, 1, 1)),
    "relu2_linear": (dict(d=16, parabolic=False, arch=[24, 40, 8], K=17, act="relu2", seed=0, linear=True,
                          h_kind=r64.H_ALLEN_CAHN, drift_kind=r64.DRIFT_DWELL),
                     ("relu2 linear", "drift double-well", "double-well with an h that reads V", "h allen-cahn"), (2, 34, 34)),
    "quad_diag": (dict(d=9, parabolic=True, arch=[12, 12, 12], K=30, act="tanh", seed=0, h_kind=r64.H_QUAD,
                       drift_kind=r64.DRIFT_DIAG, s=1.25),
                  ("h quad", "s != 1", "drift diag", "tanh"), (1, 30, 30)),
}
# one-hot weights at the last sample and at one whose tiles are all the second of their workgroup (tile = k * dir_blocks + block)
ONE_HOT = {"stride_bwd": (172, 100), "stride_fwd": (520, 200)}
DETERMINISM = ("stride_bwd", "max_lds")


def make(name):
    return r64.make_case(**CASES[name][0])


def n_in_of(case):
    return case["d"] + (1 if case["parabolic"] else 0)


def dir_blocks(case):
    return (n_in_of(case) + DIRS - 1) // DIRS


def scratch_floats(case, K=None):
    """V (K), lap (K, nblk), gradV (K, n_in), cV (K), cG (K, n_in): psp_pinn_sizes.scratch_bytes / 4."""
    return (case["K"] if K is None else K) * (2 + dir_blocks(case) + 2 * n_in_of(case))


def random_rbar(K, seed=1234):
    """Seeded fp32-representable weights with both signs and, from K = 3 on, exact zeros at every third sample."""
    w = torch.randn(K, generator=torch.Generator().manual_seed(seed)).float().double()
    if K >= 3:
        w[::3] = 0.0
        assert bool((w > 0).any()) and bool((w < 0).any())
    return w


def rbars(name, K, R64, alpha0=ALPHA0):
    """key -> weights (K,), fp32-representable, in the order the gradients are taken.  The loss's own weights are formed once,
    from the float64 residual, and handed to the kernel and to both statements alike: psp_pinn_backward is tested as the map
    rbar -> gradient.  (What the native R does to those weights is bounded by R's own check, and test_gpu_pinn.py keeps the
    end-to-end chain R -> rbar -> gradient.  A shift of mean R moves every weight of the variance form by the same amount, which
    the sum over the samples does not cancel: it would charge the backward kernel with the forward's rounding.)"""
    out = {"loss": r64.mean_square_rbar(alpha0, K)(R64), "random": random_rbar(K)}
    if K > 1:
        out["variance"] = r64.variance_rbar(alpha0, K)(R64)
    if name in ONE_HOT:
        last, second = ONE_HOT[name]
        out["one-hot last"], out["one-hot second trip"] = r64.one_hot(K, last), r64.one_hot(K, second)
    return {k: v.float().double() for k, v in out.items()}


def statement(case, weights, dtype, **switches):
    """The numbers the checks compare, by autograd in ``dtype``: V, gradV, lap, R and one flat gradient per entry of weights."""
    V, gV, lap, R = r64.parts(case, dtype, **switches)
    grads = dict(zip(weights, r64.weighted_grads(case, list(weights.values()), dtype, **switches)))
    return dict(V=V.double(), gradV=gV.double(), lap=lap.double(), R=R.double(), grads={k: g.double() for k, g in grads.items()})


def kernel_order_sum(c, nblk):
    """fp32 sum over the samples of c (K, n) in the order the kernels add: workgroup (k nblk) mod G takes sample k's tiles after
    those it already owns, and the G partials meet as reduce_grad_kernel sums them (eight slices w = u mod 8 in increasing
    order, then ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)))."""
    K, n = c.shape
    G = min(K * nblk, MAX_BWD_WG)
    part = torch.zeros(G, n, dtype=torch.float32)
    for k in range(K):
        part[(k * nblk) % G] += c[k]
    s = torch.zeros(8, n, dtype=torch.float32)
    for w in range(0, G, 8):
        s[:min(8, G - w)] += part[w:w + 8]
    return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))


def scalar_blocks_in_kernel_order(case, weights):
    """The fp32 statement's second answer for the single-entry blocks (the bias of a width-1 layer, the output bias): fp32 autograd
    per sample, the samples weighted and summed in fp32 in the kernels' order.  {key: flat (P,) float64, zero elsewhere}.

    Why: the yardstick of a block is the worst fp32 error over its entries.  Over many entries that is a fair measure of what
    fp32 does to the block; for one entry it is a single draw, which comes out near 0 now and then (the blocks are sums over
    the samples with cancellation) and would leave a correct kernel with the bare 1e-6.  So a single-entry block takes the
    larger of two draws of the same fp32 sum: autograd's order and the kernels'."""
    f32 = torch.float32
    params = [p.to(f32).clone().requires_grad_(True) for p in case["params"]]
    scal = [i for i, p in enumerate(params) if p.numel() == 1]
    R = r64.terms(case, params, f32)[3]
    per = torch.zeros(case["K"], len(scal), dtype=f32)
    for k in range(case["K"]):
        gs = torch.autograd.grad(R[k], [params[i] for i in scal], allow_unused=True, retain_graph=True)
        per[k] = torch.stack([torch.zeros((), dtype=f32) if g is None else g.reshape(()) for g in gs])
    offs = [sum(p.numel() for p in params[:i]) for i in scal]
    out = {}
    for key, w in weights.items():
        rbar = w.to(f32)
        flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.float64)
        flat[offs] = kernel_order_sum(rbar[:, None] * per, dir_blocks(case)).double()
        out[key] = flat
    return out


def build_reference(case, name=None, alpha0=ALPHA0):
    weights = rbars(name, case["K"], r64.parts(case)[3], alpha0)
    f32 = statement(case, weights, torch.float32)
    f32["grads_kernel_order"] = scalar_blocks_in_kernel_order(case, weights)
    return dict(name=name, case=case, rbar=weights, f64=statement(case, weights, torch.float64), f32=f32)


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(case, rbar, f64, f32): computed once per case, never modified."""
    return build_reference(make(name), name)


def as_native(numbers, case):
    """Statement numbers in the shape the kernels leave theirs: the Laplacian as parts per direction block (all of it in block 0)."""
    out = dict(numbers)
    lap = torch.zeros(case["K"], dir_blocks(case), dtype=torch.float64)
    lap[:, 0] = numbers["lap"]
    out["lap_parts"] = lap
    out["grads"] = dict(numbers["grads"])
    return out


# ---- the checks ------------------------------------------------------------------------------------------------------------
def bound(e32):
    return 8.0 * e32 + 1e-6


def err(v, v64):
    """max|v - v64| / max|v64|; NaN or inf anywhere in v gives inf."""
    v = v.detach().double().cpu()
    if not bool(torch.isfinite(v).all()):
        return math.inf
    return float((v - v64).abs().max()) / float(v64.abs().max())


def row(label, got, v64, v32, v32_other=None):
    """(label, e_native, e_fp32, bound, ok) of one compared vector; a vector float64 gives as exactly zero must be exactly zero.
    ``v32_other``: a second fp32 statement of a single-entry vector, the yardstick being the worse of the two."""
    if float(v64.abs().max()) == 0.0:
        ok = bool((got.detach().double().cpu() == 0.0).all())
        return (label + " (exactly 0)", 0.0 if ok else math.inf, 0.0, 0.0, ok)
    e, e32 = err(got, v64), err(v32, v64)
    if v32_other is not None and v64.numel() == 1:
        e32 = max(e32, err(v32_other, v64))
    return (label, e, e32, bound(e32), e <= bound(e32))


def global_norm_ok(g, g64, g32):
    """The check this file replaces, kept for the planted errors: one norm over the whole flat gradient."""
    return err(g, g64) <= bound(err(g32, g64))


def evaluate(ref, got):
    """Every comparison of one case as rows (label, e_native, e_fp32, bound, ok).  ``got``: R (K), V (K), gradV (K, n_in),
    lap_parts (K, nblk), grads {key: flat}."""
    case, f64, f32 = ref["case"], ref["f64"], ref["f32"]
    d, nblk = case["d"], dir_blocks(case)
    rows = [row("R", got["R"], f64["R"], f32["R"]), row("V", got["V"], f64["V"], f32["V"])]
    for j in range(n_in_of(case)):
        rows.append(row("gradV[:, %d]" % j, got["gradV"][:, j], f64["gradV"][:, j], f32["gradV"][:, j]))
    parts = got["lap_parts"].detach().double().cpu()
    assert parts.shape == (case["K"], nblk)
    rows.append(row("lap", parts.sum(1), f64["lap"], f32["lap"]))
    for b in range(nblk):
        if b * DIRS >= d:                                          # a block without a space direction adds nothing, in any order
            ok = bool((parts[:, b] == 0.0).all())
            rows.append(("lap part of block %d (exactly 0)" % b, 0.0 if ok else math.inf, 0.0, 0.0, ok))
    assert set(got["grads"]) == set(f64["grads"]), (sorted(got["grads"]), sorted(f64["grads"]))
    for key, g64 in f64["grads"].items():
        g, g32 = r64.blocks(case, got["grads"][key]), r64.blocks(case, f32["grads"][key])
        other = r64.blocks(case, f32["grads_kernel_order"][key])
        for blk, v64 in r64.blocks(case, g64).items():
            rows.append(row("grad[%s] %s" % (key, blk), g[blk], v64, g32[blk], other[blk]))
    return rows


def table(rows):
    return "\n".join("    %-34s e_native %.2e  e_torch32 %.2e  bound %.2e%s" % (r[0], r[1], r[2], r[3], "" if r[4] else "   <-- FAILS")
                     for r in rows)


def summary(rows):
    """Worst native error next to the fp32 statement's error of the same entry, per kind of check."""
    out = {}
    for label, e, e32, _, _ in rows:
        kind = "grad[%s]" % label[5:label.index("]")] if label.startswith("grad[") else label.split("[")[0].split(" ")[0]
        if kind not in out or e > out[kind][0]:
            out[kind] = (e, e32, label)
    return out


def assert_rows(rows):
    bad = [r for r in rows if not r[4]]
    assert not bad, "outside 8 e_torch32 + 1e-6:\n" + table(bad)


def check_finite(R, grad, partial_used):
    """After a call every entry of R, grad and the G x P partials in use is a number: no tile's result is missing."""
    for label, v in (("R", R), ("grad", grad), ("grad_partial[:G * P]", partial_used)):
        assert bool(torch.isfinite(v).all()), "%s: %d entries are not finite" % (label, int((~torch.isfinite(v)).sum()))


def check_padding(label, tail):
    """Buffer entries past what a call of K points owns still hold the NaN they were filled with."""
    assert bool(torch.isnan(tail).all()), "%s: %d padded entries were written" % (label, int((~torch.isnan(tail)).sum()))


def scratch_parts(scratch, K, nblk, n_in):
    """Views into a psp_pinn_residual scratch of K points by its documented layout (include/psp.h, psp_pinn_sizes)."""
    sizes = [K, K * nblk, K * n_in, K, K * n_in]
    V, lap, gV, cV, cG = torch.split(scratch[:sum(sizes)], sizes)
    return dict(V=V, lap_parts=lap.reshape(K, nblk), gradV=gV.reshape(K, n_in), cV=cV, cG=cG.reshape(K, n_in))


# ---- the device wrapper ----------------------------------------------------------------------------------------------------
def pinn_config(case, K=None):
    """(psp_pinn_config without its drift pointer, sizes or None, return code) -- psp_pinn_query needs no GPU."""
    c = nat.PinnConfig()
    c.d, c.K, c.has_time, c.n_hidden = case["d"], (case["K"] if K is None else K), int(case["parabolic"]), len(case["arch"])
    for i, h in enumerate(case["arch"][:4]):
        c.widths[i] = h
    c.activation, c.linear_layout = ACT[case["act"]], int(case["linear"])
    c.drift_kind, c.h_kind, c.sigma_scale = case["drift_kind"], case["h_kind"], case["s"]
    for i, v in enumerate(case["h_par"]):
        c.h_par[i] = v
    return c


class Native:
    """One case on the device through psp_pinn_query / psp_pinn_residual / psp_pinn_backward.  ``capacity``: the sample count the
    buffers are sized for (default: the case's K); ``K``: run the first K samples only.  R, the scratch, the partials and the
    gradient are filled with NaN before each call, so an entry no tile writes cannot pass for a result."""

    def __init__(self, case, capacity=None, K=None):
        self.lib, d = nat.load(), torch.device("cuda:0")
        f32 = torch.float32
        self.case, self.K = case, case["K"] if K is None else K
        self.capacity = self.K if capacity is None else capacity
        assert 0 < self.K <= self.capacity and self.K <= case["K"]
        self.drift = None if case["drift"] is None else case["drift"].to(d, f32).contiguous()
        cap = pinn_config(case, self.capacity)
        cap.drift = nat.ptr(self.drift)
        self.cap_sz = nat.PinnSizes()
        nat.check(self.lib.psp_pinn_query(C.byref(cap), C.byref(self.cap_sz)), "psp_pinn_query")
        c = pinn_config(case, self.K)
        c.drift = nat.ptr(self.drift)
        self.cfg, self.sz = c, nat.PinnSizes()
        nat.check(self.lib.psp_pinn_query(C.byref(c), C.byref(self.sz)), "psp_pinn_query")
        self.params = torch.cat([p.reshape(-1) for p in case["params"]]).to(d, f32).contiguous()
        assert self.params.numel() == self.sz.n_params
        self.x = case["x"][:self.K].to(d, f32).contiguous()
        self.t = case["t"][:self.K].to(d, f32).contiguous() if case["parabolic"] else None
        self.scratch = torch.empty(self.cap_sz.scratch_bytes // 4, dtype=f32, device=d)
        self.partial = torch.empty(self.cap_sz.grad_partial_bytes // 4, dtype=f32, device=d)
        self.R_buf = torch.empty(self.capacity, dtype=f32, device=d)
        self.R = self.R_buf[:self.K]
        self.grad = torch.empty(self.sz.n_params, dtype=f32, device=d)
        assert self.sz.scratch_bytes <= self.cap_sz.scratch_bytes and self.sz.grad_partial_bytes <= self.cap_sz.grad_partial_bytes

    def residual(self):
        for buf in (self.R_buf, self.scratch, self.partial, self.grad):
            buf.fill_(float("nan"))
        nat.check(self.lib.psp_pinn_residual(C.byref(self.cfg), nat.ptr(self.params), nat.ptr(self.x), nat.ptr(self.t),
                                             nat.ptr(self.scratch), nat.ptr(self.R_buf), None), "psp_pinn_residual")
        torch.cuda.synchronize()
        return self.R

    def backward(self, rbar):
        """(the scratch is the residual call's result and this call's input: it stays)"""
        rbar = rbar.to(self.params.device, torch.float32).contiguous()
        assert rbar.numel() == self.K
        for buf in (self.partial, self.grad):
            buf.fill_(float("nan"))
        nat.check(self.lib.psp_pinn_backward(C.byref(self.cfg), nat.ptr(self.params), nat.ptr(self.x), nat.ptr(self.t),
                                             nat.ptr(self.scratch), nat.ptr(rbar), nat.ptr(self.partial), nat.ptr(self.grad),
                                             None), "psp_pinn_backward")
        torch.cuda.synchronize()
        return self.grad

    def scratch_parts(self):
        """The documented layout of the scratch (include/psp.h): V (K), lap (K, nblk), gradV (K, n_in), cV (K), cG (K, n_in)."""
        return scratch_parts(self.scratch, self.K, self.sz.dir_blocks, n_in_of(self.case))

    def used(self):
        """(scratch floats, partial floats) this call owns."""
        return self.sz.scratch_bytes // 4, self.sz.bwd_workgroups * self.sz.n_params
