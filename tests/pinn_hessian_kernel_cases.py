"""Float64 per-block tests of the direction-table route of the PINN kernels (csrc/pinn_kernels.h, PSP_GENL_SIGMA_DENSE): the case
table, both statements of every case, the device wrapper and the checks.

A sample's directions are n_grad unit vectors (grad V, V_t; not counted in the Laplacian row) and then n_hess rows of the table
(counted; no first derivative stored, adjoint seed 0); a tile is one sample times one block of 14 of them.  The cases are the
smallest shapes that reach every route of that layout.  The bound, the error measure, the rbar forms and the row format are
pinn_kernel_cases'; so is the second fp32 draw of a single-entry block.
"""
import ctypes as C
import functools

import torch

import pinn_kernel_cases as kc
import ref64_pinn as r64
import ref64_pinn_dense as r64d
from util_cases import psp

nat = psp.native
DIRS, REGIME_CAP, ALPHA0 = kc.DIRS, kc.REGIME_CAP, kc.ALPHA0


def full_rank_B(d, seed):
    return torch.randn(d, d, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) / d ** 0.5


def low_rank_B(d, rank, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(d, rank, generator=g, dtype=torch.float64) @ torch.randn(rank, d, generator=g, dtype=torch.float64) / d ** 0.5


def ones_B(d):
    return (2.0 / d) ** 0.5 * torch.ones(d, d, dtype=torch.float64)


# name -> (B, how the table is made: 'eigh' (the plan's factor) or 'ones' (sqrt(2) 1 given directly), make_case arguments,
#          what it reaches, what psp_pinn_query must answer: n_grad, n_hess, dir_blocks, tiles, bwd_workgroups)
CASES = {
    "rank1": (lambda: ones_B(4), "ones",
              dict(d=4, parabolic=False, arch=[20], K=5, act="relu2", seed=0, h_kind=r64d.H_EXP_SIN_FULL, h_par=(0.5, 4.0, 0.0, 0.0)),
              "n_grad = 0, one direction: one block with 13 idle rows", (0, 1, 1, 5, 5)),
    "rank1_eigh": (lambda: ones_B(4), "eigh",
                   dict(d=4, parabolic=False, arch=[20], K=5, act="relu2", seed=0, h_kind=r64d.H_EXP_SIN_FULL,
                        h_par=(0.5, 4.0, 0.0, 0.0)),
                   "the same points with the eigh factor of sqrt(2/d) ones", (0, 1, 1, 5, 5)),
    "hess14": (lambda: full_rank_B(14, 1), "eigh",
               dict(d=14, parabolic=False, arch=[16], K=9, act="tanh", seed=0, h_kind=r64.H_ALLEN_CAHN),
               "n_grad = 0, a full block of counted directions", (0, 14, 1, 9, 9)),
    "hess15": (lambda: full_rank_B(15, 2), "eigh",
               dict(d=15, parabolic=False, arch=[16], K=9, act="tanh", seed=0, h_kind=r64.H_ALLEN_CAHN),
               "n_grad = 0, one direction alone in block 1", (0, 15, 2, 18, 18)),
    "mixed_block": (lambda: full_rank_B(15, 3), "eigh",
                    dict(d=15, parabolic=False, arch=[16, 16], K=33, act="relu2", seed=0, h_kind=r64.H_ALLEN_CAHN,
                         drift_kind=r64.DRIFT_DIAG),
                    "15 + 15 directions: block 1 holds one gradient and thirteen counted directions", (15, 15, 3, 99, 99)),
    "time_input": (lambda: full_rank_B(13, 4), "eigh",
                   dict(d=13, parabolic=True, arch=[24, 8], K=17, act="tanh2", seed=0, linear=True, h_kind=r64.H_EXP_LIN,
                        h_par=(0.5, 13.0, 0.75, 0.0)),
                   "14 + 13: block 0 has no counted direction; the time column of every u_j is 0", (14, 13, 2, 34, 34)),
    "rank_deficient": (lambda: low_rank_B(9, 3, 5), "eigh",
                       dict(d=9, parabolic=False, arch=[12, 12], K=12, act="relu2", seed=0, h_kind=r64.H_EXP_SQ,
                            h_par=(0.05, 9.0, 0.0, 0.0), drift_kind=r64.DRIFT_DWELL),
                       "B of rank 3: n_hess = 3 behind nine gradient directions", (9, 3, 1, 12, 12)),
    "stride": (lambda: full_rank_B(112, 6), "eigh",
               dict(d=112, parabolic=False, arch=[128, 128, 128, 128], K=20, act="tanh", seed=1, h_kind=r64.H_ALLEN_CAHN,
                    drift_kind=r64.DRIFT_DIAG),
               "112 + 112 directions, 16 blocks: 320 tiles on 256 backward workgroups (grid-stride, LDS reuse)",
               (112, 112, 16, 320, 256)),
}
ONE_HOT_LAST = ("mixed_block",)
# Seeds: the first at which the fp32 STATEMENT stays at or below REGIME_CAP on every compared vector and, for relu^2, no float64
# pre-activation lies within 1e-5 max|z| of the kink (test_pinn_hessian_kernel_cases.py asserts both; no kernel is involved).


def make(name):
    B, how, kw, _, _ = CASES[name]
    B = B()
    dirs = 2.0 ** 0.5 * torch.ones(1, kw["d"], dtype=torch.float64) if how == "ones" else r64d.eigh_factor(B)
    case = r64d.make_case(dirs, **kw)
    case["B"] = B
    return case


def layout(case):
    """(n_grad, n_hess, dir_blocks) as the ABI layer chooses them."""
    n_in = kc.n_in_of(case)
    n_grad = 0 if (case["drift_kind"] == r64.DRIFT_ZERO and not case["parabolic"]) else n_in
    n_hess = case["dirs"].shape[0]
    return n_grad, n_hess, (n_grad + n_hess + DIRS - 1) // DIRS


def rbars(name, K, R64):
    out = {"loss": r64.mean_square_rbar(ALPHA0, K)(R64), "random": kc.random_rbar(K), "variance": r64.variance_rbar(ALPHA0, K)(R64)}
    if name in ONE_HOT_LAST:
        out["one-hot last"] = r64.one_hot(K, K - 1)
    return {k: v.float().double() for k, v in out.items()}


def statement(case, weights, dtype):
    V, gV, second, R = r64d.parts(case, dtype)
    grads = dict(zip(weights, r64d.weighted_grads(case, list(weights.values()), dtype)))
    return dict(V=V.double(), gradV=gV.double(), lap=second.double(), R=R.double(), grads={k: g.double() for k, g in grads.items()})


def scalar_blocks_in_kernel_order(case, weights):
    """pinn_kernel_cases.scalar_blocks_in_kernel_order for this statement and this direction count."""
    f32 = torch.float32
    params = [p.to(f32).clone().requires_grad_(True) for p in case["params"]]
    scal = [i for i, p in enumerate(params) if p.numel() == 1]
    R = r64d.terms(case, params, f32)[3]
    per = torch.zeros(case["K"], len(scal), dtype=f32)
    for k in range(case["K"]):
        gs = torch.autograd.grad(R[k], [params[i] for i in scal], allow_unused=True, retain_graph=True)
        per[k] = torch.stack([torch.zeros((), dtype=f32) if g is None else g.reshape(()) for g in gs])
    offs = [sum(p.numel() for p in params[:i]) for i in scal]
    out = {}
    for key, w in weights.items():
        flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.float64)
        flat[offs] = kc.kernel_order_sum(w.to(f32)[:, None] * per, layout(case)[2]).double()
        out[key] = flat
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(case, rbar, f64, f32): computed once per case, never modified."""
    case = make(name)
    weights = rbars(name, case["K"], r64d.parts(case)[3])
    f32 = statement(case, weights, torch.float32)
    f32["grads_kernel_order"] = scalar_blocks_in_kernel_order(case, weights)
    return dict(name=name, case=case, rbar=weights, f64=statement(case, weights, torch.float64), f32=f32)


def evaluate(ref, got):
    """Every comparison of one case as pinn_kernel_cases rows.  ``got``: R (K), V (K), gradV (K, n_grad), lap_parts (K, nblk),
    grads {key: flat}."""
    case, f64, f32 = ref["case"], ref["f64"], ref["f32"]
    n_grad, n_hess, nblk = layout(case)
    rows = [kc.row("R", got["R"], f64["R"], f32["R"]), kc.row("V", got["V"], f64["V"], f32["V"])]
    assert got["gradV"].shape == (case["K"], n_grad)
    for j in range(n_grad):
        rows.append(kc.row("gradV[:, %d]" % j, got["gradV"][:, j], f64["gradV"][:, j], f32["gradV"][:, j]))
    parts = got["lap_parts"].detach().double().cpu()
    assert parts.shape == (case["K"], nblk)
    rows.append(kc.row("sum_j u_j^T Hess V u_j", parts.sum(1), f64["lap"], f32["lap"]))
    for b in range(nblk):
        if (b + 1) * DIRS <= n_grad:                               # a block of gradient directions only adds nothing, in any order
            ok = bool((parts[:, b] == 0.0).all())
            rows.append(("lap part of block %d (exactly 0)" % b, 0.0 if ok else float("inf"), 0.0, 0.0, ok))
    assert set(got["grads"]) == set(f64["grads"])
    for key, g64 in f64["grads"].items():
        g, g32 = r64.blocks(case, got["grads"][key]), r64.blocks(case, f32["grads"][key])
        other = r64.blocks(case, f32["grads_kernel_order"][key])
        for blk, v64 in r64.blocks(case, g64).items():
            rows.append(kc.row("grad[%s] %s" % (key, blk), g[blk], v64, g32[blk], other[blk]))
    return rows


def regime_rows(ref):
    """The fp32 statement against float64 on every vector the device test compares: (label, e_fp32)."""
    case, f64, f32 = ref["case"], ref["f64"], ref["f32"]
    out = [(k, kc.err(f32[k], f64[k])) for k in ("R", "V", "lap")]
    for j in range(layout(case)[0]):
        out.append(("gradV[:, %d]" % j, kc.err(f32["gradV"][:, j], f64["gradV"][:, j])))
    for key, g64 in f64["grads"].items():
        g32 = r64.blocks(case, f32["grads"][key])
        for blk, v64 in r64.blocks(case, g64).items():
            if float(v64.abs().max()) > 0.0:
                out.append(("grad[%s] %s" % (key, blk), kc.err(g32[blk], v64)))
    return out


# ---- the device wrapper ----------------------------------------------------------------------------------------------------
def pinn_config(case, K=None, dirs_ptr=None, n_dirs=None):
    """psp_pinn_config of a dense case; psp_pinn_query tests the table's pointer for NULL only, so a CPU test passes any other."""
    c = kc.pinn_config(case, K)
    c.sigma_kind, c.sigma_scale = nat.GENL_SIGMA_DENSE, 0.0
    c.n_dirs = case["dirs"].shape[0] if n_dirs is None else n_dirs
    c.dirs = dirs_ptr
    return c


def query(c):
    sz = nat.PinnSizes()
    return nat.load().psp_pinn_query(C.byref(c), C.byref(sz)), sz


class Native:
    """One dense case on the device through the C ABI.  R, the scratch, the partials and the gradient are filled with NaN before
    each call, so an entry no tile writes cannot pass for a result."""

    def __init__(self, case):
        self.lib, d = nat.load(), torch.device("cuda:0")
        f32 = torch.float32
        self.case, self.K = case, case["K"]
        self.drift = None if case["drift"] is None else case["drift"].to(d, f32).contiguous()
        self.dirs = case["dirs"].to(d, f32).contiguous()
        c = pinn_config(case, dirs_ptr=nat.ptr(self.dirs))
        c.drift = nat.ptr(self.drift)
        self.cfg, self.sz = c, nat.PinnSizes()
        nat.check(self.lib.psp_pinn_query(C.byref(c), C.byref(self.sz)), "psp_pinn_query")
        self.params = torch.cat([p.reshape(-1) for p in case["params"]]).to(d, f32).contiguous()
        assert self.params.numel() == self.sz.n_params
        self.x = case["x"].to(d, f32).contiguous()
        self.t = case["t"].to(d, f32).contiguous() if case["parabolic"] else None
        pad = 64                                                   # floats behind every buffer that must keep their NaN
        self.scratch = torch.empty(self.sz.scratch_bytes // 4 + pad, dtype=f32, device=d)
        self.partial = torch.empty(self.sz.grad_partial_bytes // 4 + pad, dtype=f32, device=d)
        self.R_buf = torch.empty(self.K + pad, dtype=f32, device=d)
        self.grad_buf = torch.empty(self.sz.n_params + pad, dtype=f32, device=d)
        self.R, self.grad = self.R_buf[:self.K], self.grad_buf[:self.sz.n_params]

    def residual(self):
        for buf in (self.R_buf, self.scratch, self.partial, self.grad_buf):
            buf.fill_(float("nan"))
        nat.check(self.lib.psp_pinn_residual(C.byref(self.cfg), nat.ptr(self.params), nat.ptr(self.x), nat.ptr(self.t),
                                             nat.ptr(self.scratch), nat.ptr(self.R_buf), None), "psp_pinn_residual")
        torch.cuda.synchronize()
        return self.R

    def backward(self, rbar):
        rbar = rbar.to(self.params.device, torch.float32).contiguous()
        assert rbar.numel() == self.K
        for buf in (self.partial, self.grad_buf):
            buf.fill_(float("nan"))
        nat.check(self.lib.psp_pinn_backward(C.byref(self.cfg), nat.ptr(self.params), nat.ptr(self.x), nat.ptr(self.t),
                                             nat.ptr(self.scratch), nat.ptr(rbar), nat.ptr(self.partial), nat.ptr(self.grad_buf),
                                             None), "psp_pinn_backward")
        torch.cuda.synchronize()
        return self.grad

    def scratch_parts(self):
        """The documented dense layout (include/psp.h): V (K), lap (K, nblk), gradV (K, n_grad), cV (K), cG (K, n_grad)."""
        return kc.scratch_parts(self.scratch, self.K, self.sz.dir_blocks, layout(self.case)[0])

    def check_padding(self):
        used = self.sz.scratch_bytes // 4
        assert used == self.K * (2 + self.sz.dir_blocks + 2 * layout(self.case)[0])
        kc.check_padding("scratch", self.scratch[used:])
        kc.check_padding("partial", self.partial[self.sz.bwd_workgroups * self.sz.n_params:])
        kc.check_padding("R", self.R_buf[self.K:])
        kc.check_padding("grad", self.grad_buf[self.sz.n_params:])
