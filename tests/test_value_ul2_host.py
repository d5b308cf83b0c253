"""Host side of the u_L2 log of Solver(approx_method='value_function'), checked without a GPU: the ctypes layout of psp_genl_ul2
against include/psp.h, the checks psp_genl_query_ul2 makes without a launch, the growth of table_bytes by the staged gains, and
value_eligibility's reasons with the flag on and off."""
import ctypes as C
import os
import re

import torch

from util_cases import ROOT, psp

nat = psp.native
pvn = psp.plan_value_native
HEADER = os.path.join(ROOT, "include", "psp.h")


def test_struct_layout_and_symbols_match_the_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct psp_genl_ul2 \{(.*?)\} psp_genl_ul2;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip(" *") for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    assert names == [f[0] for f in nat.GenlUl2._fields_] == [
        "struct_bytes", "kind", "u_l2_out", "u_ref", "tables", "group", "row", "ntables", "nrows", "ncols", "xb", "dx", "xhi",
        "K_global"]
    offs = dict(struct_bytes=0, kind=4, u_l2_out=8, u_ref=16, tables=24, group=32, row=40, ntables=48, nrows=52, ncols=56, xb=60,
                dx=64, xhi=68, K_global=72)
    for name, off in offs.items():
        assert getattr(nat.GenlUl2, name).offset == off, name
    assert C.sizeof(nat.GenlUl2) == 80
    # the structs it travels beside kept their sizes
    assert C.sizeof(nat.GenlCoeffs) == 32 and C.sizeof(nat.GenlConfig) == 192 and C.sizeof(nat.GenConfig) == 136
    for sym in ("psp_genl_query_ul2", "psp_genl_ul2_stage", "psp_genl_rollout_fwd_ul2"):
        assert re.search(r"\bint %s\(" % sym, text), sym
        assert sym in nat.SIGNATURES and hasattr(nat.load(), sym), sym
    assert (nat.UL2_TABLE, nat.UL2_LINEAR, nat.UL2_GRID) == (0, 1, 2)


def _config(d=20):
    c = nat.GenlConfig()
    c.base.d, c.base.K_local, c.base.N, c.base.h_kind = d, 200, 20, nat.GH_QUAD
    c.base.T, c.base.domain_kind = float("inf"), nat.DOM_NONE
    c.has_time, c.n_hidden, c.widths[0], c.widths[1] = 1, 2, 30, 30
    return c


_BUF = (C.c_float * 16)()
PTR = C.addressof(_BUF)                                               # (a query reads no pointer)


def _lq():
    return nat.GenlCoeffs(struct_bytes=C.sizeof(nat.GenlCoeffs), z_kind=nat.GENL_Z_SIGMA)


def _ul2(shape, **kw):
    """A valid struct of kind ``shape``, then the overrides."""
    kind = shape
    u = nat.GenlUl2(struct_bytes=C.sizeof(nat.GenlUl2), kind=kind, u_l2_out=PTR, K_global=200)
    if kind == nat.UL2_TABLE:
        u.u_ref = PTR
    else:
        u.tables = PTR
    if kind == nat.UL2_GRID:
        u.group, u.row, u.ntables, u.nrows, u.ncols, u.xb, u.dx, u.xhi = PTR, PTR, 2, 31, 99, 2.5, 0.05, 2.4
    for k, v in kw.items():
        setattr(u, k, v)
    return u


def _query(c, q, u):
    lib, sz = nat.load(), nat.GenlSizes()
    rc = lib.psp_genl_query_ul2(C.byref(c), C.byref(q) if q is not None else None, C.byref(u) if u is not None else None,
                                C.byref(sz))
    return rc, sz, (nat.last_error() if rc else "")


def test_query_rejections():
    c = _config()
    for kind in (nat.UL2_TABLE, nat.UL2_LINEAR, nat.UL2_GRID):
        assert _query(c, _lq(), _ul2(kind))[0] == 0
    assert _query(c, None, _ul2(nat.UL2_TABLE))[0] == 0 and _query(c, None, _ul2(nat.UL2_GRID))[0] == 0
    # struct_bytes
    for n in (0, C.sizeof(nat.GenlUl2) - 8, C.sizeof(nat.GenlUl2) + 8):
        rc, _, msg = _query(c, _lq(), _ul2(nat.UL2_TABLE, struct_bytes=n))
        assert rc != 0 and "psp_genl_ul2.struct_bytes" in msg, (n, msg)
    # kind
    for kind in (-1, 3):
        rc, _, msg = _query(c, _lq(), _ul2(nat.UL2_TABLE, kind=kind))
        assert rc != 0 and "kind out of range" in msg
    # pointers of the kind
    rc, _, msg = _query(c, _lq(), _ul2(nat.UL2_TABLE, u_l2_out=None))
    assert rc != 0 and "needs psp_genl_ul2.u_l2_out" in msg
    rc, _, msg = _query(c, _lq(), _ul2(nat.UL2_TABLE, u_ref=None))
    assert rc != 0 and "PSP_UL2_TABLE needs psp_genl_ul2.u_ref" in msg
    for kind in (nat.UL2_LINEAR, nat.UL2_GRID):
        rc, _, msg = _query(c, _lq(), _ul2(kind, tables=None))
        assert rc != 0 and "need psp_genl_ul2.tables" in msg
    rc, _, msg = _query(c, _lq(), _ul2(nat.UL2_GRID, group=None))
    assert rc != 0 and "needs psp_genl_ul2.group" in msg
    rc, _, msg = _query(c, _lq(), _ul2(nat.UL2_GRID, row=None))
    assert rc != 0 and "needs psp_genl_ul2.row" in msg
    rc, _, msg = _query(c, _lq(), _ul2(nat.UL2_GRID, ncols=0))
    assert rc != 0 and "must be positive" in msg
    rc, _, msg = _query(c, _lq(), _ul2(nat.UL2_GRID, dx=0.0))
    assert rc != 0 and "xb / dx must be positive" in msg
    # a run that can stop: a domain, a finite T
    c.base.domain_kind, c.base.dom_a = nat.DOM_SPHERE, 1.0
    rc, _, msg = _query(c, _lq(), _ul2(nat.UL2_TABLE))
    assert rc != 0 and "never stop" in msg
    assert _query(c, _lq(), None)[0] == 0                               # (the config itself is fine)
    c.base.domain_kind = nat.DOM_NONE
    c.base.T = 0.5
    rc, _, msg = _query(c, _lq(), _ul2(nat.UL2_GRID))
    assert rc != 0 and "never stop" in msg and "T = inf" in msg
    c.base.T = float("inf")
    # the instance shapes that carry the log
    rc, _, msg = _query(c, None, _ul2(nat.UL2_LINEAR))
    assert rc != 0 and "PSP_UL2_LINEAR runs on the linear-quadratic instances" in msg
    c.sigma_kind, c.sigma = nat.GENL_SIGMA_DENSE, PTR
    rc, _, msg = _query(c, None, _ul2(nat.UL2_TABLE))
    assert rc != 0 and "linear-quadratic instances" in msg


def test_table_bytes_grow_by_the_staged_gains_only():
    for d, db in ((20, 2), (5, 1), (17, 2), (47, 3), (48, 4)):
        c = _config(d)
        for q in (_lq(), None):
            rc, base, _ = _query(c, q, None)
            assert rc == 0
            lib, lq_sz = nat.load(), nat.GenlSizes()
            assert lib.psp_genl_query_lq(C.byref(c), C.byref(q) if q is not None else None, C.byref(lq_sz)) == 0
            assert lq_sz.table_bytes == base.table_bytes               # a NULL struct: the existing entry point
            kinds = (nat.UL2_TABLE, nat.UL2_GRID) + ((nat.UL2_LINEAR,) if q is not None else ())
            for kind in kinds:
                rc, sz, msg = _query(c, q, _ul2(kind))
                assert rc == 0, msg
                grow = int(sz.table_bytes) - int(base.table_bytes)
                if kind == nat.UL2_LINEAR:
                    gains = c.base.N * db * db * 256 * 4               # N operand tables of DB0 x DB0 blocks of 256 floats
                    assert grow == gains, (d, grow, gains)
                else:
                    assert grow == 0, (d, kind, grow)
                for f in ("path_bytes", "ahat_bytes", "n_params", "grad_partial_bytes", "n_blocks", "waves_per_tile"):
                    assert getattr(sz, f) == getattr(base, f), f


def test_lds_rule_counts_the_kept_z_image():
    """4 x 128 hidden units on 112 inputs fill the LDS with the activation images alone (2 TB KiB); a net with few hidden blocks
    and a wide input is where the carve TB + 5 DB0 decides -- both fit, and the shape limits hold."""
    c = _config(111)
    c.n_hidden = 4
    for i in range(4):
        c.widths[i] = 128
    assert _query(c, _lq(), _ul2(nat.UL2_LINEAR))[0] == 0
    c.n_hidden, c.widths[0] = 1, 16
    assert _query(c, _lq(), _ul2(nat.UL2_GRID))[0] == 0
    c.base.d = 112
    rc, _, msg = _query(c, _lq(), _ul2(nat.UL2_TABLE))
    assert rc != 0 and "112" in msg


class _Solver:
    """The attributes value_eligibility reads."""

    def __init__(self, problem, V, flag, dt=0.01):
        self.device = torch.device("cuda")                           # (only its type is read; nothing is run on it)
        self.approx_method, self.time_approx, self.loss_method = "value_function", "inner", "log-variance"
        self.adaptive_forward_process, self.detach_forward, self.learn_Y_0 = True, True, False
        self.u_l2_error_flag, self.burgers_drift, self.compute_gradient_variance, self.log_gradient = flag, False, 0, False
        self.metastability_logs, self.IS_variance_K = None, 0
        self.y_n, self.d, self.problem = [V], problem.d, problem
        self.delta_t_np = dt
        self.N = int(round(problem.T / dt))


def _net(d, arch=(30, 30)):
    return psp.DenseNet(d_in=d + 1, d_out=1, lr=1e-3, arch=list(arch), seed=1)


def test_eligibility_reasons():
    # a problem with no description the kernel reads: a double well before compute_reference_solution
    dw = psp.DoubleWell(d=1, T=0.1, eta=3.0, kappa=5.0, device="cpu")
    r = pvn.value_eligibility(_Solver(dw, _net(1), True))
    assert r == psp.plan_dense_native.ul2_unsupported(dw, 10, 0.01) and "u_true_tables" in r and "u_l2_error_flag" in r
    # the other diagnostics are refused as before, flag on or off
    for flag in (True, False):
        s = _Solver(psp.LLGC(d=6, off_diag=0.1, T=0.4, device="cpu"), _net(6), flag)
        s.log_gradient = True
        r = pvn.value_eligibility(s)
        assert r is not None and "gradient logs" in r and "u_L2" not in r
    if not nat.is_built():
        return
    dw.compute_reference_solution(nx=200)
    assert pvn.value_eligibility(_Solver(dw, _net(1), True)) is None
    # the grid tables end before the solver's time grid does: ul2_unsupported's reason
    r = pvn.value_eligibility(_late(dw))
    assert r is not None and "end at t" in r
    # LLGC (table) and LQGC (gains) with the flag on
    off = psp.LLGC(d=6, off_diag=0.1, T=0.4, device="cpu")
    assert pvn.value_eligibility(_Solver(off, _net(6), True)) is None
    assert pvn.value_eligibility(_Solver(psp.LQGC(d=6, off_diag=0.1, T=0.3, delta_t=0.005, device="cpu"), _net(6), True)) is None
    diag = psp.LLGC(d=8, off_diag=0.0, T=0.4, device="cpu")
    assert pvn.value_eligibility(_Solver(diag, _net(8), True)) is None
    # an input wider than 112: only the templated kernels would take the net, and they have no log
    d = 112
    wide = psp.LLGC(d=d, off_diag=0.0, T=0.1, device="cpu")
    assert not pvn.needs_lq(wide.native_spec())
    on, offr = pvn.value_eligibility(_Solver(wide, _net(d), True)), pvn.value_eligibility(_Solver(wide, _net(d), False))
    assert on is not None and "u_L2 log" in on and "input <= 112" in on and "u_l2_error_flag=False" in on
    # ... and with the flag off the answer is what the templated family's instance list says, as before
    cands = psp.native_shapes.gen_candidates(d, 30)
    assert (offr is None) == bool(cands)
    if offr is not None:
        assert "no compiled kernel instance covers d=112, H=30" in offr
    # unchanged reasons with the flag off
    r = pvn.value_eligibility(_Solver(psp.LLGC(d=112, off_diag=0.01, T=0.4, device="cpu"), _net(112), False))
    assert r is not None and "dense sigma / dense drift / running cost" in r and "input <= 112" in r
    s = _Solver(off, _net(6), False)
    s.adaptive_forward_process, s.detach_forward = True, False
    assert "state path" in pvn.value_eligibility(s)
    assert pvn.value_eligibility(_Solver(off, _net(6), False)) is None


def _late(dw):
    s = _Solver(dw, _net(1), True)
    s.N = 40                                                         # the tables hold rows up to t = 0.1
    return s
