"""Host logic of the attached value-function ansatz (adaptive_forward_process=True, detach_forward=False) checked without a GPU:
the Solver keyword value_state_path, value_eligibility on stub solvers, the ctypes layout of psp_genl_adj against include/psp.h
and the checks psp_genl_query_adj / psp_genl_adjoint_sweep make without a launch."""
import ctypes as C
import os
import re

import pytest
import torch

from util_cases import ROOT, psp

nat = psp.native
pvn = psp.plan_value_native


class _Solver:
    """The attributes value_eligibility reads."""

    def __init__(self, problem, V, state_path=None, loss="log-variance"):
        self.device = torch.device("cuda")                           # (only its type is read; nothing is run on it)
        self.approx_method, self.time_approx, self.loss_method = "value_function", "inner", loss
        self.adaptive_forward_process, self.detach_forward, self.learn_Y_0 = True, False, False
        self.u_l2_error_flag, self.burgers_drift, self.compute_gradient_variance, self.log_gradient = False, False, 0, False
        self.metastability_logs, self.IS_variance_K = None, 0
        self.y_n, self.d, self.problem = [V], problem.d, problem
        self.N, self.delta_t_np = 6, 0.05
        if state_path is not None:
            self.value_state_path = state_path


def _net(d, arch=(30, 30)):
    return psp.DenseNet(d_in=d + 1, d_out=1, lr=1e-3, arch=list(arch), seed=1)


def _problems():
    return [psp.LLGC(d=6, off_diag=0.1, T=0.4, device="cpu"), psp.LQGC(d=6, off_diag=0.1, T=0.3, delta_t=0.05, device="cpu"),
            psp.DoubleWell_multidim(d=6, d_1=3, d_2=3, T=0.3, eta=0.5, kappa=2.0, device="cpu")]


def test_default_keyword_keeps_the_composite_plan():
    for pb in _problems():
        for sp in (None, "torch"):
            r = pvn.value_eligibility(_Solver(pb, _net(pb.d), state_path=sp))
            assert r is not None and "state path" in r and "value_state_path" in r


def test_solver_keyword():
    pb = psp.LQGC(d=3, off_diag=0.1, T=0.5, delta_t=0.05, device="cpu")
    kw = dict(approx_method="value_function", time_approx="inner", verbose=False, device="cpu")
    assert psp.Solver("s", pb, **kw).value_state_path == "torch"
    a, b = psp.Solver("s", pb, **kw), psp.Solver("s", pb, value_state_path="native", **kw)
    assert b.value_state_path == "native"
    b.y_n, b.problem, b.y_0 = a.y_n, a.problem, getattr(a, "y_0", None)
    assert a._plan_key() != b._plan_key()                            # a plan built for one is not reused for the other
    with pytest.raises(ValueError):
        psp.Solver("s", pb, value_state_path="hip", **kw)


@pytest.mark.skipif(not nat.is_built(), reason="libpsp_hip.so is not built")
def test_native_keyword_is_eligible_on_the_three_problem_families():
    for pb in _problems() + [psp.LLGC(d=6, off_diag=0.0, T=0.4, device="cpu")]:
        assert pvn.value_eligibility(_Solver(pb, _net(pb.d), state_path="native")) is None, type(pb).__name__
    off = _problems()[0]
    assert pvn.value_eligibility(_Solver(off, _net(6, (20, 16, 12)), state_path="native")) is None
    assert pvn.value_eligibility(_Solver(off, _net(6), state_path="native", loss="moment")) is None


def test_native_keyword_still_refuses_what_the_detached_plan_refuses():
    off = _problems()[0]
    r = pvn.value_eligibility(_Solver(off, _net(6), state_path="native", loss="cross_entropy"))
    assert r is not None and "cross_entropy" in r
    dense_p = psp.LQGC(d=3, off_diag=0.1, T=0.5, delta_t=0.05, device="cpu")
    dense_p.P = dense_p.P + 0.1 * torch.ones(3, 3)
    r = pvn.value_eligibility(_Solver(dense_p, _net(3), state_path="native"))
    assert r is not None and "native_spec" in r
    if not nat.is_built():
        return
    wide = psp.LLGC(d=112, off_diag=0.01, T=0.4, device="cpu")
    r = pvn.value_eligibility(_Solver(wide, _net(112), state_path="native"))
    assert r is not None and "input <= 112" in r
    # a net the templated kernels would take, on a problem without coefficients: still the run-time-shaped family
    plain = psp.DoubleWell_multidim(d=114, d_1=57, d_2=57, T=0.3, device="cpu")
    r = pvn.value_eligibility(_Solver(plain, _net(114), state_path="native"))
    assert r is not None and "adjoint sweep" in r and "input <= 112" in r


def test_adj_layout_matches_the_header():
    offs = [("struct_bytes", 0), ("reserved", 4), ("mu", 8), ("resid_coeff", 16), ("lam_N", 24), ("lam0_out", 32),
            ("drift_t_offset", 40)]
    assert [f[0] for f in nat.GenlAdj._fields_] == [n for n, _ in offs]
    for name, off in offs:
        assert getattr(nat.GenlAdj, name).offset == off, name
    assert C.sizeof(nat.GenlAdj) == 48
    assert C.sizeof(nat.GenlConfig) == 192 and C.sizeof(nat.GenlCoeffs) == 32 and C.sizeof(nat.GenlSizes) == 80   # nothing else grew
    with open(os.path.join(ROOT, "include", "psp.h")) as fh:
        hdr = fh.read()
    body = re.search(r"typedef struct psp_genl_adj \{(.*?)\} psp_genl_adj;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r".*[\s*]", "", decl.strip()) for decl in body.split(";") if decl.strip()]
    assert names == [n for n, _ in offs]
    for sym in ("psp_genl_query_adj", "psp_genl_adjoint_sweep"):
        assert sym in nat.SIGNATURES and re.search(r"\bint %s\(" % sym, hdr)


def _config(d=20, K=200, N=20):
    c = nat.GenlConfig()
    c.base.d, c.base.K_local, c.base.N, c.base.h_kind = d, K, N, nat.GH_QUAD
    c.base.T, c.base.domain_kind = float("inf"), nat.DOM_NONE
    c.base.adaptive, c.base.per_sample_weights, c.base.store_path = 1, 1, 1
    c.has_time, c.n_hidden, c.widths[0], c.widths[1] = 1, 2, 30, 30
    return c


def _adj():
    return nat.GenlAdj(struct_bytes=C.sizeof(nat.GenlAdj))


needs_lib = pytest.mark.skipif(not nat.is_built(), reason="libpsp_hip.so is not built")


@needs_lib
def test_query_adj_returns_sizes_and_the_table_of_the_transposed_drift():
    lib = nat.load()
    assert lib.psp_version() == 400
    c, sz, base = _config(), nat.GenlSizes(), nat.GenlSizes()
    A = torch.zeros(20, 20)
    q = nat.GenlCoeffs(struct_bytes=C.sizeof(nat.GenlCoeffs), z_kind=nat.GENL_Z_SIGMA, drift_matrix=A.data_ptr())
    assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(base)) == 0
    adj = _adj()
    assert lib.psp_genl_query_adj(C.byref(c), C.byref(q), None, C.byref(adj), C.byref(sz)) == 0, nat.last_error()
    block = 2 * 2 * 256 * 4                                          # d + 1 = 21: DB0 x DB0 = 2 x 2 blocks of 256 floats
    assert base.table_bytes + block <= sz.table_bytes <= base.table_bytes + block + 12
    assert adj.drift_t_offset * 4 >= base.table_bytes and adj.drift_t_offset % 4 == 0
    assert adj.drift_t_offset * 4 + block == sz.table_bytes
    for f in ("path_bytes", "ahat_bytes", "n_params", "grad_partial_bytes", "n_blocks", "waves_per_tile"):
        assert getattr(sz, f) == getattr(base, f), f
    # without a drift matrix (sigma = s I, element-wise drift; no coefficients at all): no table
    plain = nat.GenlSizes()
    assert lib.psp_genl_query(C.byref(c), C.byref(plain)) == 0
    assert lib.psp_genl_query_adj(C.byref(c), None, None, C.byref(_adj()), C.byref(sz)) == 0, nat.last_error()
    assert sz.table_bytes in range(plain.table_bytes, plain.table_bytes + 13)
    # with the log: the table goes behind the staged gains, which stay where psp_genl_rollout_fwd_ul2 reads them
    probe = C.addressof(pvn._PROBE)
    u = nat.GenlUl2(struct_bytes=C.sizeof(nat.GenlUl2), kind=nat.UL2_LINEAR, u_l2_out=probe, tables=probe, K_global=200)
    withlog = nat.GenlSizes()
    assert lib.psp_genl_query_ul2(C.byref(c), C.byref(q), C.byref(u), C.byref(withlog)) == 0
    assert lib.psp_genl_query_adj(C.byref(c), C.byref(q), C.byref(u), C.byref(adj), C.byref(sz)) == 0
    assert adj.drift_t_offset * 4 >= withlog.table_bytes and sz.table_bytes == adj.drift_t_offset * 4 + block
    # the LDS rule counts the sweep's images: 4 x 128 units on 112 inputs fit the forward, not four images of the concatenation
    c.base.d, c.n_hidden = 111, 4
    for i in range(4):
        c.widths[i] = 128
    assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(sz)) == 0
    assert lib.psp_genl_query_adj(C.byref(c), C.byref(q), None, C.byref(adj), C.byref(sz)) != 0 and "LDS" in nat.last_error()
    c.widths[2], c.widths[3] = 64, 64                                # 7 + 24 blocks: (4 * 31 + 3 * 7) KiB = 145 KiB
    assert lib.psp_genl_query_adj(C.byref(c), C.byref(q), None, C.byref(adj), C.byref(sz)) == 0, nat.last_error()


@needs_lib
def test_query_adj_refuses_with_a_message():
    lib = nat.load()
    sz = nat.GenlSizes()
    q = nat.GenlCoeffs(struct_bytes=C.sizeof(nat.GenlCoeffs), z_kind=nat.GENL_Z_SIGMA)

    def refused(c, coeffs, adj, word):
        rc = lib.psp_genl_query_adj(C.byref(c), C.byref(coeffs) if coeffs is not None else None, None,
                                    C.byref(adj) if adj is not None else None, C.byref(sz))
        return rc != 0 and word in nat.last_error()

    assert lib.psp_genl_query_adj(C.byref(_config()), C.byref(q), None, C.byref(_adj()), C.byref(sz)) == 0
    c = _config()
    c.base.T = 1.0
    assert refused(c, q, _adj(), "T = inf")
    c = _config()
    c.base.domain_kind, c.base.dom_a = nat.DOM_SPHERE, 1.0
    assert refused(c, q, _adj(), "never stop")
    c = _config()
    c.base.adaptive = 0
    assert refused(c, q, _adj(), "adaptive")
    c = _config()
    c.base.h_kind = nat.GH_ZERO
    assert refused(c, q, _adj(), "PSP_GH_QUAD")
    assert refused(_config(), q, nat.GenlAdj(struct_bytes=C.sizeof(nat.GenlAdj) - 8), "struct_bytes")
    assert refused(_config(), q, nat.GenlAdj(), "struct_bytes")
    assert refused(_config(), q, None, "null")
    # the other orientation: a dense sigma without coefficients, and coefficients that ask for Z = B^T grad V
    B = torch.eye(20)
    c = _config()
    c.sigma_kind, c.sigma = nat.GENL_SIGMA_DENSE, B.data_ptr()
    assert refused(c, None, _adj(), "PSP_GENL_Z_SIGMA_T")
    qt = nat.GenlCoeffs(struct_bytes=C.sizeof(nat.GenlCoeffs), z_kind=nat.GENL_Z_SIGMA_T, drift_matrix=B.data_ptr())
    assert refused(_config(), qt, _adj(), "PSP_GENL_Z_SIGMA_T")


@needs_lib
def test_sweep_rejects_null_buffers_before_any_launch():
    lib = nat.load()
    c = _config()
    q = nat.GenlCoeffs(struct_bytes=C.sizeof(nat.GenlCoeffs), z_kind=nat.GENL_Z_SIGMA)
    adj = _adj()
    rc = lib.psp_genl_adjoint_sweep(C.byref(c), C.byref(q), C.byref(adj), None, None, None, None, None, None)
    assert rc != 0 and "null" in nat.last_error()
    rc = lib.psp_genl_adjoint_sweep(C.byref(c), C.byref(q), None, None, None, None, None, None, None)
    assert rc != 0 and "null" in nat.last_error()
    rc = lib.psp_genl_adjoint_sweep(None, None, C.byref(adj), None, None, None, None, None, None)
    assert rc != 0 and "null" in nat.last_error()
