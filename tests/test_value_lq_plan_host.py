"""Host logic of the linear-quadratic route of Solver(approx_method='value_function'), checked without a GPU: the ctypes layout of
psp_genl_coeffs, the translation of a problem's native_spec() into psp_genl_config + psp_genl_coeffs
(plan_value_native.lq_coeffs), value_eligibility on stub solvers, and the checks psp_genl_query_lq makes without a launch."""
import ctypes as C

import pytest
import torch

from util_cases import psp

nat = psp.native
pvn = psp.plan_value_native


def test_coeffs_layout_and_the_config_it_travels_beside():
    offs = [("struct_bytes", 0), ("z_kind", 4), ("runcost_kind", 8), ("reserved", 12), ("drift_matrix", 16), ("runcost", 24)]
    assert [f[0] for f in nat.GenlCoeffs._fields_] == [n for n, _ in offs]
    for name, off in offs:
        assert getattr(nat.GenlCoeffs, name).offset == off, name
    assert C.sizeof(nat.GenlCoeffs) == 32
    assert C.sizeof(nat.GenlConfig) == 192 and C.sizeof(nat.GenConfig) == 136      # neither config grew
    assert (nat.GENL_Z_SIGMA_T, nat.GENL_Z_SIGMA) == (0, 1)
    z = nat.GenlCoeffs()                                             # zero-initialised: nothing asked
    assert z.struct_bytes == 0 and z.z_kind == 0 and z.runcost_kind == 0 and not z.drift_matrix and not z.runcost


def _floats(ptr, n):
    return list((C.c_float * n).from_address(ptr))


def test_lq_coeffs_uploads_row_major_A_and_B():
    d = 5
    pb = psp.LLGC(d=d, off_diag=0.3, T=0.4, seed=42, device="cpu")
    assert not torch.equal(pb.A, pb.A.t()) and not torch.equal(pb.B, pb.B.t())
    spec = pb.native_spec()
    assert spec["drift"][0] == nat.DRIFT_DENSE and spec["sigma"][0] == nat.SIGMA_DENSE and pvn.needs_lq(spec)
    gcfg = nat.GenlConfig()
    gcfg.base.d = d
    gcfg.base.drift_kind, gcfg.base.drift = nat.DRIFT_DIAG, 12345    # stale values are overwritten
    keep = []
    q = pvn.lq_coeffs(gcfg, spec, torch.device("cpu"), keep)
    assert q is not None and q.struct_bytes == C.sizeof(nat.GenlCoeffs) == 32
    assert q.z_kind == nat.GENL_Z_SIGMA == 1 and q.runcost_kind == nat.RUNCOST_ZERO and not q.runcost
    assert gcfg.sigma_kind == nat.GENL_SIGMA_DENSE and gcfg.base.drift_kind == nat.DRIFT_ZERO and not gcfg.base.drift
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in keep)
    assert {gcfg.sigma, q.drift_matrix} == {t.data_ptr() for t in keep}
    assert _floats(q.drift_matrix, d * d) == [float(v) for v in pb.A.reshape(-1)]      # row-major A, not its transpose
    assert _floats(q.drift_matrix, d * d) != [float(v) for v in pb.A.t().reshape(-1)]
    assert _floats(gcfg.sigma, d * d) == [float(v) for v in pb.B.reshape(-1)]
    # a transposed VIEW (and another dtype) is uploaded by value, not by stride
    spec_t = dict(spec, drift=(nat.DRIFT_DENSE, pb.A.double().t()))
    keep2 = []
    q2 = pvn.lq_coeffs(gcfg, spec_t, torch.device("cpu"), keep2)
    assert _floats(q2.drift_matrix, d * d) == [float(v) for v in pb.A.t().contiguous().reshape(-1)]
    with pytest.raises(ValueError):
        pvn.lq_coeffs(gcfg, dict(spec, drift=(nat.DRIFT_DENSE, torch.zeros(d, d + 1))), torch.device("cpu"), [])


def test_lq_coeffs_running_cost_and_the_plain_catalogue():
    d = 4
    pb = psp.LQGC(d=d, off_diag=0.0, T=0.3, delta_t=0.05, device="cpu")
    spec = pb.native_spec()
    assert spec["drift"][0] == nat.DRIFT_DIAG and spec["sigma"][0] == nat.SIGMA_IDENTITY and pvn.needs_lq(spec)
    gcfg = nat.GenlConfig()
    gcfg.base.d = d
    gcfg.sigma_kind, gcfg.sigma = 1, 12345
    keep = []
    q = pvn.lq_coeffs(gcfg, spec, torch.device("cpu"), keep)
    assert q.runcost_kind == nat.RUNCOST_DIAG_QUAD and _floats(q.runcost, d) == [0.5] * d and not q.drift_matrix
    assert gcfg.sigma_kind == nat.GENL_SIGMA_SCALED and not gcfg.sigma and gcfg.base.sigma_scale == 1.0
    assert gcfg.base.drift_kind == nat.DRIFT_DIAG and _floats(gcfg.base.drift, d) == [-1.0] * d
    # identity sigma, element-wise drift, f = 0: no struct at all -- the plain entry points' behaviour
    plain = psp.LLGC(d=d, off_diag=0.0, T=0.3, device="cpu").native_spec()
    assert not pvn.needs_lq(plain)
    assert pvn.lq_coeffs(gcfg, plain, torch.device("cpu"), []) is None and gcfg.base.drift_kind == nat.DRIFT_DIAG


class _Solver:
    """The attributes value_eligibility reads."""

    def __init__(self, problem, V, adaptive=True, detach=True):
        self.device = torch.device("cuda")                           # (only its type is read; nothing is run on it)
        self.approx_method, self.time_approx, self.loss_method = "value_function", "inner", "log-variance"
        self.adaptive_forward_process, self.detach_forward, self.learn_Y_0 = adaptive, detach, False
        self.u_l2_error_flag, self.burgers_drift, self.compute_gradient_variance, self.log_gradient = False, False, 0, False
        self.metastability_logs, self.IS_variance_K = None, 0
        self.y_n, self.d, self.problem = [V], problem.d, problem


def _net(d, arch=(30, 30)):
    return psp.DenseNet(d_in=d + 1, d_out=1, lr=1e-3, arch=list(arch), seed=1)


def test_eligibility_of_the_linear_quadratic_cases():
    d = 6
    off = psp.LLGC(d=d, off_diag=0.1, T=0.4, device="cpu")
    # the state-path check comes first, whatever the coefficients
    r = pvn.value_eligibility(_Solver(off, _net(d), adaptive=True, detach=False))
    assert r is not None and "state path" in r
    r = pvn.value_eligibility(_Solver(psp.LQGC(d=3, off_diag=0.1, T=0.5, delta_t=0.05, device="cpu"), _net(3), detach=False))
    assert r is not None and "state path" in r
    # a dense P: native_spec() is None, the composite plan with the reason it always had
    dense_p = psp.LQGC(d=3, off_diag=0.1, T=0.5, delta_t=0.05, device="cpu")
    dense_p.P = dense_p.P + 0.1 * torch.ones(3, 3)
    r = pvn.value_eligibility(_Solver(dense_p, _net(3)))
    assert r is not None and "native_spec" in r
    if not nat.is_built():
        return
    # off-diagonal LLGC and LQGC, detached (or non-adaptive): native, also with a net the templated kernels would take
    assert pvn.value_eligibility(_Solver(off, _net(d))) is None
    assert pvn.value_eligibility(_Solver(off, _net(d), adaptive=False, detach=False)) is None
    assert pvn.value_eligibility(_Solver(psp.LQGC(d=d, off_diag=0.0, T=0.3, delta_t=0.05, device="cpu"), _net(d))) is None
    assert pvn.value_eligibility(_Solver(off, _net(d, (20, 16, 12)))) is None
    # outside the run-time-shaped family: the input limit (d + 1 <= 112), the widths
    wide = psp.LLGC(d=112, off_diag=0.01, T=0.4, device="cpu")
    r = pvn.value_eligibility(_Solver(wide, _net(112)))
    assert r is not None and "input <= 112" in r
    r = pvn.value_eligibility(_Solver(off, _net(d, (130, 130))))
    assert r is not None and "128" in r


def _query_config():
    c = nat.GenlConfig()
    c.base.d, c.base.K_local, c.base.N, c.base.h_kind = 20, 200, 20, nat.GH_QUAD
    c.has_time, c.n_hidden, c.widths[0], c.widths[1] = 1, 2, 30, 30
    return c


def test_query_lq_checks_the_struct():
    lib = nat.load()
    c, sz = _query_config(), nat.GenlSizes()
    n = C.sizeof(nat.GenlCoeffs)
    A, p = torch.zeros(20, 20), torch.ones(20)                       # (a query reads no pointer)
    assert lib.psp_genl_query(C.byref(c), C.byref(sz)) == 0
    plain = int(sz.table_bytes)
    # NULL, all zero, and a struct that asks for nothing: the plain plan
    for q in (None, C.byref(nat.GenlCoeffs()), C.byref(nat.GenlCoeffs(struct_bytes=n))):
        assert lib.psp_genl_query_lq(C.byref(c), q, C.byref(sz)) == 0 and int(sz.table_bytes) == plain
    # a wrong size
    q = nat.GenlCoeffs(struct_bytes=n - 8, z_kind=nat.GENL_Z_SIGMA)
    assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(sz)) != 0 and "struct_bytes" in nat.last_error()
    q = nat.GenlCoeffs(struct_bytes=0, z_kind=nat.GENL_Z_SIGMA)
    assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(sz)) != 0 and "struct_bytes" in nat.last_error()
    # DIAG_QUAD without its vector; with another h
    q = nat.GenlCoeffs(struct_bytes=n, runcost_kind=nat.RUNCOST_DIAG_QUAD)
    assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(sz)) != 0 and "vector missing" in nat.last_error()
    q.runcost = p.data_ptr()
    assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(sz)) == 0
    c.base.h_kind = nat.GH_ZERO
    assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(sz)) != 0 and "PSP_GH_QUAD" in nat.last_error()
    c.base.h_kind = nat.GH_QUAD
    # enums
    q = nat.GenlCoeffs(struct_bytes=n, z_kind=2)
    assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(sz)) != 0 and "enum" in nat.last_error()
    # a drift matrix together with the diagonal kind
    q = nat.GenlCoeffs(struct_bytes=n, drift_matrix=A.data_ptr())
    c.base.drift_kind, c.base.drift = nat.DRIFT_DIAG, p.data_ptr()
    assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(sz)) != 0 and "drift matrix" in nat.last_error()
    c.base.drift_kind, c.base.drift = nat.DRIFT_ZERO, None
    assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(sz)) == 0


def test_query_lq_table_growth_is_the_table_of_A():
    lib = nat.load()
    c, sz = _query_config(), nat.GenlSizes()
    n = C.sizeof(nat.GenlCoeffs)
    A = torch.zeros(20, 20)
    block = 2 * 2 * 256 * 4                                          # d + 1 = 21: DB0 x DB0 = 2 x 2 blocks of 256 floats
    assert lib.psp_genl_query(C.byref(c), C.byref(sz)) == 0
    plain = int(sz.table_bytes)
    q = nat.GenlCoeffs(struct_bytes=n, z_kind=nat.GENL_Z_SIGMA)     # the dense path: the tables of B = s I and B^T
    assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(sz)) == 0
    with_b = int(sz.table_bytes)
    assert plain + 2 * block <= with_b <= plain + 2 * block + 12    # (16-byte alignment of the first)
    q.drift_matrix = A.data_ptr()
    assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(sz)) == 0
    assert int(sz.table_bytes) == with_b + block
    # the other sizes do not depend on the coefficients
    base = nat.GenlSizes()
    assert lib.psp_genl_query(C.byref(c), C.byref(base)) == 0
    for f in ("path_bytes", "ahat_bytes", "n_params", "grad_partial_bytes", "n_blocks", "waves_per_tile"):
        assert getattr(sz, f) == getattr(base, f), f
    # the LDS rule is the dense path's: 4 x 128 hidden units on 112 inputs still fit (as with a dense sigma), and the shape limits hold
    c.base.d, c.n_hidden = 111, 4
    for i in range(4):
        c.widths[i] = 128
    assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(sz)) == 0
    c.base.d = 112
    assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(sz)) != 0 and "112" in nat.last_error()
