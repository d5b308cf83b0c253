"""Host side of the u_L2 log of the DenseNet-control forward (plan_dense_native.ul2_reference, include/psp.h PSP_UL2_*): the
description of u* the kernel reads, evaluated with a torch emulation of the kernel's arithmetic, against problem.u_true itself;
and the argument checks of the new psp_dnet_config fields.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

from util_cases import psp

nat = psp.native
pdn = psp.plan_dense_native


def emulate_u(ref, X, n):
    """u*(X, t_n) for the LOCAL trajectories X (K_local, d_pad) of the rank whose first global index is ref['k_offset'],
    with the arithmetic of hjbd_fwd_kernel<.., LOGU> (csrc/hjbd_kernels.h): fp32 throughout, a true division for the cell."""
    X = X.float()
    if ref["kind"] == nat.UL2_TABLE:
        return ref["table"][n].expand_as(X)
    if ref["kind"] == nat.UL2_LINEAR:
        return X @ ref["gains"][n].t()
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    xb, dx, xhi = f32(ref["xb"]), f32(ref["dx"]), f32(ref["xhi"])
    cell = torch.floor((torch.minimum(torch.maximum(X, -xb), xhi) + xb) / dx).long()
    if ref["k_offset"] + X.shape[0] == ref["K_global"]:
        cell[-1, :] -= 2                                 # the globally last trajectory
    cell = torch.where(cell < 0, cell + ref["ncols"], cell)
    tab = ref["tables"][ref["group"].long()]             # (d_pad, nrows, ncols)
    row = int(ref["row"][n])
    u = tab[torch.arange(X.shape[1]).view(1, -1), row, cell]
    u[:, ref["d"]:] = 0.0                                # the kernel reads no table for padding coordinates
    return u


def _u_true(problem, X, t):
    return torch.tensor(np.asarray(problem.u_true(X, t))).t().float()    # (K, d), as solver.py:493 forms it


def _states(K, d, seed, xb=None):
    g = torch.Generator().manual_seed(seed)
    X = 1.5 * torch.randn(K, d, generator=g)
    if xb is not None:
        X[0] = xb + 0.7                                  # beyond the grid on both sides
        X[1] = -xb - 0.3
        X[-1] = -xb + 0.25 * torch.rand(d, generator=g) * (xb / 100)   # last trajectory in the first cells: cell - 2 < 0
    return X


def _problems():
    out = [("llgc", psp.LLGC(d=5, off_diag=0.1, T=0.3, seed=3, device="cpu"), 0.01),
           ("lqgc", psp.LQGC(d=4, off_diag=0.1, T=0.3, seed=3, delta_t=0.005, device="cpu"), 0.01)]
    dw = psp.DoubleWell(d=1, T=0.2, eta=3.0, kappa=5.0, device="cpu")
    dw.compute_reference_solution(nx=400)
    mdw = psp.DoubleWell_multidim(d=5, d_1=2, d_2=3, T=0.2, eta=0.5, kappa=2.0, device="cpu")
    mdw.compute_reference_solution(nx=300)
    mdw.compute_reference_solution_2(nx=300)
    out += [("dw1", dw, 0.01), ("dw_multi", mdw, 0.01)]
    return out


@pytest.mark.parametrize("name,problem,dt", _problems(), ids=lambda v: v if isinstance(v, str) else "")
def test_description_reproduces_u_true(name, problem, dt):
    d, K = problem.d, 37
    N = int(np.floor(problem.T / dt))
    d_pad = 16
    grid = name.startswith("dw")
    X = _states(K, d, seed=11, xb=problem.xb if grid else None)
    Xp = torch.zeros(K, d_pad)
    Xp[:, :d] = X
    # one rank (k_offset 0), an upper rank that holds the last trajectory, a lower rank that does not
    for lo, hi in ((0, K), (20, K), (5, 20)):
        ref = pdn.ul2_reference(problem, N, dt, d_pad, K, lo)
        assert ref is not None and ref["kind"] == {"llgc": 0, "lqgc": 1}.get(name, 2)
        for n in range(N):
            want = _u_true(problem, X, n * dt)[lo:hi]
            got = emulate_u(ref, Xp[lo:hi], n)
            assert float(got[:, d:].abs().max()) == 0.0
            got = got[:, :d]
            if grid:
                assert torch.equal(got, want), (name, n, lo, hi)
            else:
                assert float((got - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max())), (name, n)


def test_last_trajectory_wraps_like_numpy():
    dw = psp.DoubleWell(d=1, T=0.1, eta=3.0, kappa=5.0, device="cpu")
    dw.compute_reference_solution(nx=400)
    ref = pdn.ul2_reference(dw, 10, 0.01, 16, 8, 0)
    X = torch.full((8, 16), -dw.xb - 1.0)               # every trajectory clamped into cell 0
    u = emulate_u(ref, X, 3)[:, 0]
    row = int(ref["row"][3])
    assert float(u[0]) == float(np.float32(dw.u[row, 0]))
    assert float(u[-1]) == float(np.float32(dw.u[row, -2]))     # cell 0 - 2 -> the second-to-last column
    want = _u_true(dw, X[:, :1], 3 * 0.01)[:, 0]
    assert torch.equal(u, want)


def test_no_description_keeps_the_composite_plan_reason():
    dw = psp.DoubleWell(d=1, T=0.1, eta=3.0, kappa=5.0, device="cpu")       # no compute_reference_solution yet
    assert pdn.ul2_kind(dw) is None and pdn.ul2_reference(dw, 10, 0.01, 16, 8, 0) is None
    model = psp.Solver("x", dw, K=32, L=1, delta_t=0.01, verbose=False, device="cpu")
    model.device = torch.device("cuda")                                    # (eligibility only: nothing runs)
    reason = pdn.dense_eligibility(model)
    assert "u_true_tables" in reason and "u_l2_error_flag" in reason


def _dnet_cfg():
    c = nat.DnetConfig()
    b = c.base
    b.d, b.H, b.K_local, b.N, b.K_global = 16, 32, 32, 4, 32
    b.dt, b.sqrt_dt = 0.01, 0.1
    b.drift_kind, b.sigma_kind = nat.DRIFT_DENSE, nat.SIGMA_DENSE
    b.adaptive, b.store_path = 1, 0
    c.d_real, c.H_real, c.per_step = 10, 30, 1
    return c


@pytest.fixture(scope="module")
def lib():
    if not nat.is_built():
        import __graft_entry__
        __graft_entry__.build()
    return nat.load()


def _fwd_error(lib, c):
    dummy = (C.c_float * 64)()
    part = (C.c_double * 64)()
    rc = lib.psp_dnet_rollout_fwd(C.byref(c), dummy, dummy, 0, None, None, 1, 0, None, None, None, dummy, None, None, None,
                                  part, dummy, None)
    assert rc != 0
    return nat.last_error()


def test_ul2_fields_are_validated_before_any_launch(lib):
    buf = (C.c_float * 64)()
    ibuf = (C.c_int32 * 64)()
    c = _dnet_cfg()
    c.ul2_kind = 3
    assert "ul2_kind out of range" in _fwd_error(lib, c)
    c = _dnet_cfg()
    c.ul2_kind = -1
    assert "ul2_kind out of range" in _fwd_error(lib, c)
    c = _dnet_cfg()
    c.ul2_kind = nat.UL2_LINEAR
    assert "needs ul2_tables" in _fwd_error(lib, c)
    c.ul2_tables = C.cast(buf, C.c_void_p)
    assert "needs base.u_l2_out" in _fwd_error(lib, c)
    c.base.u_ref = C.cast(buf, C.c_void_p)
    assert "base.u_ref is the PSP_UL2_TABLE reference" in _fwd_error(lib, c)
    c = _dnet_cfg()
    c.ul2_kind = nat.UL2_GRID
    c.ul2_tables = C.cast(buf, C.c_void_p)
    c.base.u_l2_out = C.cast(buf, C.c_void_p)
    assert "needs ul2_group" in _fwd_error(lib, c)
    c.ul2_group = C.cast(ibuf, C.c_void_p)
    assert "needs ul2_row" in _fwd_error(lib, c)
    c.ul2_row = C.cast(ibuf, C.c_void_p)
    assert "must be positive" in _fwd_error(lib, c)
    c.ul2_ntables, c.ul2_nrows, c.ul2_ncols = 1, 4, 8
    assert "ul2_xb / ul2_dx must be positive" in _fwd_error(lib, c)
    c = _dnet_cfg()
    c.base.u_ref = C.cast(buf, C.c_void_p)                       # kind 0: the entry point of the narrow family
    assert "needs base.u_l2_out" in _fwd_error(lib, c)


def test_query_sizes_the_gain_tables(lib):
    c = _dnet_cfg()
    s0 = nat.DnetSizes()
    assert lib.psp_dnet_query(C.byref(c), C.byref(s0)) == 0
    buf = (C.c_float * 64)()
    c.ul2_kind, c.ul2_tables, c.base.u_l2_out = nat.UL2_LINEAR, C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p)
    s1 = nat.DnetSizes()
    assert lib.psp_dnet_query(C.byref(c), C.byref(s1)) == 0
    assert s1.table_bytes - s0.table_bytes == 4 * c.base.N * 16 * 16


def test_grid_tables_the_kernel_cannot_read_have_precise_reasons():
    dw = psp.DoubleWell(d=1, T=0.2, eta=3.0, kappa=5.0, device="cpu")
    dw.compute_reference_solution(nx=400)
    assert pdn.ul2_unsupported(dw, 20, 0.01) is None
    reason = pdn.ul2_unsupported(dw, 40, 0.01)                  # the solver's grid runs past the tables' last row
    assert reason is not None and "end at t = 0.2" in reason
    with pytest.raises(ValueError, match="end at"):
        pdn.ul2_reference(dw, 40, 0.01, 16, 8, 0)

    class Uneven:
        d, T = 2, 0.1

        def u_true(self, x, t):
            raise AssertionError("not called")

        def u_true_tables(self):
            return dict(tables=[np.zeros((21, 99)), np.zeros((21, 49))], group_of_dim=[0, 1], xb=2.5, dx=0.05, delta_t=0.005)

    reason = pdn.ul2_unsupported(Uneven(), 10, 0.01)
    assert reason is not None and "unequal shapes" in reason
    with pytest.raises(ValueError, match="unequal shapes"):
        pdn.ul2_reference(Uneven(), 10, 0.01, 16, 8, 0)
