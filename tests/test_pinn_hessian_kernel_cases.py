"""The case table of the direction-table kernel tests (pinn_hessian_kernel_cases.py), on the CPU: every case stays in the regime
its bound assumes, relu^2 cases keep their distance from the kink, and psp_pinn_query answers the geometry each case claims."""
import ctypes as C

import pytest

import pinn_hessian_kernel_cases as hc
import ref64_pinn as r64
from util_cases import psp

nat = psp.native


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_case_stays_in_the_fp32_regime(name):
    ref = hc.reference(name)
    rows = hc.regime_rows(ref)
    print("\n".join("    %-30s e_torch32 %.2e" % r for r in rows))
    bad = [r for r in rows if not r[1] <= hc.REGIME_CAP]
    assert not bad, bad
    if ref["case"]["act"] == "relu2":
        assert r64.preact_margin(ref["case"]) >= 1e-5


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_query_answers_the_geometry_the_case_claims(name):
    case = hc.make(name)
    n_grad, n_hess, blocks, tiles, wgs = hc.CASES[name][4]
    assert hc.layout(case) == (n_grad, n_hess, blocks)
    anything = (C.c_float * 1)()                                  # psp_pinn_query tests the table for NULL only
    c = hc.pinn_config(case, dirs_ptr=C.cast(anything, C.c_void_p))
    if case["drift"] is not None:
        c.drift = C.cast(anything, C.c_void_p)
    rc, sz = hc.query(c)
    assert rc == 0, nat.last_error()
    assert (sz.dir_blocks, sz.tiles, sz.bwd_workgroups) == (blocks, tiles, wgs)
    assert sz.scratch_bytes == 4 * case["K"] * (2 + blocks + 2 * n_grad)
    assert sz.grad_partial_bytes == 4 * sz.n_params * wgs


def test_query_limits_of_the_direction_table():
    case = hc.make("rank1")
    some = C.cast((C.c_float * 1)(), C.c_void_p)
    rc, _ = hc.query(hc.pinn_config(case, dirs_ptr=None))
    assert rc == -4 and "dense sigma" in nat.last_error()
    assert hc.query(hc.pinn_config(case, dirs_ptr=some, n_dirs=0))[0] == -1
    assert hc.query(hc.pinn_config(case, dirs_ptr=some, n_dirs=case["d"] + 1))[0] == -1
    assert hc.query(hc.pinn_config(case, dirs_ptr=some, n_dirs=case["d"]))[0] == 0
    c = hc.pinn_config(case, dirs_ptr=some)
    c.h_kind = nat.GH_QUAD
    assert hc.query(c)[0] == -1 and "reads z" in nat.last_error()
    c = hc.pinn_config(case, dirs_ptr=some)                       # the full-Hessian h on the scaled path as well
    c.sigma_kind, c.sigma_scale = nat.GENL_SIGMA_SCALED, 1.0
    assert c.h_kind == nat.GH_EXPBALL_SIN_FULL and hc.query(c)[0] == 0
