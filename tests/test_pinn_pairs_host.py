"""Host side of the native PINN plan for an h that reads t: the pinn_time_h keyword, the reasons pinn_eligibility gives, what
psp_pinn_pairs_query accepts and refuses, and null buffers.  No GPU."""
import ctypes as C

import pytest

import ref64_pinn_pairs as rp
from conftest import load_golden
from pinn_cases import COMPOSITE_ONLY, build
from pinn_kernel_cases import pinn_config
from util_cases import psp

nat = psp.native
READS_T = ("pinn_expsphere_par_d3", "pinn_expsphere_par_d3_neumann")
H_PAR = (C.c_float * 4)


def config(d=10, has_time=1, widths=(20,), K=8, **over):
    c = nat.PinnConfig()
    c.d, c.K, c.has_time, c.n_hidden = d, K, has_time, len(widths)
    for i, h in enumerate(widths):
        c.widths[i] = h
    c.sigma_scale, c.h_kind, c.h_par = 1.0, nat.GH_EXPBALL_SIN, H_PAR(0.5, 10.0, 1.0, 1.0)
    for k, v in over.items():
        setattr(c, k, v)
    return c


def pairs_query(c):
    sz, work = nat.PinnSizes(), C.c_int64(-1)
    return nat.load().psp_pinn_pairs_query(C.byref(c), C.byref(sz), C.byref(work)), sz, work.value


def test_keyword_is_validated_in_the_constructor():
    case = load_golden(READS_T[0])["case"]
    with pytest.raises(ValueError, match="pinn_time_h"):
        build(case, pinn_time_h="device")
    assert build(case)[1].pinn_time_h == "torch"
    assert build(case, pinn_time_h="native")[1].pinn_time_h == "native"


@pytest.mark.parametrize("name", READS_T)
def test_native_only_lacks_a_gpu_here_and_the_default_keeps_its_reason(name):
    case = load_golden(name)["case"]
    reason = psp.plan_pinn_native.pinn_eligibility
    why = reason(build(case, pinn_time_h="native")[1])
    assert "need a GPU" in why and "reads t" not in why
    why = reason(build(case)[1])
    assert COMPOSITE_ONLY[name] in why and "pinn_time_h" in why
    _, model = build(case, backend="native")                      # the default plan of this configuration is still the composite
    with pytest.raises(NotImplementedError, match="reads t"):
        model.train_PINN()
    _, model = build(case, pinn_time_h="native", L=1)             # no GPU: the keyword alone changes no number
    model.train_PINN()
    assert model.plan_name == "torch" and "need a GPU" in model.plan_reason


def test_keyword_is_ignored_where_h_does_not_read_t():
    case = load_golden("pinn_heat_d6")["case"]
    reason = psp.plan_pinn_native.pinn_eligibility
    assert reason(build(case, pinn_time_h="native")[1]) == reason(build(case)[1])


def test_keyword_is_part_of_the_plan_key(monkeypatch):
    """_choose_pinn_plan rebuilds its plan when the keyword changes (seen through a stand-in plan class: no GPU here)."""
    ppn = psp.plan_pinn_native
    _, model = build(load_golden("pinn_heat_d6")["case"])
    made = []

    class Plan:
        def __init__(self, solver):
            self.net, self.key = solver.V, None
            self.flat = next(iter(solver.V.parameters())).data
            self.params = [self.flat]
            made.append(self)

    monkeypatch.setattr(ppn, "pinn_eligibility", lambda s: None)
    monkeypatch.setattr(ppn, "PinnNativePlan", Plan)
    first = model._choose_pinn_plan()
    assert model._choose_pinn_plan() is first
    model.pinn_time_h = "native"
    assert model._choose_pinn_plan() is not first and len(made) == 2


@pytest.mark.parametrize("name", sorted(rp.CASES))
def test_pairs_query_accepts_the_kernel_test_shapes(name):
    case = rp.make(name)
    rc, sz, work = pairs_query(pinn_config(case))
    assert rc == 0, nat.last_error()
    assert work == 8 * case["K"]
    n_in = case["d"] + 1
    assert sz.n_params == sum(p.numel() for p in case["params"])
    assert sz.dir_blocks == (n_in + 13) // 14 and sz.tiles == case["K"] * sz.dir_blocks
    assert sz.scratch_bytes == 4 * case["K"] * (2 + sz.dir_blocks + 2 * n_in)          # the layout of psp_pinn_query, unchanged
    old = nat.PinnSizes()                                                                # which still refuses the same config
    assert nat.load().psp_pinn_query(C.byref(pinn_config(case)), C.byref(old)) == -1


def test_pairs_query_limits():
    assert pairs_query(config())[0] == 0
    assert pairs_query(config(h_kind=nat.GH_EXPBALL_SQ, h_par=H_PAR(0.5, 10.0, 0.0, -0.25)))[0] == 0     # any tau
    assert pairs_query(config(h_par=H_PAR(0.5, 10.0, 1.0, 0.0)))[0] == 0
    assert pairs_query(config(h_kind=nat.GH_ALLEN_CAHN, h_par=H_PAR(0.0, 0.0, 0.0, 0.0)))[0] == 0       # tau = 0: every h_kind
    rc, _, _ = pairs_query(config(d=10, has_time=0))
    assert rc == -1 and "time input" in nat.last_error()
    rc, _, _ = pairs_query(config(sigma_kind=nat.GENL_SIGMA_DENSE, n_dirs=3))
    assert rc == -1 and "dense sigma" in nat.last_error()
    for kind in (nat.GH_EXPBALL_LIN, nat.GH_EXPBALL_SIN_FULL):
        rc, _, _ = pairs_query(config(h_kind=kind))
        assert rc == -1 and "read t" in nat.last_error()
    assert pairs_query(config(K=16384))[0] == 0                                                          # the stated cap
    rc, _, _ = pairs_query(config(K=16385))
    assert rc == -1 and "16384" in nat.last_error()
    assert pairs_query(config(widths=(129,)))[0] == -2                                                   # psp_pinn_query's limits hold
    assert pairs_query(config(K=0))[0] == -1
    lib = nat.load()
    assert lib.psp_pinn_pairs_query(None, None, None) == -1
    assert lib.psp_pinn_pairs_query(C.byref(config()), None, None) == -1


def test_old_entry_points_still_refuse_an_h_that_reads_t():
    lib, c = nat.load(), config()
    one = C.c_void_p(8)                                                                  # never dereferenced: the config is refused first
    assert lib.psp_pinn_query(C.byref(c), C.byref(nat.PinnSizes())) == -1 and "reads t" in nat.last_error()
    assert lib.psp_pinn_residual(C.byref(c), one, one, one, one, one, None) == -1 and "reads t" in nat.last_error()
    assert lib.psp_pinn_backward(C.byref(c), one, one, one, one, one, one, one, None) == -1 and "reads t" in nat.last_error()
    assert lib.psp_version() == 400


def test_null_buffers_are_rejected_before_any_launch():
    lib, c = nat.load(), config()
    p = C.c_void_p(8)                                                                    # never dereferenced: a null is found first
    for i in range(5):                                           # params, x, t, scratch, A_out
        args = [p] * 5
        args[i] = None
        assert lib.psp_pinn_pairs_residual(C.byref(c), *args, None) == -1
        assert "null buffer" in nat.last_error()
    for i in range(8):                                           # x, t, scratch, A | pair_work, loss_out, rho_out, nu_out
        args = [p] * 8
        args[i] = None
        assert lib.psp_pinn_pairs_reduce(C.byref(c), *args[:4], 1.0, *args[4:], None) == -1
        assert "null buffer" in nat.last_error()
    for i in (0, 1, 2, 3, 4, 6, 7):                              # params, x, t, scratch, rbar, (vadd may be null), partial, out
        args = [p] * 8
        args[i] = None
        assert lib.psp_pinn_pairs_backward(C.byref(c), *args, None) == -1
        assert "null buffer" in nat.last_error()
