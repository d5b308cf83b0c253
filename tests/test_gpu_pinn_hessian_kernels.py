"""The direction-table route of the PINN kernels (csrc/pinn_kernels.h, PSP_GENL_SIGMA_DENSE) on the GPU, through the C ABI with
NaN-filled buffers, against the float64 statement of ref64_pinn_dense.py.  The project's bound per named parameter block and per
output vector: e_native <= 8 e_fp32 + 1e-6 with e = max|v - v64| / max|v64|, the fp32 autograd statement as the yardstick."""
import ctypes as C

import pytest
import torch

import pinn_hessian_kernel_cases as hc
import pinn_kernel_cases as kc

pytestmark = pytest.mark.gpu
nat = hc.nat


def run_case(name):
    ref = hc.reference(name)
    run = hc.Native(ref["case"])
    R = run.residual().clone()
    parts = {k: v.clone() for k, v in run.scratch_parts().items()}
    grads = {}
    for key, rbar in ref["rbar"].items():
        grads[key] = run.backward(rbar).clone()
        kc.check_finite(run.R, run.grad, run.partial[:run.sz.bwd_workgroups * run.sz.n_params])
        run.check_padding()
    got = dict(R=R, V=parts["V"], gradV=parts["gradV"], lap_parts=parts["lap_parts"], grads=grads)
    return ref, run, got


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_every_block_matches_float64(name):
    ref, run, got = run_case(name)
    assert (run.sz.dir_blocks, run.sz.tiles, run.sz.bwd_workgroups) == hc.CASES[name][4][2:]
    rows = hc.evaluate(ref, got)
    print("%s (%s)\n%s" % (name, hc.CASES[name][3], kc.table(rows)))
    kc.assert_rows(rows)


def test_both_tables_of_the_ones_matrix_give_the_same_residual():
    """sqrt(2) 1 given directly and the eigh factor of sqrt(2/d) ones(d, d) on the same points: each within the bound (above), and
    one direction either way."""
    a, b = hc.reference("rank1"), hc.reference("rank1_eigh")
    assert a["case"]["dirs"].shape == b["case"]["dirs"].shape == (1, 4)
    assert torch.equal(a["case"]["x"], b["case"]["x"])
    Ra, Rb = hc.Native(a["case"]).residual().clone(), hc.Native(b["case"]).residual().clone()
    for R, ref in ((Ra, a), (Rb, b)):
        kc.assert_rows([kc.row("R", R, ref["f64"]["R"], ref["f32"]["R"])])


def test_backward_is_deterministic_on_the_stride_case():
    ref = hc.reference("stride")
    run = hc.Native(ref["case"])
    R = run.residual().clone()
    g1 = run.backward(ref["rbar"]["random"]).clone()
    g2 = run.backward(ref["rbar"]["random"])
    assert torch.equal(g1, g2) and torch.equal(run.residual(), R)


def test_query_limits_on_the_device():
    case = hc.make("rank1")
    dirs = case["dirs"].to("cuda:0", torch.float32).contiguous()
    rc, _ = hc.query(hc.pinn_config(case, dirs_ptr=None))
    assert rc == -4 and "dense sigma" in nat.last_error()
    assert hc.query(hc.pinn_config(case, dirs_ptr=nat.ptr(dirs), n_dirs=0))[0] == -1
    assert hc.query(hc.pinn_config(case, dirs_ptr=nat.ptr(dirs), n_dirs=case["d"] + 1))[0] == -1
    c = hc.pinn_config(case, dirs_ptr=nat.ptr(dirs))
    c.h_kind = nat.GH_QUAD
    assert hc.query(c)[0] == -1
    R = torch.full((case["K"],), float("nan"), device="cuda:0")    # a refused config launches nothing
    rc = nat.load().psp_pinn_residual(C.byref(c), nat.ptr(dirs), nat.ptr(dirs), None, nat.ptr(dirs), nat.ptr(R), None)
    torch.cuda.synchronize()
    assert rc == -1 and bool(torch.isnan(R).all())
