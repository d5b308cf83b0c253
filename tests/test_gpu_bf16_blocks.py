"""Solver(mlp_dtype='bf16') -- hjb_fwd_kernel<D, H, MODE = 1> and the fp32 backward behind it -- against a float64 reference that
rounds what the kernel rounds (tests/ref64.py: iteration(..., operands='bf16')), block by block.

Every judged quantity q (per-trajectory D, the loss, each of the seven gradient blocks) has three values: q_exact (float64), q_model
(float64, both operands of the three control-net products rounded to bf16) and q_kernel.  With e_model = |q_model - q_exact| and
e_kernel = |q_kernel - q_model| in the normalisation of tests/test_gpu_block_gradients.py,

    e_kernel <= 1/2 e_model + (that test's fp32 bound: D 2e-5, each block 2e-4, the loss its conditioning rule),

and for the loss e_model is max(e_model(loss), e_model(D)).  1/2 comes from the reference, not from the kernels: a torch stand-in
(fp32 arithmetic on bf16-rounded operands, tests/test_ref64_bf16.py) stays within 0.16 e_model on every case of the table, one
product left unrounded costs 0.5 .. 1.0 e_model, and a weight table that overruns its LDS carve costs about 100 e_model.  e_model
itself is 1e-3 .. 1e-2 on every weight block, five times the fp32 bound at least (asserted on the CPU), so no case is vacuous.

Cases (tests/block_cases.py: BF16_CASES): the four instances with d <= 12, whose bf16 W1 image is larger than the fp32 one and
overran Geo's carve until it was sized for both (csrc/hjb_kernels.h: Geo::tbl) -- each on supplied noise (FAST = 0 instance) and on
Philox noise (FAST = 1), detached and attached; d = 5, H = 20 padded onto (8, 30); (16, 16), where the two images are equal;
(20, 30) with a ragged K over 19 tiles; (48, 48) and (100, 64), whose odd block counts take the zero-filled half k-step of gemm_Tb;
(48, 64); store_path 4.  The plan accepts the mode detached and attached on every case; the wide family declines it (asserted).

Measured on an MI355X (19 tests in 5.4 s), worst e_kernel / e_model per route (the test prints them; bound 1/2 plus the fp32 term):
  route        D      block         loss        route        D      block         loss
  bf16-d10     0.292  0.199 (W1x)   0.021       bf16-20x30   0.061  0.008 (b1)    0.001
  bf16-d2      0.008  0.001 (W1t)   0.000       bf16-48x48   0.131  0.085 (W3)    0.026
  bf16-d4      0.000  0.000         0.000       bf16-48x64   0.064  0.031 (W1x)   0.003
  bf16-d8      0.002  0.003 (W3)    0.001       bf16-100x64  0.020  0.009 (b3)    0.005
  bf16-pad-d5  0.000  0.000         0.000       bf16-store4  0.101  0.003 (W1x)   0.001
  bf16-16x16   0.000  0.000         0.000
The largest, (10, 30) over N = 20 steps, is one hidden unit rounding to the other bf16 neighbour (tanh_f32 and the fp32 time feature
differ from float64 in the last bits).  On the parent's library, whose Geo carved W1's table by the fp32 image alone, the nine cases
on (2, 30), (4, 30), (8, 30), (10, 30) miss every quantity: D 0.22 .. 0.75 and blocks 0.03 .. 3.4 absolute, 50 .. 1000 e_model; the
(16, 16) cases pass there as here.
"""
import pytest
import torch

import block_cases as bc
from test_gpu_block_gradients import BLOCK_TOL, D_TOL, assert_route, philox_noise, run_case
from util_cases import BLOCK_NAMES, make_pkg_solver

pytestmark = pytest.mark.gpu

WORST = {}                   # route -> {quantity: (largest e_kernel / e_model, case id)}: printed by the last case of the module


@pytest.mark.parametrize("c", bc.BF16_CASES, ids=[c["id"] for c in bc.BF16_CASES])
def test_bf16_first_iteration_matches_the_float64_bf16_operand_reference(c, monkeypatch):
    model, plan, K = run_case(c, monkeypatch)
    assert_route(c, model, plan)
    assert plan.state_basis == "x"                                       # (the mode keeps the two d x d products: plan_native.py)
    draw = philox_noise if c["noise"] == "philox" else bc.host_noise
    noise = lambda: draw(int(model.seed), K, c["d"], c["N"])
    exact = bc.reference(c, K, noise)
    ref = bc.reference(c, K, noise, operands="bf16")
    got = dict(D=plan.D, loss=float(model.loss_log[0]), grad=plan.grad.cpu())
    assert got["grad"].shape == ref["grad"].shape
    ek, em = bc.bf16_errors(c, got, ref, exact)
    w = WORST.setdefault(c["route"], {})
    for name, a, b in [("D", ek["D"], em["D"]), ("loss", ek["loss"], em["loss"])] + list(zip(BLOCK_NAMES, ek["blocks"], em["blocks"])):
        key = name if name in ("D", "loss") else "block"
        if a / b > w.get(key, (-1.0,))[0]:
            w[key] = (a / b, name, c["id"])
    try:
        bc.assert_bf16(c, got, ref, exact, bc.BF16_C, D_TOL, BLOCK_TOL, tag=c["id"])
    finally:
        if c is bc.BF16_CASES[-1]:
            for route, q in sorted(WORST.items()):
                print("worst e_kernel / e_model per route: %-12s %s" % (route, "  ".join("%s %.3f (%s)" % (k, v[0], v[1]) for k, v in sorted(q.items()))))


def test_the_wide_family_declines_the_bf16_control_net_mode():
    """d = 120 runs on the wide kernels, which have no bf16 forward: the library says so and nothing falls back quietly."""
    c = bc._c("wide-bf16", "LLGC", 120, 64, 48, 3, True, "bf16", (2, 128, 64))
    model = make_pkg_solver(bc.golden_style(c, 48), torch.device("cuda:0"), backend="native", noise="reference", L=1, mlp_dtype="bf16")
    with pytest.raises(RuntimeError, match="bf16 control-net mode exists for the narrow kernel family only"):
        model.train()
