"""The bf16-operand float64 reference of the control-net Solver (tests/ref64.py: iteration(..., operands='bf16')) and the case table
it judges (tests/block_cases.py: BF16_CASES), checked on the CPU:

  a. operands='fp32' is the exact reference to float64 rounding; operands='bf16' is not;
  b. the custom product passes gradcheck with the rounding off, rounds both operands with it on, and its backward with the rounding
     on is the fp32 one on the UNROUNDED operands -- not the adjoint of the rounded product;
  c. a torch stand-in of the kernels -- the same statements in fp32 on operands cast through torch.bfloat16, on the same draws --
     passes the criterion of tests/test_gpu_bf16_blocks.py with c = 1/4, half the GPU test's margin, on every case: the inputs are
     such that operands which an fp32-sized perturbation moves to the other bf16 neighbour stay well inside the bound (measured:
     at most 0.16 e_model on D, the store_path 4 case with its 8208 trajectories, 0.13 at (48, 48), 0.09 on a gradient block);
  d. no case is vacuous: e_model of the blocks of the three rounded products' weights (W1x, W2, W3) is at least five times the
     fp32 block bound (measured 1.4e-3 .. 7e-3 against 2e-4); leaving any ONE of the three products unrounded misses the criterion
     on the (10, 30) case;
  e. the cases are in the nonlinear regime (as tests/test_ref64.py asserts of CASES) and cover what they are there for.
"""
import math

import pytest
import torch

import block_cases as bc
import ref64
from test_ref64 import cpu_noise
from util_cases import BLOCK_NAMES, block_errors, grad_blocks

D_TOL, BLOCK_TOL = 2e-5, 2e-4          # the fp32 bounds of tests/test_gpu_block_gradients.py
STANDIN_C = bc.BF16_C / 2
IDS = [c["id"] for c in bc.BF16_CASES]


def three(c):
    """(exact, model, stand-in) of a case, each computed once."""
    K = bc.case_K(c)
    noise = lambda: cpu_noise(c, K)
    return (bc.reference(c, K, noise), bc.reference(c, K, noise, operands="bf16"),
            bc.reference(c, K, noise, operands="bf16", dtype=torch.float32))


def test_fp32_operands_are_the_exact_reference_and_bf16_operands_are_not():
    c = bc.BF16_CASES[0]
    K = bc.case_K(c)
    oprob, ocfg, z = bc.scaled_oracle(c, K)
    xi = cpu_noise(c, K)
    ref64_product = ref64.product
    try:                                                                   # the reference as it stood before the switch: plain matmuls
        ref64.product = lambda a, W, operands="fp32": a @ W.t()
        plain = ref64.iteration(oprob, ocfg, z, xi)
    finally:
        ref64.product = ref64_product
    exact = ref64.iteration(oprob, ocfg, z, xi, operands="fp32")
    model = ref64.iteration(oprob, ocfg, z, xi, operands="bf16")
    assert float((exact["D"] - plain["D"]).abs().max()) <= 1e-12 * float(plain["D"].abs().max())
    assert max(block_errors(exact["grad"], plain["grad"], c["d"], c["H"])) <= 1e-12
    assert math.isclose(exact["loss"], plain["loss"], rel_tol=1e-12)
    assert min(block_errors(model["grad"], exact["grad"], c["d"], c["H"])) > 1e-3
    assert float((model["D"] - exact["D"]).abs().max()) > 1e-3


def test_product_gradcheck_and_rounding_points():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(5, 7, dtype=torch.float64, generator=g, requires_grad=True)
    W = torch.randn(4, 7, dtype=torch.float64, generator=g, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, W: ref64.product(a, W, "fp32"), (a, W))
    rb = ref64.rb
    assert torch.equal(rb(a), a.to(torch.bfloat16).double()) and not torch.equal(rb(a), a)
    # round to nearest even: 1 + 2^-8 is a tie between 1 and 1 + 2^-7 and goes to the even mantissa, 1 + 3 * 2^-8 goes up to 1 + 2^-6
    assert rb(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)).tolist() == [1.0, 1.0 + 2.0 ** -6]
    out = ref64.product(a, W, "bf16")
    assert torch.equal(out, rb(a) @ rb(W).t())
    v = torch.randn(5, 4, dtype=torch.float64, generator=g)
    ga, gW = torch.autograd.grad((out * v).sum(), (a, W))
    assert torch.equal(ga, v @ W.detach()) and torch.equal(gW, v.t() @ a.detach())           # unrounded: the fp32 backward kernels
    assert not torch.allclose(ga, v @ rb(W.detach()), rtol=1e-6, atol=0.0)                    # (a straight-through rounding op gives this)


@pytest.mark.parametrize("c", bc.BF16_CASES, ids=IDS)
def test_the_fp32_stand_in_passes_the_gpu_criterion_with_half_the_margin(c):
    exact, model, standin = three(c)
    bc.assert_bf16(c, standin, model, exact, STANDIN_C, D_TOL, BLOCK_TOL, tag=c["id"])


@pytest.mark.parametrize("c", bc.BF16_CASES, ids=IDS)
def test_no_case_is_vacuous_and_every_case_is_in_the_nonlinear_regime(c):
    exact, model, _ = three(c)
    _, em = bc.bf16_errors(c, model, model, exact)
    e = dict(zip(BLOCK_NAMES, em["blocks"]))
    print("%s: e_model D %.2e  %s" % (c["id"], em["D"], "  ".join("%s %.2e" % x for x in e.items())))
    assert min(e["W1x"], e["W2"], e["W3"]) >= 5 * BLOCK_TOL, e
    assert em["D"] >= 5 * D_TOL, em["D"]
    m1, m2 = float(exact["h1"].abs().median()), float(exact["h2"].abs().median())
    bm = [float(b.abs().max()) for b in grad_blocks(exact["grad"], c["d"], c["H"])]
    assert 0.15 <= m1 <= 0.85 and 0.15 <= m2 <= 0.85, (m1, m2)
    assert float(exact["D"].abs().max()) < 200.0 and min(bm) > 2e-2 * max(bm), bm


@pytest.mark.parametrize("skip", [0, 1, 2])
def test_one_product_left_unrounded_misses_the_criterion(skip):
    """What a kernel that forgot a rounding point -- or a reference that models one too many -- looks like to the criterion."""
    c = bc.BF16_CASES[0]
    exact, model, _ = three(c)
    K = bc.case_K(c)
    oprob, ocfg, z = bc.scaled_oracle(c, K)
    calls = [0]
    keep = ref64.product

    def product(a, W, operands="fp32"):
        calls[0] += 1
        return keep(a, W, "fp32" if (calls[0] - 1) % 3 == skip else operands)
    try:
        ref64.product = product
        wrong = ref64.iteration(oprob, ocfg, z, cpu_noise(c, K), operands="bf16")
    finally:
        ref64.product = keep
    assert calls[0] == 3 * c["N"]
    ek, em = bc.bf16_errors(c, wrong, model, exact)
    print("product %d unrounded: D %.2f e_model, blocks %s" % (skip, ek["D"] / em["D"], " ".join("%.2f" % (a / b) for a, b in zip(ek["blocks"], em["blocks"]))))
    with pytest.raises(AssertionError):
        bc.assert_bf16(c, wrong, model, exact, bc.BF16_C, D_TOL, BLOCK_TOL, tag="product %d unrounded" % skip)


def test_the_table_covers_what_it_is_there_for():
    cs = bc.BF16_CASES
    assert all(c["mode"] == "bf16" and c["expect"][0] == 1 and case_seconds_small(c) for c in cs)
    for inst in bc.BF16_OVERRUN:                                          # each overrunning instance on both compiled forwards
        assert {c["noise"] for c in cs if c["expect"][1:] == inst and (c["d"], c["H"]) == inst} == {"reference", "philox"}, inst
        assert {c["detach"] for c in cs if c["expect"][1:] == inst} == {True, False}, inst
    blocks = {(-(-c["expect"][1] // 16), -(-c["expect"][2] // 16)) for c in cs}
    assert any(db % 2 and hb % 2 and db > 1 for db, hb in blocks) and any(db % 2 and not hb % 2 and db > 1 for db, hb in blocks)   # (48, 48); (100, 64)
    assert any((c["d"], c["H"]) != c["expect"][1:] for c in cs) and any((c["d"], c["H"]) == c["expect"][1:] for c in cs)
    assert any(c["expect"][1:] == (16, 16) for c in cs)                      # fp32 and bf16 images of every table equal
    assert any(c["regen"] for c in cs)                                       # store_path 4
    assert any(isinstance(c["K"], int) and c["K"] % 16 and c["K"] > 256 for c in cs)      # ragged, more than one workgroup of 16 waves
    assert {c["kind"] for c in cs} == set(ref64.KINDS)
    for noise in ("reference", "philox"):
        assert {c["detach"] for c in cs if c["noise"] == noise} == {True, False}


def case_seconds_small(c):
    """K <= 300 and N <= 20, but for the one store_path 4 case, which needs more than two tiles per CU (N = 3 there)."""
    return c["N"] <= 20 and (c["K"] == "cu" and c["N"] <= 3 or c["K"] != "cu" and c["K"] <= 300)
