"""The bf16-operand float64 reference of the templated value-net kernels (tests/ref64_general.py: iteration(..., operands='bf16')) and
its case tables (tests/general_block_cases.py: BF16_CASES for 'bf16_fwd', BF16_FULL_CASES for the full 'bf16' mode, whose gradient
is ref64_general.kernel_backward with the bf16 backward's rounding points), checked on the CPU on the fp32 oracle's draws of every case -- the
Philox cases too: their device draws exist on the GPU only, the configuration is the same:

  a. the kernels' three sweeps with exact products (sweeps=True, operands='fp32') are the autograd reference to float64 rounding:
     end points, loss and every gradient block; with operands='bf16' they are not; and the kernels' backward written out by hand
     (kernel_backward, rounded=False) is the autograd gradient of the same forward, with exact and with bf16 operands;
  b. every case meets the conditions of tests/test_ref64_general.py on its exact reference, and the discrete results (active steps)
     of the bf16-operand model equal the exact ones, so that the two can be compared trajectory by trajectory;
  c. a torch stand-in of the kernels -- the same statements in fp32 on operands cast through torch.bfloat16 -- passes the criterion
     of tests/test_gpu_general_bf16_blocks.py with c = 1/4, half the GPU test's margin (measured: at most 0.01 e_model);
  d. no case is vacuous: e_model of every weight block that passes through a bf16 product (W1x, W2x, W2h1) is at least
     five times the fp32 block bound, and so is e_model of Y_N and V_N against theirs;
  e. a reference with one product in nine left unrounded misses the criterion.  (One whose gradient differentiates the REVERSE
     sweep's rounded products instead of the tangent sweep's -- the kernels' backward runs through the stored tangent images --
     differs by 0.13 e_model on the (10, 24) case: inside the criterion, so the choice is made by reading gen_bwd2_kernel;)
  f. the table covers what it is there for.
"""
import pytest
import torch

import general_block_cases as gc
import ref64
import ref64_general as r64
from test_ref64_general import MIN_MARGIN, RELU_MARGIN

BLOCK_TOL, D_TOL, LOSS_TOL = 2e-4, 2e-5, 5e-5          # the fp32 bounds of tests/test_gpu_general_block_gradients.py
ALL = gc.BF16_CASES + gc.BF16_FULL_CASES
IDS = [c["id"] for c in ALL]
_THREE = {}


def three(c):
    """(exact, model, stand-in) on the oracle's draws of the case, each computed once."""
    if c["id"] not in _THREE:
        run = gc.runs(c)
        args = (c, run["oprob"], run["net"], run["trace"])
        back = "bf16" if c["mode"] == "bf16" else "autograd"
        _THREE[c["id"]] = (run["ref"], gc.bf16_reference(*args), r64.iteration(*args, operands="bf16", backward=back, dtype=torch.float32))
    return _THREE[c["id"]]


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_the_sweeps_with_exact_products_are_the_autograd_reference(c):
    run = gc.runs(c)
    exact, model, _ = three(c)
    sw = r64.iteration(c, run["oprob"], run["net"], run["trace"], operands="fp32", sweeps=True)
    ek, em = gc.bf16_errors(c, sw, exact, exact)
    assert max(ek["blocks"][1]) <= 1e-11 and all(ek[k] <= 1e-12 for k in ("YN", "VN", "XN", "tN", "loss")), ek
    ek, _ = gc.bf16_errors(c, model, exact, exact)
    assert min(ek["blocks"][1]) > 1e-5 and ek["YN"] > 1e-4 and ek["VN"] > 1e-4, ek
    # the kernels' backward, written out (kernel_backward), is the autograd gradient when nothing is rounded
    for operands, ref in (("fp32", exact), ("bf16", r64.iteration(c, run["oprob"], run["net"], run["trace"], operands="bf16"))):
        hand = r64.iteration(c, run["oprob"], run["net"], run["trace"], operands=operands, sweeps=True, backward="fp32")
        lay, kw = gc.layout(c)
        assert max(gc.general_block_errors(hand["grad"], ref["grad"], *lay, **kw)[1]) <= 1e-11


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_cases_satisfy_the_conditions_and_keep_their_discrete_results(c):
    ref, model, standin = three(c)
    lay, kw = gc.layout(c)
    names, blocks = gc.general_grad_blocks(ref["grad"], *lay, **kw)
    _, dom = gc.general_grad_blocks(ref["grad_domain"], *lay, **kw)
    gmax = float(ref["grad"].abs().max())
    share = {n: float(b.abs().max()) / gmax for n, b in zip(names, blocks)}
    domain = {n: float(q.abs().max()) / float(b.abs().max()) for n, b, q in zip(names, blocks, dom)}
    m, ts = ref["margins"], ref["tile_steps"]
    print("%s: smallest block %.2e (%s)  smallest domain part %.2f (%s)  margins exit %.1e time %.1e relu %.1e  K_count %d" %
          (c["id"], min(share.values()), min(share, key=share.get), min(domain.values()), min(domain, key=domain.get), m["exit"],
           m["time"], m["relu"], ref["K_count"]))
    assert all(v >= gc.BLOCK_FLOOR for v in share.values()), share
    assert all(v >= 0.5 for v in domain.values()), domain
    assert m["exit"] >= MIN_MARGIN and m["time"] >= MIN_MARGIN and m["relu"] >= RELU_MARGIN, m
    assert ref["K_count"] > 0
    if c["early"]:
        assert int(ts.min()) < int(ts.max()) or ref["n_loop"] < c["solver"]["N"], ts
    for other in (model, standin):
        assert torch.equal(other["steps"], ref["steps"]) and other["K_count"] == ref["K_count"]


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_the_fp32_stand_in_passes_the_gpu_criterion_with_half_the_margin(c):
    exact, model, standin = three(c)
    gc.assert_bf16(c, standin, model, exact, gc.BF16_C / 2, D_TOL, LOSS_TOL, BLOCK_TOL, tag=c["id"])


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_no_case_is_vacuous(c):
    exact, model, _ = three(c)
    _, em = gc.bf16_errors(c, model, model, exact)
    e = dict(zip(*em["blocks"]))
    print("%s: e_model YN %.2e VN %.2e XN %.2e  %s" % (c["id"], em["YN"], em["VN"], em["XN"], "  ".join("%s %.2e" % x for x in e.items())))
    assert all(e[n] >= 5 * BLOCK_TOL for n in gc.BF16_PRODUCT_BLOCKS), e
    assert em["YN"] >= 5 * D_TOL and em["VN"] >= 5 * D_TOL, em
    if c["solver"]["adaptive_forward_process"]:
        assert em["XN"] > 0.0, em["XN"]                                    # the bf16 products move the state
    else:
        assert em["XN"] == 0.0 and em["tN"] == 0.0


def test_a_reference_with_a_product_left_unrounded_misses_the_criterion(monkeypatch):
    c = gc.BF16_CASES[1]
    run = gc.runs(c)
    exact, model, _ = three(c)
    args = (c, run["oprob"], run["net"], run["trace"])
    judge = lambda wrong, tag: gc.assert_bf16(c, wrong, model, exact, gc.BF16_C, D_TOL, LOSS_TOL, BLOCK_TOL, tag=tag)
    # one product in nine left unrounded
    calls = [0]
    keep = ref64.product

    def product(a, W, operands="fp32"):
        calls[0] += 1
        return keep(a, W, "fp32" if calls[0] % 9 == 1 else operands)
    monkeypatch.setattr(r64, "product", product)
    with pytest.raises(AssertionError):
        judge(r64.iteration(*args, operands="bf16"), "one product in nine unrounded")


def test_the_table_covers_what_it_is_there_for():
    full = gc.BF16_FULL_CASES
    assert all(c["mode"] == "bf16" and c["route"]["mode"] == "bf16" for c in full) and len(full) == len(gc.BF16_CASES) + 1
    assert any(c["solver"]["K"] % 16 and (c["solver"]["N"] + 1) * -(-c["solver"]["K"] // 16) >= 256 for c in full)   # rounds, ragged tail
    cs = gc.BF16_CASES
    assert all(c["mode"] == "bf16_fwd" and c["route"]["mode"] == "bf16_fwd" and c["route"]["plan"] == "gen" for c in cs)
    assert all(c["solver"]["K"] <= 300 and c["solver"]["N"] <= 20 for c in cs)
    sup = {c["route"]["inst"] for c in cs if c["noise"] == "reference"}
    assert {(6, 30), (10, 24), (10, 32), (16, 16), (48, 48)} <= sup          # the three that overran, equal images, odd block counts
    phx = [c for c in cs if c["noise"] == "philox"]
    assert {c["route"]["spec"] for c in phx if c["route"]["inst"] == (100, 64)} == {gc.SPEC_ALLEN_CAHN, gc.SPEC_DWELL}
    assert any(c["solver"]["adaptive_forward_process"] and c["route"]["spec"] is None for c in phx)
    assert any(c["family"] == "general_bounded" and c["early"] for c in phx)
    d_of = lambda c: c["problem"]["kwargs"]["d"]
    assert any((d_of(c), c["net"]["arch"][0]) != c["route"]["inst"] for c in cs) and any((d_of(c), c["net"]["arch"][0]) == c["route"]["inst"] for c in cs)
    assert any(c["solver"]["K"] % 16 for c in cs) and any(c["solver"]["K"] > 256 for c in cs)
    moved = [gc.bf16_errors(c, three(c)[1], three(c)[1], three(c)[0])[1]["XN"] for c in cs if c["solver"]["adaptive_forward_process"]]
    assert max(moved) >= 5 * D_TOL, moved                                  # a state that the bf16 products move measurably
