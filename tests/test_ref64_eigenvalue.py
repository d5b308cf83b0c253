"""The float64 restatement of EigenvalueSolver's iteration (tests/ref64_eigenvalue.py) against the fp32 composite plan on the same
draws, over the cases of tests/eigen_kernel_cases.py: loss parts, parameter gradient per block, dLoss/dlambda; the conditions under
which the GPU test's discrete results are well defined; the planted error the per-block bound must catch.

dLoss/dlambda is a scalar, alpha[0] (2 / K) sum_k D_k S_k with terms of both signs, so its error is measured against the sum of
the absolute terms, sum_k |w_k S_k|.  The fp32 composite plan's worst error over the cases, measured here on the CPU, is
DLAM_FP32_ERR below; the GPU test allows four times that (the margin this project uses where only a scalar is compared)."""
import copy

import pytest
import torch

import eigen_kernel_cases as ec
import ref64_eigenvalue as r64
from general_block_cases import assert_general_blocks, general_block_errors

# worst |dlam_fp32 - dlam_f64| / sum_k |w_k S_k| of the fp32 composite plan over ec.CASES, measured by
# test_composite_matches_float64 on an x86 CPU build of torch (it prints every case's figure): 1.11e-5 (fp-d5-K48-relu10-init;
# D_k = V(X_N) - V(X_0) - Y is a difference of O(1) numbers that is O(1e-2) itself, so fp32 leaves it ~1e-5 relative), the other
# ten cases between 2.9e-8 and 7.7e-6.  Rounded up to two digits.
DLAM_FP32_ERR = 1.2e-5
BLOCK_TOL = 2e-4
PART_TOL = 5e-5


def composite(c):
    """(loss, parts, flat gradient, dLoss/dlambda) of the fp32 composite plan on the case's draws."""
    run = ec.runs(c)
    V = copy.deepcopy(run["V"])
    pb, model = ec.solver(c, V, backend="torch")
    torch.manual_seed(c["seed"])
    import numpy as np
    np.random.seed(c["seed"])
    loss, parts = model.composite_iteration()
    params = list(V.parameters())
    gs = torch.autograd.grad(loss, params + [model.lambda_.Y_0], allow_unused=True)
    g = torch.cat([(gi if gi is not None else torch.zeros_like(p)).reshape(-1) for gi, p in zip(gs[:-1], params)])
    return model, loss.item(), parts, g, float(gs[-1])


@pytest.mark.parametrize("c", ec.CASES, ids=[c["id"] for c in ec.CASES])
def test_composite_matches_float64(c):
    torch.set_num_threads(1)
    run = ec.runs(c)
    full = run["full"]
    model, loss, parts, g, dlam = composite(c)
    assert parts["K_count"] == full["K_count"]
    scale = model.center_scale
    got = dict(center=parts["center"].item(), boundary=parts["boundary"].item(),
               derivative_boundary=parts["derivative_boundary"].item(), domain=parts["domain"].item())
    for k, v in got.items():
        want = full["parts"][k]
        assert abs(v - want) <= PART_TOL * max(abs(want), 1e-6), (k, v, want)
    assert abs(loss - full["loss"]) <= PART_TOL * abs(full["loss"]), (loss, full["loss"], scale)
    assert abs(parts["V_L2"] - full["V_L2"]) <= 1e-4 * abs(full["V_L2"]) + 1e-12
    lay, kw = ec.layout(c)
    assert_general_blocks(g, full["grad"], lay, BLOCK_TOL, tag=c["id"], **kw)
    e = abs(dlam - full["dlam"]) / full["dlam_scale"]
    print("%s: dLoss/dlambda fp32 %.9e float64 %.9e, error %.2e of sum |w_k S_k| = %.3e" % (c["id"], dlam, full["dlam"], e, full["dlam_scale"]))
    assert e <= DLAM_FP32_ERR, e


@pytest.mark.parametrize("c", ec.CASES, ids=[c["id"] for c in ec.CASES])
def test_conditions_of_the_gpu_test(c):
    """Asserted on the reference alone: the margins, the share of closed gates, exits where delta_t = 0.05."""
    ref = ec.runs(c)["ref"]
    assert ref["margins"]["exit"] >= ec.MIN_MARGIN, ref["margins"]
    assert ref["margins"]["gate"] >= ec.MIN_MARGIN, ref["margins"]
    if c["gate"] == "drawn":
        assert 0.2 <= ref["closed_share"] <= 0.8, ref["closed_share"]
    if c["dt"] == 0.05 and c["d"] == 2:
        assert 0.25 <= ref["stopped_share"] <= 0.75, ref["stopped_share"]
    if c["dt"] == 0.05:
        assert ref["stopped_share"] > 0 and int(ref["tile_steps"].min()) >= 1
    # dLoss/dlambda from S_k, as the native plan forms it
    w = (2.0 * ec.ALPHA[0] / c["K"]) * ref["D"]
    assert abs(float((w * ref["S"]).sum()) - ref["dlam"]) <= 1e-12 * ref["dlam_scale"] + 1e-300
    # the kernels' part of every gradient block carries weight
    assert float(ref["grad_domain"].abs().max()) > 0


@pytest.mark.parametrize("c", ec.GATED, ids=[c["id"] for c in ec.GATED])
def test_planted_open_tangent_gate_fails_the_block_bound(c):
    """A gate left open on the tangent (Z = s grad o) but closed on the value (V = relu(o)) must not pass the per-block bound."""
    run = ec.runs(c)
    bad = r64.iteration(plant="open_tangent_gate", **run["kw"])
    lay, kw = ec.layout(c)
    names, errs = general_block_errors(bad["grad_domain"], run["ref"]["grad_domain"], *lay, **kw)
    print("%s: planted error, worst block %.2e (%s), end points %.2e" % (c["id"], max(errs), names[errs.index(max(errs))],
                                                                        float((bad["YN"] - run["ref"]["YN"]).abs().max())))
    assert max(errs) > BLOCK_TOL, (c["id"], max(errs))
    assert float((bad["YN"] - run["ref"]["YN"]).abs().max()) > 2e-5
