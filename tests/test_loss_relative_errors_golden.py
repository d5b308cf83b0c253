"""utilities.loss_relative_errors, composite plan, against the reference notebook's own cell.

tests/golden/loss_relerr_d{1,3,5}.json were produced once, outside the repository, by running the third cell of the reference's
`experiments/HJB-log-variance-loss/Compare relative errors of losses.ipynb` (with the notebook's LLGC class of its second cell and
the reference's DenseNet) with these changes only: d restricted to the file's d, K = 64, delta_t_np = 0.125, random.seed and
torch.manual_seed fixed, the problem seed fixed (4200 + d), and two more appends per d -- the cell's final Y and g(X).  Each file
holds the seeds, d, K, N, the per-trajectory Y and g and the ten numbers the cell appends.

The cell draws randn(K, d) per step after LLGC (which seeds the generator) and the DenseNet (which seeds it again, with 42) were
built; noise='reference' with seed=None continues the generator from there, so the composite plan redraws the same noise."""
import numpy as np
import pytest
import torch

from conftest import has_gpu, load_golden
from util_cases import psp

U = psp.utilities
DIMS = (1, 3, 5)


def run_on_golden(d, device, backend):
    gold = load_golden("loss_relerr_d%d" % d)
    assert gold["d"] == d and gold["K"] == 64 and gold["N"] == 8
    problem = psp.LLGC(d=d, off_diag=gold["off_diag"], T=gold["T"], seed=gold["seeds"]["problem"], device=device)
    net = psp.DenseNet(d_in=d + 1, d_out=d, lr=gold["lr"]).to(device)          # seeds the generator with 42, as the reference's
    out = U.loss_relative_errors(problem, net, gold["K"], delta_t=gold["delta_t"],
                                 adaptive_forward_process=gold["adaptive_forward_process"], noise="reference", seed=None,
                                 device=device, backend=backend, return_samples=True)
    return gold, out


def per_trajectory_gaps(gold, out):
    Y = out["Y"].double().cpu().numpy()
    g = Y - out["D"].double().cpu().numpy()
    Yr, gr = np.array(gold["Y"]), np.array(gold["g"])
    return (np.abs(Y - Yr).max() / max(1.0, np.abs(Yr).max()), np.abs(g - gr).max() / max(1.0, np.abs(gr).max()))


@pytest.mark.parametrize("d", DIMS)
def test_composite_plan_redraws_the_cell(d):
    """Per trajectory: Y and g = Y - D against the cell's to 1e-6 max(1, max|.|) (fp32 torch ops on both sides, the update on
    different code paths).  Statistics: within 1e-5 relative of the cell's fp32-reduced numbers (64-term torch reductions; this
    side sums in float64).  Measured on the CPU: per-trajectory gaps 0 .. 6e-8, statistics 2e-7 at most."""
    gold, out = run_on_golden(d, "cpu", "auto")
    assert out["plan"] == "torch" and out["K"] == 64 and out["N"] == 8
    gy, gg = per_trajectory_gaps(gold, out)
    print("d=%d per-trajectory gaps: Y %.3g  g %.3g" % (d, gy, gg))
    assert gy <= 1e-6 and gg <= 1e-6
    a = gold["appended"]
    sel = out["cross_entropy_detach_selection"]
    pairs = [("var_g", out["terminal"][1]), ("mean_g", out["terminal"][0]),
             ("var_CE", out["cross_entropy"][1]), ("mean_CE", out["cross_entropy"][0]),
             ("var_CE_detach", out["cross_entropy_detach"][1]), ("mean_CE_detach", out["cross_entropy_detach"][0]),
             ("var_CE_detach_selection", np.sqrt(sel[1])), ("mean_CE_detach_selection", abs(sel[0])),    # the cell's own two forms
             ("var_var", out["log_variance"][1]), ("mean_var", out["log_variance"][0])]
    worst = 0.0
    for name, got in pairs:
        rel = abs(got - a[name]) / abs(a[name])
        worst = max(worst, rel)
        print("d=%d %-26s got %.9g  cell %.9g  rel %.2e" % (d, name, got, a[name], rel))
    assert worst <= 1e-5
    assert sel[3] == 64                                                        # nothing reaches 100 at these sizes
    for key in U.LRE_KEYS:                                                     # relative_error is sqrt(variance) / |mean|
        m, v, r = out[key][:3]
        assert r == pytest.approx(np.sqrt(v) / abs(m), rel=1e-14)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_native_plan_on_the_cells_draws(d):
    """The GPU twin: the native plan on the same draws under the forward kernels' parity bar, max|delta| <= 1e-4 max(1, max|ref|)
    (measured on an MI355X: Y within 1.7e-7, g within 2.3e-7)."""
    assert has_gpu()
    gold, out = run_on_golden(d, torch.device("cuda:0"), "native")
    assert out["plan"] == "native"
    gy, gg = per_trajectory_gaps(gold, out)
    print("d=%d native per-trajectory gaps: Y %.3g  g %.3g" % (d, gy, gg))
    assert gy <= 1e-4 and gg <= 1e-4
