"""The native gradients of the value-function ansatz with the state path attached (tests/test_gpu_value_attached.py: forward kernel,
the adjoint sweep of csrc/genl_adj_kernels.h, the backward kernel) block by block against the float64 gradient of
tests/ref64_value.py -- that file asserts the whole vector against the fp32 oracle at 5e-4 max |g| with the output bias cut off.

The blocks are those of tests/general_block_cases.py with the time input FIRST ([t, x], solver.py:336-339); each is held to
BLOCK_TOL = 2e-4 of its own maximum, floored at BLOCK_FLOOR = 1e-4 of the whole gradient's.

The output bias is not excluded.  Under the log-variance loss its gradient is zero analytically (the loss does not see a shift of V;
1e-15 .. 1e-19 of the maximum in float64), so the block is held to the floor.  2e-4 of the floor is 2e-8 of the whole gradient's
maximum, below what ANY fp32 sum of the K cancelling weights (2 / K)(D_k - mean D) times terms of the size of that maximum can
keep: one rounding of such a term is 1.2e-7 of it, 1.2e-3 in units of the floor.  The fp32 oracle on the CPU misses the figure
itself -- its output-bias error in units of the floor, measured with four threads: llgc_d8_off 5.6e-5, lqgc_d5 and lqgc_d5_ul2
1.4e-4, lqgc_d5_tanh 1.0e-4, lqgc_d20_wide 3.2e-4, lqgc_d5_one_step 4.2e-3 (the residue depends on the summation order, hence on
the CPU and its thread count: 0 on lqgc_d5 and 1.4e-2 on lqgc_d5_one_step also occur) -- so the bound of THAT block is four times that worst,
OUT_BIAS_TOL = 4 x 4.22e-3 = 1.7e-2 of the floor, i.e. 1.7e-6 of the whole gradient's maximum, fixed here from the CPU measurement
and not from the kernels' output.  Where the output bias carries a gradient (the moment loss) it is an ordinary block at 2e-4.
Measured on an MI355X: every other block within 1.1e-6; the output bias at the floor within 1.3e-3 (lqgc_d15_diag)."""
import pytest

import general_block_cases as gc
import value_attached_cases as vac
from test_gpu_value_attached import first_iteration

pytestmark = pytest.mark.gpu

BLOCK_TOL = 2e-4
OUT_BIAS_TOL = 4 * 4.22e-3  # the output bias where it is held to the floor (log-variance loss): see the module docstring


def layout(name):
    case = vac.CASES[name]
    return case["problem"]["kwargs"]["d"], True, list(case.get("net", {}).get("arch", [30, 30]))


@pytest.mark.parametrize("name", vac.NAMES)
def test_attached_gradient_blocks_match_float64(name):
    g, g_ref = first_iteration(name)["grad"], vac.ref64(name)["grad"]
    assert g.shape == g_ref.shape
    names, ref_blocks = gc.general_grad_blocks(g_ref, *layout(name), time_first=True)
    at_floor = float(ref_blocks[-1].abs().max()) < gc.BLOCK_FLOOR * float(g_ref.abs().max())
    bound_b = OUT_BIAS_TOL if at_floor else BLOCK_TOL
    names, errs = gc.general_block_errors(g, g_ref, *layout(name), time_first=True)
    print("%s blocks %s (<= %.3g; %s <= %.3g)" % (name, "  ".join("%s %.2e" % ne for ne in zip(names, errs)), BLOCK_TOL, names[-1], bound_b))
    bad = [(n, e) for n, e in zip(names[:-1], errs[:-1]) if not e <= BLOCK_TOL]
    assert not bad, (name, bad)
    assert errs[-1] <= bound_b, (name, names[-1], errs[-1], bound_b)
