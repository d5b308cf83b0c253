"""Shared by the gradient-variance tests: the golden cases of tests/golden/make_golden_gradvar.py, the package solver of one of
them (z_n swapped for a list of DenseNets, as the generator does with the reference's), and the comparison of a rel matrix
with a recorded one."""
import torch

from util_cases import flat_params, make_pkg_problem, psp

RUN_CASES = ["gradvar_llgc2_moment_nonadaptive", "gradvar_llgc2_moment_attached_learn_y0", "gradvar_llgc2_logvar_nonadaptive",
             "gradvar_llgc2_logvar_default_flags", "gradvar_lqgc3_logvar_attached_cadence"]
RAISE_CASES = ["gradvar_llgc2_raises_detached", "gradvar_llgc2_raises_variance_loss"]
REL_CUT = 30.0            # entries with golden |rel| above this (|mean| << sqrt(var)) are left out of the comparison ...
MAX_LEFT_OUT = 0.15       # ... and their share of all entries is capped


def make_gradvar_solver(case, device, **over):
    prob = make_pkg_problem(case["problem"], device)
    kw = dict(case["solver"])
    kw.update(over)
    model = psp.Solver(name=case["name"], problem=prob, verbose=False, device=device, **kw)
    net = case["net"]
    model.z_n = [psp.DenseNet(d_in=prob.d, d_out=prob.d, lr=kw["lr"], arch=net["arch"], seed=net["seed"]) for _ in range(model.N)]
    model.update_Phis()
    return model


def record_matrices(model):
    """Wraps the bound get_gradient_variances so that every matrix it returns is kept; returns the list."""
    out = []
    bound = model.get_gradient_variances

    def recording(X, Y):
        rel = bound(X, Y)
        out.append(rel.detach().cpu().clone())
        return rel

    model.get_gradient_variances = recording
    return out


def compare_rel(got, want, rel_tol):
    """got, want: (N, p) rel matrices.  Exact zeros where the golden is 0, rel_tol on entries with golden |rel| <= REL_CUT, the
    share of entries left out <= MAX_LEFT_OUT.  Returns (worst relative error over the compared entries, share left out)."""
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    assert got.shape == want.shape
    zero = want == 0
    assert bool((got[zero] == 0).all()), "entries that are exactly 0 in the golden"
    keep = (~zero) & (want.abs() <= REL_CUT)
    left_out = float((~zero & ~keep).double().mean())
    assert left_out <= MAX_LEFT_OUT, left_out
    err = ((got[keep] - want[keep]).abs() / want[keep].abs())
    worst = float(err.max()) if err.numel() else 0.0
    assert worst <= rel_tol, (worst, rel_tol)
    return worst, left_out


# ---- float64-reference cases (tests/ref64_gradvar.py): the regime of tests/dense_block_cases.py, time_approx='outer', LLGC ----------
import dense_block_cases as dc  # noqa: E402

# (d, H, K, N, instance): ragged last tile with padded d and H; two slices; the two column passes; several slices of more than four
# tiles (more than one round); N = 1 rides along on the first shape
KERNEL_SHAPES = [(12, 16, 37, 4, (16, 32)), (20, 40, 80, 3, (32, 64)), (70, 40, 48, 3, (112, 64)), (20, 30, 9001, 4, (32, 32)),
                 (12, 16, 37, 1, (16, 32))]
PLAN_SHAPES = KERNEL_SHAPES[:3]


def block_case(d, H, K, N, expect, loss="moment", adaptive=False, mode="fp32"):
    """A dense_block_cases case of the shape: non-adaptive, or adaptive with gradients through the state path (attached)."""
    bwd = "kernel2" if expect == (112, 64) else "kernel1"
    return dc._c("outer", "LLGC", d, H, K, N, not adaptive, mode, expect, bwd, loss=loss, adaptive=adaptive,
                 slices_gt1=K > 1000)


def variance_blocks_alive(var, d, H, N):
    """Every one of the 9 blocks of every set has non-zero grads_var."""
    from util_cases import dense_grad_blocks
    return all(float(b.abs().max()) > 0.0 for blocks in dense_grad_blocks(var.reshape(-1), d, H, N, False) for b in blocks)


def forward_once(c, device, lr=0.0, **over):
    """One iteration of the case on the native plan; lr = 0 leaves the parameters as they were.  (model, plan, oracle problem,
    oracle config, oracle nets)."""
    case = dc.golden_style(c)
    case["solver"].update(lr=lr, **over)
    oprob, ocfg, onets = dc.scaled_oracle(c)
    prob = make_pkg_problem(case["problem"], device)
    prob.X_0 = dc.x0_of(c, prob.X_0).to(device)
    model = psp.Solver(name=case["name"], problem=prob, verbose=False, device=device, backend="native", noise="reference",
                       mlp_dtype=c["mode"], **case["solver"])
    nets = [psp.DenseNet(d_in=d_in, d_out=c["d"], lr=lr, arch=[c["H"], c["H"]], seed=seed).to(device) for d_in, seed in dc.net_specs(c)]
    dc.prepare_nets(c, nets)
    model.z_n = nets
    model.update_Phis()
    model.train()
    torch.cuda.synchronize()
    plan = model._native_plan
    assert model.plan_name == "native" and isinstance(plan, psp.plan_dense_native.DenseNativePlan)
    assert (plan.d_pad, plan.H_pad) == c["expect"] and plan.kernel_bwd
    if lr == 0.0:
        assert torch.equal(plan.flat.cpu(), torch.cat([flat_params(n) for n in onets]))
    return model, plan, oprob, ocfg, onets
