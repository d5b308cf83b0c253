"""The cases of the attached value-function ansatz (adaptive_forward_process=True, detach_forward=False) shared by
test_ref64_value.py (CPU) and test_gpu_value_attached.py (GPU), with the builders of both sides and the float64 reference of
ref64_value.py computed once per case.

``scale`` multiplies every parameter of the value net -- the oracle's and the package's, built from the same seed -- where the
nets at initialisation would leave the attached and the detached gradient less than (or barely) 1e-2 of max|g| apart (measured
at initialisation: LLGC d = 17 1.0e-2, the double well 3.9e-3; LLGC losses overflow at 2, hence 1.25 there).  The GPU gradient
bound is 5e-4: a plan that silently ran the detached path must not pass."""
import copy
import functools

import torch

import ref64_value as r64
from util_cases import make_pkg_problem, orc, psp

VF = dict(approx_method="value_function", time_approx="inner", u_l2_error_flag=False, early_stopping_time=None, seed=42, L=3,
          lr=0.005, adaptive_forward_process=True, detach_forward=False)
LQ5 = dict(kind="LQGC", kwargs=dict(d=5, off_diag=0.1, T=0.5, seed=42, delta_t=0.05))
CASES = {
    # dense A and B, ragged last tile
    "llgc_d8_off": dict(problem=dict(kind="LLGC", kwargs=dict(d=8, off_diag=0.1, T=0.4, seed=42)),
                        solver=dict(VF, loss_method="log-variance", delta_t=0.02, K=40)),
    # the time input falls in the second input block
    "llgc_d17_off_moment": dict(problem=dict(kind="LLGC", kwargs=dict(d=17, off_diag=0.1, T=0.3, seed=42)),
                                solver=dict(VF, loss_method="moment", delta_t=0.02, K=40), scale=1.25),
    # the running cost at the moved state
    "lqgc_d5": dict(problem=LQ5, solver=dict(VF, loss_method="log-variance", delta_t=0.05, K=40)),
    # three layers; the state fills block 0 exactly
    "lqgc_d16_arch3_moment": dict(problem=dict(kind="LQGC", kwargs=dict(d=16, off_diag=0.05, T=0.3, seed=42, delta_t=0.05)),
                                  solver=dict(VF, loss_method="moment", delta_t=0.05, K=40), net=dict(arch=[20, 16, 12], seed=7)),
    # sigma = I and a diagonal drift through the dense path
    "lqgc_d15_diag": dict(problem=dict(kind="LQGC", kwargs=dict(d=15, off_diag=0.0, T=0.3, seed=42, delta_t=0.05)),
                          solver=dict(VF, loss_method="log-variance", delta_t=0.05, K=24)),
    # sigma = s I, element-wise drift Jacobian, no coefficients struct
    "dwell_d10": dict(problem=dict(kind="DoubleWell_multidim", kwargs=dict(d=10, d_1=5, d_2=5, T=0.3, eta=0.5, kappa=2.0)),
                      solver=dict(VF, loss_method="log-variance", delta_t=0.02, K=40), scale=2.0),
    # enough hidden blocks for the eight-wave instance
    "lqgc_d20_wide": dict(problem=dict(kind="LQGC", kwargs=dict(d=20, off_diag=0.1, T=0.3, seed=42, delta_t=0.05)),
                          solver=dict(VF, loss_method="log-variance", delta_t=0.05, K=24), net=dict(arch=[48, 48, 40], seed=7)),
    # another phi_2
    "lqgc_d5_tanh": dict(problem=LQ5, solver=dict(VF, loss_method="log-variance", delta_t=0.05, K=40),
                         net=dict(arch=[30, 30], seed=7, activation="tanh")),
    # N = 1: no residual terms, one step
    "lqgc_d5_one_step": dict(problem=dict(kind="LQGC", kwargs=dict(d=5, off_diag=0.1, T=0.05, seed=42, delta_t=0.05)),
                             solver=dict(VF, loss_method="log-variance", delta_t=0.05, K=40)),
    # the log instances together with the sweep
    "lqgc_d5_ul2": dict(problem=LQ5, solver=dict(VF, loss_method="log-variance", delta_t=0.05, K=40, u_l2_error_flag=True)),
}
for _name, _case in CASES.items():
    _case.update(name=_name)
NAMES = list(CASES)
# the three shapes shared with test_gpu_value_function_lq.py
SHARED = ["llgc_d8_off", "lqgc_d5", "lqgc_d15_diag"]


def _scale(net, s):
    if s != 1.0:
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(s)


def make_oracle(name, detach=False):
    """(problem, config, models) of the CPU oracle for a case; detach=True: the same case with the state path detached."""
    case = CASES[name]
    prob = orc.make_problem(case["problem"]["kind"], **case["problem"]["kwargs"])
    s = case["solver"]
    cfg = orc.HJBConfig(K=s["K"], delta_t=s["delta_t"], lr=s["lr"], L=s["L"], seed=s["seed"], loss_method=s["loss_method"],
                        time_approx="inner", learn_Y_0=False, adaptive_forward_process=True, detach_forward=detach,
                        random_X_0=False, approx_method="value_function")
    z, y0, N = orc.hjb_build(prob, cfg)
    net = case.get("net")
    if net is not None:
        z = orc.DenseNetOracle(prob.d + 1, 1, cfg.lr, arch=net["arch"], seed=net["seed"], activation=net.get("activation", "relu2"))
    _scale(z, case.get("scale", 1.0))
    return prob, cfg, (z, y0, N)


def make_pkg(name, device, backend="native", noise="reference", **over):
    """The package's Solver for a case, value_state_path='native' unless overridden."""
    case = copy.deepcopy(CASES[name])
    prob = make_pkg_problem(case["problem"], device)
    kw = dict(case["solver"], value_state_path="native")
    kw.update(over)
    model = psp.Solver(name=name, problem=prob, verbose=False, device=device, backend=backend, noise=noise, **kw)
    net = case.get("net")
    if net is not None:
        extra = dict(activation=net["activation"]) if "activation" in net else {}
        model.y_n = [psp.DenseNet(d_in=prob.d + 1, d_out=1, lr=kw["lr"], arch=net["arch"], seed=net["seed"], **extra).to(device)]
        model.update_Phis()
    _scale(model.y_n[0], case.get("scale", 1.0))
    return model


def first_noise(name):
    """The first iteration's noise in the reference's order (solver.py:422, 381)."""
    prob, cfg, (z, y0, N) = make_oracle(name)
    torch.manual_seed(cfg.seed)
    return torch.randn(cfg.K, prob.d, N + 1)


@functools.lru_cache(maxsize=None)
def ref64(name):
    """The float64 sweep restatement of a case's first iteration (ref64_value.sweep_iteration), computed once."""
    prob, cfg, (z, y0, N) = make_oracle(name)
    params, act = r64.net64(z)
    return r64.sweep_iteration(r64.coeffs64(prob), params, act, first_noise(name), cfg.delta_t, N, cfg.loss_method)


@functools.lru_cache(maxsize=None)
def ref64_autograd(name):
    prob, cfg, (z, y0, N) = make_oracle(name)
    params, act = r64.net64(z)
    return r64.autograd_iteration(r64.coeffs64(prob), params, act, first_noise(name), cfg.delta_t, N, cfg.loss_method)


@functools.lru_cache(maxsize=None)
def oracle(name, detach=False):
    """One fp32 oracle run per case (L = 3, traced): (loss log, first-iteration gradient)."""
    torch.set_num_threads(4)
    prob, cfg, models = make_oracle(name, detach=detach)
    ref = orc.hjb_train(prob, cfg, step_models=models, trace=True)
    g = torch.cat([g.reshape(-1) for g in ref["traces"][0]["grads"]])
    return tuple(ref["loss_log"]), g
