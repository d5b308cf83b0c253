"""Goldens of Solver.train with a linear, affine or constant control per time step (time_approx='outer', z_n a list of
function_space.Linear / Affine / Constant -- the notebook `Ornstein-Uhlenbeck - quadratic costs - linear ansatz.ipynb`): the
reference's own Solver runs.  A separate script so that make_golden.py, index.json and the fixtures it writes stay as they are.

    python tests/golden/make_golden_affine.py [case names]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as mg  # noqa: E402

LQ10 = dict(kind="LQGC", kwargs=dict(d=10, off_diag=0.1, T=0.5, seed=42, delta_t=0.005))
NB = dict(L=6, lr=0.1, K=64, delta_t=0.01, time_approx="outer", adaptive_forward_process=True, seed=42)

CASES = [
    dict(name="lqgc_d10_linear_outer_logvar", problem=LQ10, control=dict(kind="Linear"),
         solver=dict(NB, loss_method="log-variance", detach_forward=True)),
    dict(name="lqgc_d10_linear_outer_moment_learn_y0", problem=LQ10, control=dict(kind="Linear"),
         solver=dict(NB, loss_method="moment", detach_forward=True, learn_Y_0=True)),
    dict(name="lqgc_d10_linear_outer_cross_entropy", problem=LQ10, control=dict(kind="Linear"),
         solver=dict(NB, loss_method="cross_entropy", detach_forward=True)),
    dict(name="lqgc_d10_linear_outer_relative_entropy_attached", problem=LQ10, control=dict(kind="Linear"),
         solver=dict(NB, loss_method="relative_entropy", detach_forward=False)),
    dict(name="lqgc_d5_linear_outer_relative_entropy_randx0",
         problem=dict(kind="LQGC", kwargs=dict(d=5, off_diag=0.1, T=0.5, seed=1142, delta_t=0.005)), control=dict(kind="Linear"),
         solver=dict(NB, loss_method="relative_entropy", detach_forward=False, random_X_0=True, K=37, seed=1142)),
    # Affine starts at zero in the reference; small non-zero A, b so that the first gradient sees the matrix
    dict(name="llgc_d20_affine_outer_attached_logvar",
         problem=dict(kind="LLGC", kwargs=dict(d=20, off_diag=0.05, T=0.2, seed=42)),
         control=dict(kind="Affine", init=dict(scale=0.1, seed0=100)),
         solver=dict(NB, loss_method="log-variance", detach_forward=False, K=50, delta_t=0.02)),
    dict(name="llgc_d3_constant_outer_nonadaptive",
         problem=dict(kind="LLGC", kwargs=dict(d=3, off_diag=0.05, T=0.5, seed=42)), control=dict(kind="Constant"),
         solver=dict(NB, loss_method="log-variance", adaptive_forward_process=False, detach_forward=True, K=37, delta_t=0.05)),
]


def build_modules(fs, control, d, N, lr, seed, device=None):
    """The list a notebook assigns to model.z_n: N modules of `fs`.<kind> (reference or this package's function_space)."""
    kind = control["kind"]
    mods = []
    for n in range(N):
        if kind == "Linear":
            eye = torch.eye(d) if device is None else torch.eye(d, device=device)
            m = fs.Linear(d=d, B=eye, Q=eye, lr=lr, seed=seed)
        elif kind == "Affine":
            m = fs.Affine(d=d, lr=lr, seed=seed)
        else:
            m = fs.Constant(d=d, lr=lr, seed=seed)
        init = control.get("init")
        if init is not None:
            g = torch.Generator().manual_seed(init["seed0"] + n)
            with torch.no_grad():
                for p in m.parameters():
                    p.copy_(init["scale"] * torch.randn(p.shape, generator=g))
        mods.append(m)
    return mods


def run_case(case):
    problem = mg.make_problem(case["problem"])
    skw = dict(case["solver"])
    model = mg.ref_sv.Solver(name=case["name"], problem=problem, verbose=False, **skw)
    model.z_n = build_modules(mg.ref_fs, case["control"], model.d, model.N, model.lr, skw["seed"])
    model.update_Phis()
    model.train()
    xp = mg.probe_points(problem.d)
    probes = []
    for n in sorted(set([0, model.N // 2, model.N - 1])):
        t = 0.0 if n == 0 else (n - 0.5) * skw["delta_t"]         # ceil(t / delta_t) = n whatever the rounding
        with torch.no_grad():
            z = model.Z_n(xp, torch.tensor(t))
        probes.append({"t": t, "step": n, "minus_Z": mg.f32list(-z)})
    return {"N": model.N, "loss_log": [float(v) for v in model.loss_log], "u_L2_loss": [float(v) for v in model.u_L2_loss],
            "Y_0_log": [float(v) for v in model.Y_0_log], "probe_x": mg.f32list(xp), "probes": probes}


def main():
    torch.set_num_threads(1)
    only = set(sys.argv[1:])
    for case in CASES:
        if only and case["name"] not in only:
            continue
        print("running", case["name"], flush=True)
        res = run_case(case)
        with open(os.path.join(HERE, case["name"] + ".json"), "w") as fh:
            json.dump({"case": case, "expected": res, "torch": torch.__version__}, fh, indent=1)
        print("   loss_log", res["loss_log"], "u_L2", res["u_L2_loss"], flush=True)


if __name__ == "__main__":
    main()
