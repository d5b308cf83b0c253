"""Goldens of the exit-time and box-domain problems (DoubleWell_stopping, DoubleWell_stopping_linear,
DoubleWell_expectation_hitting_time, QuadraticGradient, Helmholtz, Oscillations, SinNorm2): the reference's own EllipticSolver on
its own classes, on CPU through make_golden's proxy.  A separate script so that make_golden.py, index.json and the fixtures
they write stay as they are; the records have the layout of make_golden's elliptic cases plus ``min_exit_margin`` (the PINN
records the layout of make_golden_pinn's).

Exit-margin condition: a GPU rollout forms the state in another rounding order than torch does, and the exit test decides
K_log.  The script records how close the reference's own tests came to flipping and refuses a fixture below 1e-5:
  * sphere domains: min | |X_n| - r | over every (k, n >= 1) the reference tests (as make_golden_dense_sigma.py);
  * box domains: the test reads the PROPOSAL, so the recorder rebuilds it -- with the expression of solver.py:746-747, from
    the X and Z that problem.h receives and the xi of the last randn(K, d) -- and takes the distance of every coordinate of
    every proposal of a not yet stopped trajectory to the faces the test compares with.
A BSDE case whose run prints "Not all trajectories stopped" is refused: raise N.

    python tests/golden/make_golden_elliptic_catalogue.py [case names]
"""
import contextlib
import io
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as mg  # noqa: E402
import make_golden_pinn as mgp  # noqa: E402

MIN_MARGIN = 1e-5

REFSOL = [["compute_reference_solution", {}]]
D = dict(seed=42, delta_t=0.01, N=30, lr=0.001, L=3, K=64, K_boundary=20, loss_method="diffusion", K_test_log=100)
P = dict(seed=42, delta_t=0.01, N=10, lr=0.001, L=3, K=64, K_boundary=20, loss_method="PINN", alpha=[1.0, 1.0])

PROBLEMS = dict(
    dwstop=dict(kind="DoubleWell_stopping", kwargs=dict(d=1, beta=1), calls=REFSOL),
    dwstoplin=dict(kind="DoubleWell_stopping_linear", kwargs=dict(d=1, beta=1), calls=REFSOL),
    dwhit=dict(kind="DoubleWell_expectation_hitting_time", kwargs=dict(d=1, beta=1), calls=REFSOL),
    quadgrad=dict(kind="QuadraticGradient", kwargs=dict(d=3)),
    helmholtz=dict(kind="Helmholtz", kwargs=dict(d=2)),
    oscillations=dict(kind="Oscillations", kwargs=dict(d=1)),
)

CASES = [dict(name="cat_%s_diffusion" % k, family="elliptic", problem=p, solver=dict(D)) for k, p in PROBLEMS.items()] + [
    dict(name="cat_sinnorm2_lin_d4_diffusion", family="elliptic",
         problem=dict(kind="SinNorm2", kwargs=dict(d=4, linear=True)), solver=dict(D, N=20)),
    dict(name="cat_sinnorm2_nl_d4_diffusion", family="elliptic",
         problem=dict(kind="SinNorm2", kwargs=dict(d=4, linear=False, alpha=0.8)), solver=dict(D, N=20)),
    # BSDE: N large enough that every trajectory leaves the box
    dict(name="cat_helmholtz_bsde", family="elliptic", problem=PROBLEMS["helmholtz"],
         solver=dict(D, loss_method="BSDE", N=400)),
    dict(name="cat_oscillations_bsde", family="elliptic", problem=PROBLEMS["oscillations"],
         solver=dict(D, loss_method="BSDE", N=300)),
] + [dict(name="cat_%s_pinn" % k, family="elliptic", pinn=True, problem=p, solver=dict(P)) for k, p in PROBLEMS.items()]


def run_case(case):
    """make_golden.run_elliptic_case with the margin recorder around problem.h."""
    problem = mg.make_problem(case["problem"])
    model = mg.ref_sv.EllipticSolver(problem=problem, name=case["name"], verbose=False, **case["solver"])
    state = dict(iteration=-1, n=0, margin=float("inf"), xi=None, stopped=None)
    h_ref, box = problem.h, problem.boundary == "square"
    K, d = case["solver"]["K"], problem.d
    randn_ref = torch.randn

    def randn(*shape, **kw):
        out = randn_ref(*shape, **kw)
        if tuple(shape) == (K, d):
            state["xi"] = out
        return out

    def h(x, y, z):
        it = len(model.loss_log)
        if it != state["iteration"]:
            state["iteration"], state["n"], state["stopped"] = it, 0, torch.zeros(K, dtype=torch.bool)
        if box:
            X, xi, sel = x.detach(), state["xi"], ~state["stopped"]
            c = -z.detach().t() if model.adaptive_forward_process else torch.zeros(d, K)
            Xp = (X + ((problem.b(X) + torch.mm(problem.sigma(X), c).t()) * model.delta_t
                       + torch.mm(problem.sigma(X), xi.t()).t() * model.sq_delta_t) * sel.float().unsqueeze(1).repeat(1, d))
            dist = torch.abs(Xp.double() - problem.X_r)
            inside = torch.all(Xp <= problem.X_r, 1)
            if not problem.one_boundary:
                dist = torch.minimum(dist, torch.abs(Xp.double() - problem.X_l))
                inside = torch.all((Xp >= problem.X_l) & (Xp <= problem.X_r), 1)
            if bool(sel.any()):
                state["margin"] = min(state["margin"], float(torch.min(dist[sel])))
            state["stopped"] = state["stopped"] | ~inside
        elif state["n"] >= 1:
            r = torch.sqrt(torch.sum(x.detach().double() ** 2, 1))
            state["margin"] = min(state["margin"], float(torch.min(torch.abs(r - problem.boundary_distance))))
        state["n"] += 1
        return h_ref(x, y, z)

    problem.h = h
    mg._proxy.randn = randn
    init_fp = mg.param_fingerprint(model.V)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            model.train()
    finally:
        del mg._proxy.randn
    if "Not all trajectories stopped" in buf.getvalue():
        raise RuntimeError("%s: N is too small, not every trajectory left the domain" % case["name"])
    xp = 0.4 * mg.probe_points(problem.d)
    with torch.no_grad():
        v = model.V(xp).squeeze()
    return {
        "loss_log": [float(v_) for v_ in model.loss_log],
        "K_log": [int(v_) for v_ in model.K_log],
        "V_L2_log": [float(v_) for v_ in model.V_L2_log],
        "V_test_L2": [float(v_) for v_ in model.V_test_L2], "V_test_abs": [float(v_) for v_ in model.V_test_abs],
        "init_params": init_fp, "final_params": mg.param_fingerprint(model.V),
        "probe_x": mg.f32list(xp), "probe_V": mg.f32list(v),
        "min_exit_margin": state["margin"],
    }


def main():
    torch.set_num_threads(1)
    warnings.filterwarnings("ignore")
    only = set(sys.argv[1:])
    for case in CASES:
        if only and case["name"] not in only:
            continue
        print("running", case["name"], flush=True)
        if case.get("pinn"):
            res = mgp.run_case(case)
        else:
            res = run_case(case)
            print("  K_log", res["K_log"], "min_exit_margin %.3e" % res["min_exit_margin"], flush=True)
            if not res["min_exit_margin"] >= MIN_MARGIN:
                raise RuntimeError("%s: exit margin %.3e below %.0e -- take the next seed"
                                   % (case["name"], res["min_exit_margin"], MIN_MARGIN))
        print("  loss_log", res["loss_log"], flush=True)
        with open(os.path.join(HERE, case["name"] + ".json"), "w") as fh:
            json.dump({"case": case, "expected": res, "torch": torch.__version__}, fh, indent=1)


if __name__ == "__main__":
    main()
