"""Goldens of the gradient-variance diagnostic: the reference's own Solver(compute_gradient_variance=m), made with make_golden's
problems and its CUDA-to-CPU redirection.  A separate script so that make_golden.py, index.json and the fixtures it writes stay
as they are.  z_n is swapped for a list of DenseNet(arch=[8, 8]) (p = 150 at d = 2) to keep the files small.  Besides the logs,
the (N, p) matrix every get_gradient_variances call returned is recorded through a wrapper around the bound method; the two
configurations the reference fails on are recorded as exception type names.

    python tests/golden/make_golden_gradvar.py [case names]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as mg  # noqa: E402

OUTER = dict(time_approx="outer", early_stopping_time=None, u_l2_error_flag=False, lr=0.01, seed=42, K=16, L=3,
             compute_gradient_variance=1)
LLGC2 = dict(kind="LLGC", kwargs=dict(d=2, off_diag=0.1, T=0.2, seed=42))       # N = 4
NET = dict(kind="densenet_list", arch=[8, 8], seed=42)
REL_CUT, MAX_OUTLIER_SHARE = 30.0, 0.10

CASES = [
    dict(name="gradvar_llgc2_moment_nonadaptive", problem=LLGC2,
         solver=dict(OUTER, delta_t=0.05, loss_method="moment", adaptive_forward_process=False)),
    dict(name="gradvar_llgc2_moment_attached_learn_y0", problem=LLGC2,
         solver=dict(OUTER, delta_t=0.05, loss_method="moment", adaptive_forward_process=True, detach_forward=False,
                     learn_Y_0=True)),
    dict(name="gradvar_llgc2_logvar_nonadaptive", problem=LLGC2,
         solver=dict(OUTER, delta_t=0.05, loss_method="log-variance", adaptive_forward_process=False)),
    dict(name="gradvar_llgc2_logvar_default_flags", problem=LLGC2,            # adaptive, attached: the constructor defaults
         solver=dict(OUTER, delta_t=0.05, loss_method="log-variance")),
    dict(name="gradvar_lqgc3_logvar_attached_cadence",                        # m = 2 over L = 4: logged at l = 0 and l = 2
         problem=dict(kind="LQGC", kwargs=dict(d=3, off_diag=0.1, T=0.2, seed=42, delta_t=0.05)),
         solver=dict(OUTER, delta_t=0.05, loss_method="log-variance", adaptive_forward_process=True, detach_forward=False,
                     compute_gradient_variance=2, L=4)),
    # the two configurations the reference raises on
    dict(name="gradvar_llgc2_raises_detached", problem=LLGC2,
         solver=dict(OUTER, delta_t=0.05, loss_method="log-variance", adaptive_forward_process=True, detach_forward=True, L=1)),
    dict(name="gradvar_llgc2_raises_variance_loss", problem=LLGC2,
         solver=dict(OUTER, delta_t=0.05, loss_method="variance", adaptive_forward_process=False, L=1)),
]
for _c in CASES:
    _c["net"] = NET


def run_case(case):
    problem = mg.make_problem(case["problem"])
    skw = dict(case["solver"])
    model = mg.ref_sv.Solver(name=case["name"], problem=problem, verbose=False, **skw)
    net = case["net"]
    model.z_n = [mg.ref_fs.DenseNet(d_in=problem.d, d_out=problem.d, lr=skw["lr"], arch=net["arch"], seed=net["seed"])
                 for _ in range(model.N)]
    model.update_Phis()
    matrices = []
    bound = model.get_gradient_variances

    def recording(X, Y):
        rel = bound(X, Y)
        matrices.append(rel.detach().clone())
        return rel

    model.get_gradient_variances = recording
    try:
        model.train()
    except Exception as e:          # noqa: BLE001  (the type name IS the recorded result)
        return {"raises": type(e).__name__, "message": str(e)[:200]}
    share = [float((m.abs() > REL_CUT).double().mean()) for m in matrices]
    total = sum(float((m.abs() > REL_CUT).sum()) for m in matrices) / sum(m.numel() for m in matrices)
    assert total <= MAX_OUTLIER_SHARE, (case["name"], total, "pick another seed or K")
    return {"raises": None, "N": model.N, "p": int(model.p),
            "loss_log": [float(v) for v in model.loss_log],
            "Y_0_log": [float(v) for v in model.Y_0_log],
            "grads_rel_error_log": [float(v) for v in model.grads_rel_error_log],
            "rel_matrices": [[float(v) for v in m.reshape(-1).tolist()] for m in matrices],
            "outlier_share": share, "zero_share": [float((m == 0).double().mean()) for m in matrices]}


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
        print("  ", {k: v for k, v in res.items() if k != "rel_matrices"}, flush=True)


if __name__ == "__main__":
    main()
