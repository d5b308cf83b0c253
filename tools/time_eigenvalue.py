"""Time of one EigenvalueSolver iteration two ways on the same GPU, alternating in one process: the native plan
(plan_eigen_native.py: psp_genl_rollout_fwd_eig, psp_genl_rollout_bwd, psp_adam_step, the boundary and normalisation terms by torch
autograd) and the composite torch plan (eigenvalue_solver.py: the notebooks' op sequence on autograd).

Shapes: the notebooks' -- d = 5 and 10, K = 500, N = 20, K_boundary = 50, delta_t = 0.001 -- for the Fokker-Planck problem with its
relu^2 net [10] * 4 ('center' normalisation) and for the Schroedinger problem with the d = 5 notebook's tanh net and the d = 10
notebook's relu^2 net [15] * 4 ('l2' normalisation, K more points in the torch-side terms).  noise='reference', the V_L2 diagnostic
on, as the notebooks run.  Five warm-up iterations, then twenty timed ones per plan (host clock, a device synchronise before and
after each), native and composite taking turns; the median is reported, with the share of the native iteration spent in the
torch-side boundary and normalisation terms (timed inside the plan, synchronised).  Nothing is gated on these numbers.

    python tools/time_eigenvalue.py [--json profiles/eigenvalue_timing.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import path_space_pde_solver_amd as psp  # noqa: E402

WARMUP, TIMED = 5, 20


def build(kind, d, dev, backend):
    if kind == "fokker_planck":
        pb = psp.FokkerPlanckEigenvalue(d=d, device=dev)
        model = psp.EigenvalueSolver(pb, kind, L=1, lambda_init=0.5, lambda_lr=0.01, normalisation="center", verbose=False,
                                     device=dev, backend=backend)
        return model                                              # the constructor's net is the notebook's
    pb = psp.SchroedingerEigenvalue(d=d, device=dev)
    model = psp.EigenvalueSolver(pb, kind, L=1, lambda_init=-2.0, lambda_lr=0.001, normalisation="l2", verbose=False, device=dev,
                                 backend=backend)
    if d == 5:
        model.V = psp.DenseNet_tanh(d, 1, lr=0.001, arch=[15] * 4, output_relu=True).to(dev)
    else:
        model.V = psp.DenseNet(d, 1, lr=0.001, arch=[15] * 4, output_relu=True, weight_scale=0.01, weight_shift=0.01,
                               bias_init=0.1).to(dev)
    return model


def one_iteration(model, plan):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if plan is None:
        model._train_composite()
    else:
        plan.train()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_eigenvalue.py needs the GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda:0")
    out = {"what": "one EigenvalueSolver iteration, K = 500, N = 20, K_boundary = 50, delta_t = 0.001, noise='reference'; median of "
                   "%d iterations after %d warm-ups, native and composite alternating in one process; one run on one GPU"
                   % (TIMED, WARMUP), "device": torch.cuda.get_device_name(0), "rows": []}
    for kind, d in (("fokker_planck", 5), ("fokker_planck", 10), ("schroedinger", 5), ("schroedinger", 10)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            native, composite = build(kind, d, dev, "native"), build(kind, d, dev, "torch")
            torch.manual_seed(42)
            np.random.seed(42)
            plan = native._choose_plan()
            assert native.plan_name == "native", native.plan_reason
            assert composite._choose_plan() is None
            times = {"native": [], "composite": []}
            for it in range(WARMUP + TIMED):
                if it == WARMUP:
                    plan.timing = []
                for name, model, p in (("native", native, plan), ("composite", composite, None)):
                    t = one_iteration(model, p)
                    if it >= WARMUP:
                        times[name].append(t)
        med = {k: 1e3 * sorted(v)[len(v) // 2] for k, v in times.items()}
        torch_ms = 1e3 * sorted(plan.timing)[len(plan.timing) // 2]
        row = {"problem": kind, "d": d, "net": type(native.V).__name__ + str(list(native.V.nn_dims[1:-1])),
               "native_median_ms": med["native"], "composite_median_ms": med["composite"],
               "composite_over_native": med["composite"] / med["native"], "native_torch_side_terms_median_ms": torch_ms,
               "native_torch_side_share": torch_ms / med["native"], "native_min_ms": 1e3 * min(times["native"]),
               "composite_min_ms": 1e3 * min(times["composite"])}
        out["rows"].append(row)
        print("%-14s d=%-2d native %.3f ms (torch-side terms %.3f ms = %.0f %%), composite %.3f ms: x%.1f"
              % (kind, d, med["native"], torch_ms, 100 * row["native_torch_side_share"], med["composite"], row["composite_over_native"]),
              flush=True)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
