"""Per-iteration time of train_PINN() with an h that reads t, two ways on the same GPU in one process: the native plan with the
pair kernel (GeneralSolver(pinn_time_h='native'): psp_pinn_pairs_residual / _reduce / _backward, csrc/pinn_kernels.h) and the
composite torch plan (backend='torch': d + 1 autograd.grad calls per iteration and the (K, K) broadcast, the reference's op
sequence, unchanged code).

Shape: the PINN cell of `Nonlinear toy problem - parabolic with Neumann.ipynb` -- ExponentialOnSphereNonlinearParabolic d = 20,
T = 1, boundary_type 'Neumann', K = 200, K_boundary = 50, DenseNet(d + 1, 1, arch=[d + 20, d, d, d]), alpha = [1, 1, 1].

Both solvers are built once; then single-iteration train_PINN() calls alternate between them, `--warmup` pairs untimed and
`--iters` pairs timed one by one (host clock, a device synchronise before and after each call); the medians are reported.
One run on one GPU.

    python tools/time_pinn_time_h.py [--iters 20] [--warmup 5] [--json profiles/pinn_time_h_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import path_space_pde_solver_amd as psp  # noqa: E402

SHAPE = dict(problem="ExponentialOnSphereNonlinearParabolic", d=20, T=1.0, boundary_type="Neumann", K=200, K_boundary=50,
             arch=[40, 20, 20, 20], alpha=[1.0, 1.0, 1.0])
PLANS = {"native": dict(pinn_time_h="native"), "torch": dict(backend="torch")}


def build(dev, **plan):
    pb = psp.ExponentialOnSphereNonlinearParabolic(d=SHAPE["d"], T=SHAPE["T"], device=dev)
    pb.boundary_type = SHAPE["boundary_type"]
    model = psp.GeneralSolver(problem=pb, name="pinn", seed=42, lr=1e-3, L=1, K=SHAPE["K"], K_boundary=SHAPE["K_boundary"],
                              alpha=list(SHAPE["alpha"]), loss_method="PINN", verbose=False, print_every=10 ** 9, device=dev, **plan)
    model.V = psp.DenseNet(d_in=SHAPE["d"] + 1, d_out=1, lr=1e-3, arch=SHAPE["arch"], seed=42).to(dev)
    return model


def timed_iteration(model):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.train_PINN()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pinn_time_h.py needs the GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    models = {name: build(dev, **plan) for name, plan in PLANS.items()}
    times = {name: [] for name in models}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for it in range(a.warmup + a.iters):
            for name, model in models.items():
                dt = timed_iteration(model)
                assert model.plan_name == name, (name, model.plan_name, model.plan_reason)
                if it >= a.warmup:
                    times[name].append(dt)
    out = {"shape": SHAPE, "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "rows": {}}
    for name, ts in times.items():
        out["rows"][name] = {"median_ms_per_iteration": 1e3 * statistics.median(ts), "min_max_ms": [1e3 * min(ts), 1e3 * max(ts)],
                             "last_loss": models[name].loss_log[-1]}
        print("%-6s %.3f ms per iteration (min %.3f, max %.3f)" % (name, 1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts)),
              flush=True)
    out["torch_over_native"] = out["rows"]["torch"]["median_ms_per_iteration"] / out["rows"]["native"]["median_ms_per_iteration"]
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
