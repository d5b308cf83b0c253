"""Per-iteration time of train_PINN() two ways on the same GPU: the native plan (backend='native': psp_pinn_residual /
psp_pinn_backward, csrc/pinn_kernels.h) and the composite torch plan (backend='torch': d + 1 autograd.grad calls per iteration,
the reference's op sequence), which is what the reference itself runs.

Shapes (the PINN cells of the reference's notebooks):
  allencahn_notebook   GeneralSolver, Allen-Cahn d = 100, K = 200, K_boundary = 50, arch [110, 110, 50], uniform_square
                       (the reference's notebook prints 0.54 - 0.60 s per iteration for this cell)
  elliptic_dirichlet   EllipticSolver, ExponentialOnBallNonlinearSin d = 50, K = 200, K_boundary = 50, arch [70, 50, 50, 50]
  full_hessian         EllipticSolver(full_hessian=True, hessian='directions'), ExponentialOnBallNonlinearSinHessian d = 20 (sigma = sqrt(2/d) ones),
                       K = 200, K_boundary = 50, the solver's default net, as the notebook leaves it.  Composite: one
                       autograd.functional.hessian call per sample; native: one direction u = sqrt(2) 1 per sample.
                       `--shapes full_hessian --json profiles/pinn_hessian_timing.json` wrote the committed record.

Each plan is warmed up by `--warmup` single-iteration train_PINN() calls, then `--iters` single-iteration calls are timed one by
one (host clock, a device synchronise before and after); the median is reported.  One run on one GPU.

    python tools/time_pinn.py [--iters 20] [--warmup 5] [--shapes allencahn_notebook,elliptic_dirichlet]
                              [--json profiles/pinn_timing.json]
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

REFERENCE_PUBLISHED_S = 0.54           # Allen-Cahn.ipynb, cell 8 output (the reference's own GPU)
SHAPES = {"allencahn_notebook": dict(solver="GeneralSolver", problem="AllenCahn", d=100, K=200, K_boundary=50, arch=[110, 110, 50]),
          "elliptic_dirichlet": dict(solver="EllipticSolver", problem="ExponentialOnBallNonlinearSin", d=50, K=200, K_boundary=50,
                                     arch=[70, 50, 50, 50]),
          "full_hessian": dict(solver="EllipticSolver", problem="ExponentialOnBallNonlinearSinHessian", d=20, K=200, K_boundary=50,
                               alpha=1.0, arch=None, full_hessian=True)}
DEFAULT_SHAPES = "allencahn_notebook,elliptic_dirichlet"


def build(dev, shape, backend):
    common = dict(name="pinn", seed=42, lr=1e-3, L=1, K=shape["K"], K_boundary=shape["K_boundary"], loss_method="PINN",
                  verbose=False, print_every=10 ** 9, device=dev, backend=backend)
    if shape["solver"] == "GeneralSolver":
        pb = psp.AllenCahn(d=shape["d"], T=0.3, seed=42, modus="pt", device=dev)
        pb.B = pb.B_pt                                              # as the notebook does before the PINN cell
        model = psp.GeneralSolver(problem=pb, uniform_square=True, **common)
        d_in = shape["d"] + 1
    else:
        pb = getattr(psp, shape["problem"])(d=shape["d"], alpha=shape.get("alpha", 0.5), device=dev)
        model = psp.EllipticSolver(problem=pb, full_hessian=shape.get("full_hessian", False), hessian="directions",
                                   **common)
        d_in = shape["d"]
    if shape["arch"] is not None:
        model.V = psp.DenseNet(d_in=d_in, d_out=1, lr=1e-3, arch=shape["arch"], seed=42).to(dev)
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
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated rows of SHAPES")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pinn.py needs the GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda:0")
    shapes = {k: SHAPES[k] for k in a.shapes.split(",")}
    out = {"shapes": shapes, "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "reference_published_s_per_iteration": REFERENCE_PUBLISHED_S, "rows": {}}
    for row, shape in shapes.items():
        rec = {}
        for backend in ("native", "torch"):
            torch.manual_seed(42)
            model = build(dev, shape, backend)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for _ in range(a.warmup):
                    timed_iteration(model)
                assert model.plan_name == backend, (row, model.plan_name, model.plan_reason)
                times = [timed_iteration(model) for _ in range(a.iters)]
            rec[backend] = {"median_ms_per_iteration": 1e3 * statistics.median(times),
                            "min_max_ms": [1e3 * min(times), 1e3 * max(times)], "last_loss": model.loss_log[-1]}
            print("%-20s %-6s %.3f ms per iteration (min %.3f, max %.3f)"
                  % (row, backend, 1e3 * statistics.median(times), 1e3 * min(times), 1e3 * max(times)), flush=True)
        rec["torch_over_native"] = rec["torch"]["median_ms_per_iteration"] / rec["native"]["median_ms_per_iteration"]
        out["rows"][row] = rec
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
