"""Per-iteration time of Solver.train with a list of Linear controls (time_approx='outer'; the notebook
`Ornstein-Uhlenbeck - quadratic costs - linear ansatz.ipynb`) two ways on the same GPU: the native plan (backend='native':
psp_aff_rollout_fwd / psp_aff_adjoint_sweep / psp_aff_rollout_bwd, csrc/aff_kernels.h) and the composite torch plan
(backend='torch': N steps of eager ops plus an autograd graph), which is what these lists ran on before the kernels existed.

Shapes:
  (a) the notebook's: LQGC d = 10, off_diag = 0.1, T = 0.5, K = 500, delta_t = 0.01 (N = 50), lr = 0.1, u_L2 log on, the
      reference's host noise stream; log-variance with a detached forward process and relative entropy attached; each without and
      with the in-loop importance-sampling sweep (IS_variance_K = 20000, native through psp_is_rollout);
  (b) LQGC d = 64, K = 65536, N = 50, noise='philox' (the composite plan has no device noise: it draws on the host as always),
      log-variance detached, u_L2 log on.

Each plan is warmed up by `--warmup` single-iteration train() calls, then `--iters` single-iteration calls are timed one by one
(host clock, a device synchronise before and after the timed block); the median is reported.  One run on one GPU.

    python tools/time_affine_control.py [--iters 20] [--warmup 5] [--json profiles/affine_control_timing.json]
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

LOGVAR = dict(loss_method="log-variance", detach_forward=True)
RELENT = dict(loss_method="relative_entropy", detach_forward=False)
NOTEBOOK = dict(d=10, K=500, T=0.5, delta_t=0.01, problem_delta_t=0.005)
LARGE = dict(d=64, K=65536, T=0.5, delta_t=0.01, problem_delta_t=0.005)
# (row, shape, solver keywords)
ROWS = [("notebook_logvar", NOTEBOOK, dict(LOGVAR)),
        ("notebook_relent_attached", NOTEBOOK, dict(RELENT)),
        ("notebook_logvar_is20000", NOTEBOOK, dict(LOGVAR, IS_variance_K=20000)),
        ("notebook_relent_attached_is20000", NOTEBOOK, dict(RELENT, IS_variance_K=20000)),
        ("d64_K65536_logvar_philox", LARGE, dict(LOGVAR, noise="philox"))]


def build(dev, shape, backend, **kw):
    d = shape["d"]
    pb = psp.LQGC(d=d, off_diag=0.1, T=shape["T"], seed=42, delta_t=shape["problem_delta_t"], device=dev)
    if backend == "torch":
        kw.pop("noise", None)
    model = psp.Solver(name="linear_ansatz", problem=pb, lr=0.1, L=1, K=shape["K"], delta_t=shape["delta_t"], time_approx="outer",
                       adaptive_forward_process=True, early_stopping_time=None, seed=42, verbose=False, print_every=10 ** 9,
                       device=dev, backend=backend, **kw)
    eye = torch.eye(d, device=dev)
    model.z_n = [psp.Linear(d=d, B=eye, Q=eye, lr=model.lr, seed=42).to(dev) for _ in range(model.N)]
    model.update_Phis()
    return model


def timed_iteration(model):
    model.L = 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.train()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_affine_control.py needs the GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda:0")
    out = {"shapes": {"notebook": NOTEBOOK, "d64_K65536": LARGE}, "iters": a.iters, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "rows": {}}
    for row, shape, kw in ROWS:
        rec = {"solver": {k: v for k, v in kw.items()}}
        for backend in ("native", "torch"):
            model = build(dev, shape, backend, **dict(kw))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for _ in range(a.warmup):                          # code objects, plan buffers, the first launches
                    timed_iteration(model)
                assert model.plan_name == backend, (row, model.plan_name, model.plan_reason)
                times = [timed_iteration(model) for _ in range(a.iters)]
            rec[backend] = {"median_ms_per_iteration": 1e3 * statistics.median(times),
                            "min_max_ms": [1e3 * min(times), 1e3 * max(times)], "last_loss": model.loss_log[-1],
                            "last_u_L2": model.u_L2_loss[-1]}
            print("%-34s %-6s %.3f ms per iteration (min %.3f, max %.3f)"
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
