"""Time of ONE logged iteration of Solver(compute_gradient_variance=1) two ways on the same GPU: the native plan
(DenseNativePlan.gradient_moments: adjoint sweeps, psp_dnet_rollout_bwd / psp_dnet_rollout_bwd_sq, psp_gradvar_finish) and the
composite torch plan (Solver.get_gradient_variances: K backward passes per time step through the N-step autograd graph, plus the
terminal-cost gradient), and the native plan's iteration with the diagnostic off.

Shape: LLGC d = 10, the constructor's default nets and flags (time_approx='outer', log-variance, adaptive, attached), K = 100,
delta_t = 0.05, T = 0.5 (N = 10): about 1000 autograd passes per logged iteration for the composite plan.  One warm-up iteration,
then one timed iteration per plan (host clock, a device synchronise before and after); the composite plan is too slow for more.
Nothing is gated on these numbers.

    python tools/time_gradient_variance.py [--json profiles/gradient_variance_timing.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import path_space_pde_solver_amd as psp  # noqa: E402

SHAPE = dict(d=10, K=100, T=0.5, delta_t=0.05)


def build(dev, backend, m):
    pb = psp.LLGC(d=SHAPE["d"], off_diag=0.1, T=SHAPE["T"], seed=42, device=dev)
    return psp.Solver(name="gradvar", problem=pb, L=1, K=SHAPE["K"], delta_t=SHAPE["delta_t"], compute_gradient_variance=m,
                      early_stopping_time=None, verbose=False, print_every=10 ** 9, device=dev, backend=backend)


def timed_iteration(model):
    model.L = 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.train()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--native-iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gradient_variance.py needs the GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda:0")
    out = {"shape": SHAPE, "device": torch.cuda.get_device_name(0), "rows": {}}
    for row, backend, m, iters in (("native_logged", "native", 1, a.native_iters), ("native_diagnostic_off", "native", 0, a.native_iters),
                                   ("composite_logged", "torch", 1, 1)):
        model = build(dev, backend, m)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            timed_iteration(model)                                  # warm-up: code objects, plan buffers, the first launches
            assert model.plan_name == backend, (row, model.plan_name, model.plan_reason)
            times = [timed_iteration(model) for _ in range(iters)]
        out["rows"][row] = {"N": model.N, "p": int(model.p), "timed_iterations": iters, "first_ms": 1e3 * times[0],
                            "median_ms": 1e3 * sorted(times)[len(times) // 2],
                            "grads_rel_error_log_last": model.grads_rel_error_log[-1] if model.grads_rel_error_log else None}
        print("%-24s %-6s first %.3f ms, median of %d: %.3f ms" % (row, backend, 1e3 * times[0], iters, out["rows"][row]["median_ms"]),
              flush=True)
    out["composite_over_native_logged"] = out["rows"]["composite_logged"]["median_ms"] / out["rows"]["native_logged"]["median_ms"]
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
