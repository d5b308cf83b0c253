"""Per-iteration time of Solver(approx_method='value_function') on LQGC with off-diagonal entries -- dense drift matrix, dense
sigma, running cost -- two ways on the same GPU: the native plan (backend='native', noise='philox': the linear-quadratic
instances of the run-time-shaped value-net kernels, psp_genl_rollout_fwd_lq + psp_genl_rollout_bwd) and the composite torch plan
(backend='torch': autograd with create_graph=True through every step), which is what this configuration ran on before the
kernels took these coefficients.  Each of the two is timed with the u_L2 log off and on (u_l2_error_flag): the native plan
accumulates the log inside the forward kernel (psp_genl_rollout_fwd_ul2: one more d x d product per step from gains staged once),
the composite plan evaluates problem.u_true on the host every step.  Two more rows time the ATTACHED state path
(detach_forward=False, the constructor default), u_L2 log off: the native plan with the adjoint sweep between its forward and
backward kernels (value_state_path='native': psp_genl_adjoint_sweep, csrc/genl_adj_kernels.h) and the composite torch plan, which
is what the default value_state_path='torch' runs for this configuration.

Configuration: LQGC d = 20, off_diag = 0.1, T = 1, delta_t = 0.05 (N = 20), K = 4096, log-variance loss, adaptive forward process
with the state path detached (rows native, native_u_l2, torch, torch_u_l2) or attached (rows native_attached, torch_attached).

Each plan is warmed up by `--warmup` single-iteration train() calls, then `--iters` single-iteration calls are timed one by one
(host clock, a device synchronise before and after the timed block); the median is reported.

    python tools/time_value_function.py [--iters 20] [--warmup 5] [--json profiles/value_function_timing.json]
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

CONFIG = dict(d=20, off_diag=0.1, T=1.0, delta_t=0.05, K=4096)
MODES = [("native", "native", dict(backend="native", noise="philox", u_l2_error_flag=False)),
         ("native_u_l2", "native", dict(backend="native", noise="philox", u_l2_error_flag=True)),
         ("torch", "torch", dict(backend="torch", u_l2_error_flag=False)),
         ("torch_u_l2", "torch", dict(backend="torch", u_l2_error_flag=True)),
         ("native_attached", "native", dict(backend="native", noise="philox", u_l2_error_flag=False, detach_forward=False,
                                            value_state_path="native")),
         ("torch_attached", "torch", dict(backend="torch", u_l2_error_flag=False, detach_forward=False))]


def build(dev, detach_forward=True, **kw):
    pb = psp.LQGC(d=CONFIG["d"], off_diag=CONFIG["off_diag"], T=CONFIG["T"], delta_t=CONFIG["delta_t"], seed=42, device=dev)
    return psp.Solver(name="lqgc_d20_value_function", problem=pb, lr=0.001, L=1, K=CONFIG["K"], delta_t=CONFIG["delta_t"],
                      approx_method="value_function", time_approx="inner", loss_method="log-variance",
                      adaptive_forward_process=True, detach_forward=detach_forward, early_stopping_time=None,
                      seed=42, verbose=False, print_every=10 ** 9, device=dev, **kw)


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
        raise SystemExit("time_value_function.py needs the GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda:0")
    out = {"config": dict(CONFIG, N=int(round(CONFIG["T"] / CONFIG["delta_t"])), problem="LQGC", loss_method="log-variance"),
           "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "plans": {}}
    ms = {}
    for name, plan_name, kw in MODES:
        model = build(dev, **kw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(a.warmup):                              # code objects, plan buffers, the first launches
                timed_iteration(model)
            assert model.plan_name == plan_name, (name, model.plan_name, model.plan_reason)
            assert bool(model.u_l2_error_flag) == kw["u_l2_error_flag"] and (model.u_L2_loss[-1] > 0) == kw["u_l2_error_flag"]
            times = [timed_iteration(model) for _ in range(a.iters)]
        ms[name] = 1e3 * statistics.median(times)
        out["plans"][name] = {"noise": kw.get("noise", "reference"), "u_l2_error_flag": kw["u_l2_error_flag"],
                              "detach_forward": kw.get("detach_forward", True),
                              "median_ms_per_iteration": ms[name], "min_max_ms": [1e3 * min(times), 1e3 * max(times)],
                              "last_loss": model.loss_log[-1], "last_u_L2": model.u_L2_loss[-1]}
        print("%-12s %.3f ms per iteration (min %.3f, max %.3f)" % (name, ms[name], 1e3 * min(times), 1e3 * max(times)))
    out["torch_over_native"] = ms["torch"] / ms["native"]
    out["torch_over_native_u_l2"] = ms["torch_u_l2"] / ms["native_u_l2"]
    out["native_u_l2_over_native"] = ms["native_u_l2"] / ms["native"]
    out["torch_attached_over_native_attached"] = ms["torch_attached"] / ms["native_attached"]
    out["native_attached_over_native"] = ms["native_attached"] / ms["native"]
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
