"""Per-iteration time of a diffusion-loss notebook run with its K_test_log diagnostic three ways: without the log
(K_test_log=None), with the reference's host log (test_log='reference': CPU generator, upload, torch forward, device-to-host
copy, numpy -- every iteration) and with the device log (test_log='device': psp_genl_test_error, read back once).

Two configurations: the full-Hessian notebook's diffusion leg (`Nonlinear toy problem - elliptic with full Hessian.ipynb`:
ExponentialOnBallNonlinearSinHessian, d = 20, K = 200, N = 20, K_test_log = 10000) and an Allen-Cahn-sized value net
(arch = [110, 110, 50] at d = 100) on the exponential-on-the-ball problem, both with noise='philox'.

Every mode is warmed up by a train() call of its own, then the modes are timed alternately (repeats x one train() of `steps`
iterations each, host clock around a run that ends in a device synchronise); the median over the repeats is reported.

    python tools/time_test_log.py [--steps 200] [--repeats 5] [--json profiles/test_log_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import path_space_pde_solver_amd as psp  # noqa: E402

MODES = [("none", dict(K_test_log=None)), ("reference", dict(K_test_log=10000, test_log="reference")),
         ("device", dict(K_test_log=10000, test_log="device"))]


def build(config, dev, **kw):
    common = dict(seed=42, delta_t=0.001, lr=0.001, K_boundary=50, print_every=10 ** 9, verbose=False, device=dev,
                  backend="native", noise="philox", v_l2_error_flag=False)
    common.update(kw)
    if config == "full_hessian_d20":
        pb = psp.ExponentialOnBallNonlinearSinHessian(d=20, device=dev)
        return psp.EllipticSolver(pb, config, K=200, N=20, **common)
    pb = psp.ExponentialOnBallNonlinear(d=100, device=dev)
    model = psp.EllipticSolver(pb, config, K=200, N=20, **common)
    model.V = psp.DenseNet(d_in=100, d_out=1, lr=0.001, arch=[110, 110, 50], seed=42).to(dev)
    return model


def timed_train(model, steps):
    model.L = steps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.train()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_test_log.py needs the GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda:0")
    out = {"steps": a.steps, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "configs": {}}
    for config in ("full_hessian_d20", "allen_cahn_net_d100"):
        models = {name: build(config, dev, L=a.warmup, **kw) for name, kw in MODES}
        for name, model in models.items():                       # warm-up: code objects, plan buffers, the first launches
            timed_train(model, a.warmup)
            assert model.plan_name == "native", (name, model.plan_name, model.plan_reason)
        times = {name: [] for name in models}
        for _ in range(a.repeats):                                # alternate the modes: other work shares the host
            for name, model in models.items():
                times[name].append(timed_train(model, a.steps))
        ms = {name: 1e3 * statistics.median(v) for name, v in times.items()}
        spread = {name: [1e3 * min(v), 1e3 * max(v)] for name, v in times.items()}
        host_share = (ms["reference"] - ms["none"]) / ms["reference"]
        rec = {"ms_per_iteration": ms, "min_max_ms": spread, "host_log_share_of_reference_iteration": host_share,
               "device_log_cost_ms": ms["device"] - ms["none"],
               "last_V_test_L2": {n: (m.V_test_L2[-1] if m.V_test_L2 else None) for n, m in models.items()}}
        out["configs"][config] = rec
        print("%-22s none %.3f ms | reference %.3f ms | device %.3f ms | host log = %.0f %% of the reference iteration, "
              "device log costs %.3f ms" % (config, ms["none"], ms["reference"], ms["device"], 100 * host_share,
                                            rec["device_log_cost_ms"]))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
