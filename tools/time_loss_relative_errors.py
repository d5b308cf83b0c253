"""Time of utilities.loss_relative_errors at the notebook's shape on one GPU, both plans.

Shape: `Compare relative errors of losses.ipynb` at its largest d -- LLGC d = 15, off_diag = 0.1, T = 1, delta_t = 0.005 (N = 200),
K = 5e7, noise='philox', the default untrained DenseNet(d + 1 -> d).  The native plan runs that K once, in its default chunks.
The composite torch plan (backend='torch' on the same GPU, the kernels' noise stream) is chunked too, so no K is too large
for it to fit; it runs K = 2**20 once and both are reported in seconds per 1e6 trajectories.  One small warm-up call per plan
(code objects, the first launches); host clock around each call, which ends with the read-back of the statistics.
Not a test, not run by bench.py; nothing is gated on these numbers.

    python tools/time_loss_relative_errors.py [--json profiles/loss_relative_errors_timing.json] [--K 50000000] [--K-torch 1048576]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import path_space_pde_solver_amd as psp  # noqa: E402

SHAPE = dict(d=15, off_diag=0.1, T=1, delta_t=0.005, lr=0.05, problem_seed=42, seed=0)


def timed(problem, net, K, backend):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = psp.loss_relative_errors(problem, net, K, delta_t=SHAPE["delta_t"], noise="philox", seed=SHAPE["seed"], backend=backend)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join("profiles", "loss_relative_errors_timing.json"))
    ap.add_argument("--K", type=int, default=5 * 10 ** 7)
    ap.add_argument("--K-torch", type=int, default=1 << 20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_loss_relative_errors.py needs the GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda:0")
    problem = psp.LLGC(d=SHAPE["d"], off_diag=SHAPE["off_diag"], T=SHAPE["T"], seed=SHAPE["problem_seed"], device=dev)
    net = psp.DenseNet(d_in=SHAPE["d"] + 1, d_out=SHAPE["d"], lr=SHAPE["lr"]).to(dev)
    out = {"shape": dict(SHAPE, N=int(SHAPE["T"] / SHAPE["delta_t"])), "device": torch.cuda.get_device_name(0),
           "runs": "one run on one GPU", "rows": {}}
    for row, backend, K in (("native", "native", a.K), ("composite", "torch", a.K_torch)):
        timed(problem, net, 1 << 16, backend)                                   # warm-up
        sec, res = timed(problem, net, K, backend)
        assert res["plan"] == backend and res["K"] == K, (res["plan"], res["plan_reason"])
        out["rows"][row] = {"K": K, "chunk": res["chunk"], "seconds": sec, "seconds_per_1e6_trajectories": sec / (K / 1e6),
                            "statistics": {key: list(res[key]) for key in psp.utilities.LRE_KEYS}}
        print("%-10s K = %d  chunk = %d: %.3f s, %.4f s per 1e6 trajectories" % (row, K, res["chunk"], sec, sec / (K / 1e6)), flush=True)
    out["composite_over_native_per_trajectory"] = (out["rows"]["composite"]["seconds_per_1e6_trajectories"]
                                                   / out["rows"]["native"]["seconds_per_1e6_trajectories"])
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
