"""Wall time of do_importance_sampling_me(control='true', simulate_naive=True) above d = 64, two ways on one MI355X: the wide-state
kernel (wide_states='native', psp_isw_rollout, K = 2^20) and the composite plan (wide_states='torch', the code path before the
kernel existed: u_true on the host every step, K = 2^16).  noise='philox', delta_t = 0.01, T = 1; one warm-up call of the same
shape before each timed call; the host clock runs around the call and a device synchronise.  Both are reported per 10^6
trajectories (the naive and the controlled path together).  Recorded, not gated: no test reads the file.

    python tools/time_is_wide.py [--out profiles/is_wide_timing.json] [--K-native 1048576] [--K-torch 65536]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import path_space_pde_solver_amd as psp  # noqa: E402

DELTA_T, T = 0.01, 1.0


def problems(dev):
    nat = psp.native
    for d in (100, 200, nat.ISW_MAX_D):
        yield "LLGC d=%d" % d, psp.LLGC(d=d, off_diag=0.1 / math.sqrt(d), T=T, seed=42, device=dev)
    yield "LQGC d=100", psp.LQGC(d=100, off_diag=0.1 / math.sqrt(100), T=T, seed=42, delta_t=0.005, device=dev)


def timed(prob, dev, K, wide_states):
    model = psp.Solver("t", prob, L=0, K=16, delta_t=DELTA_T, time_approx="inner", verbose=False, device=dev,
                       backend="native" if wide_states == "native" else "auto", noise="philox")
    out = wall = None
    for _ in range(2):                                  # the first call is the warm-up
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = psp.do_importance_sampling_me(prob, model, K, control="true", simulate_naive=True, delta_t=DELTA_T,
                                            wide_states=wide_states)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    return wall, [float(v) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "is_wide_timing.json"))
    ap.add_argument("--K-native", type=int, default=1 << 20)
    ap.add_argument("--K-torch", type=int, default=1 << 16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_is_wide.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    rows = []
    for label, prob in problems(dev):
        row = {"problem": label, "N": int(math.ceil(T / DELTA_T))}
        for ws, K in (("native", a.K_native), ("torch", a.K_torch)):
            wall, out = timed(prob, dev, K, ws)
            row[ws] = {"K": K, "wall_s": wall, "s_per_1e6_trajectories": wall * 1e6 / K, "rel_error_naive": out[2],
                       "rel_error_IS": out[5]}
            print("%-12s %-6s K=%-8d wall %8.3f s   %9.3f s per 1e6 trajectories" % (label, ws, K, wall, wall * 1e6 / K), flush=True)
        row["speedup_per_trajectory"] = row["torch"]["s_per_1e6_trajectories"] / row["native"]["s_per_1e6_trajectories"]
        rows.append(row)
    rec = {"device": torch.cuda.get_device_name(0), "delta_t": DELTA_T, "T": T, "noise": "philox",
           "call": "do_importance_sampling_me(control='true', simulate_naive=True)", "runs": 1, "warmup_calls": 1, "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
