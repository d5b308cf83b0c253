"""Wall time of the paper notebook's importance-sampling call (Double well - 1d - high metastability.ipynb, cell 3:
do_importance_sampling_me(dw, model, 1e7, control='true', simulate_naive=True, delta_t=0.01, cross_statistics=[[0]])) three ways:
native with on-device noise, native with the reference's CPU-generator noise, and the composite plan on the same GPU.

    python tools/time_is_eval.py [--K 10000000] [--native-only]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import path_space_pde_solver_amd as psp  # noqa: E402


def run(K, backend, noise, delta_t=0.01):
    dev = torch.device("cuda:0")
    prob = psp.DoubleWell(d=1, T=1, eta=3.0, kappa=5.0, device=dev)
    prob.compute_reference_solution()
    model = psp.Solver("t", prob, L=0, K=16, delta_t=delta_t, time_approx="inner", verbose=False, device=dev, backend=backend,
                       noise=noise)
    torch.manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = psp.do_importance_sampling_me(prob, model, K, control="true", simulate_naive=True, verbose=True, delta_t=delta_t,
                                        cross_statistics=torch.tensor([[0]]))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    N = int(round(prob.T / delta_t))
    print("%-28s K=%d  wall %.3f s  %.3e trajectory-steps/s (both paths)" % (backend + " / " + noise, K, wall, 2 * K * N / wall))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=10_000_000)
    ap.add_argument("--native-only", action="store_true")
    a = ap.parse_args()
    run(min(a.K, 1 << 16), "native", "philox")          # warm-up: module load, first launch
    run(a.K, "native", "philox")
    if not a.native_only:
        run(a.K, "native", "reference")
        run(a.K, "torch", "reference")


if __name__ == "__main__":
    main()
