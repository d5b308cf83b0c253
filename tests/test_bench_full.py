"""bench.py --full: a plain run prints the headline line only; the side measurements and self-checks run with --full.

The GPU cases start bench.py as a child process on small workloads (an eager one, a hipGraph one, a GeneralSolver one)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY_KEYS = ("also_sustained", "also_configs1_K1024_N50", "also_fp32_mfma_kernels", "cpu_baseline",
                  "loss_rel_err_vs_cpu_ref", "gpu_over_cpu", "also_composite_torch_plan_same_gpu", "parity_vs_1rank")
EAGER = "hjb_llgc_d100_K16384_N50_h64"       # 1024 tiles: eager launches
GRAPH = "hjb_llgc_d100_K4096_N50_h64"        # 256 tiles: the iteration is replayed as a hipGraph


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    a = bench.parse_args(["--full", "--no-cpu-baseline", "--no-secondary", "--no-sustained", "--steps", "2"])
    assert a.full and a.no_cpu_baseline and a.no_secondary and a.no_sustained and a.steps == 2


def run_bench(*argv):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"]
                         + list(argv), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    for k in HEADLINE_KEYS:
        assert k in line, k
    assert line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0
    return line


@pytest.mark.gpu
def test_plain_eager_run_keeps_the_roofline_of_the_timed_steps():
    line = run_bench("--workload", EAGER)
    assert line["config"]["launch"] == "eager launches"
    assert line["roofline"]["fwd_kernel_ms"] > 0 and line["roofline"]["bwd_kernel_ms"] > 0
    assert not [k for k in FULL_ONLY_KEYS if k in line]


@pytest.mark.gpu
def test_full_eager_run_adds_the_side_legs():
    line = run_bench("--workload", EAGER, "--full", "--no-cpu-baseline", "--sustain-s", "0.2")
    assert line["also_sustained"]["steps"] >= 50
    if line["config"]["matrix_products"] != "v_mfma_f32_16x16x4_f32":
        assert line["also_fp32_mfma_kernels"]["matrix_products"] == "fp32"
    assert "cpu_baseline" not in line


@pytest.mark.gpu
def test_graph_run_times_its_kernels_only_with_full():
    plain = run_bench("--workload", GRAPH)
    assert plain["config"]["launch"].startswith("hipGraph")
    assert plain["roofline"] is None
    full = run_bench("--workload", GRAPH, "--full", "--no-cpu-baseline", "--no-secondary")
    assert full["roofline"]["fwd_kernel_ms"] > 0 and full["roofline"]["bwd_kernel_ms"] > 0


@pytest.mark.gpu
def test_plain_general_run():
    line = run_bench("--workload", "diffusion_allencahn_d100_K200_N25_a110")
    assert line["reference_published"]["s_per_iteration"] == [0.31, 0.35]
    assert not [k for k in FULL_ONLY_KEYS if k in line]
