"""csrc/block_index.h on the host: the producers of hjb_bwd2_kernel / hjb_bwd3_kernel walk their sample blocks with
psp::BlockCursor -- (tile, step) advanced by a constant pair and one carry -- instead of dividing the block number by the tile
count every round.  A stand-alone program (its own main, the C++ compiler of build.py, no GPU) walks every workgroup, producer
slot and round of every launch shape below, two rounds past the workgroup's last (the kernels' loop runs it = 0 .. R and reads
the cursor of round it + 1), and compares the cursor's (t16, n, valid, block) with the division form
    b0 = (bid + it * grid) * 4 + sub;  valid = b0 < N * ntile16;  b = valid ? b0 : N * ntile16 - 1;  (b % ntile16, b / ntile16).
The shapes cover stride < / = / > ntile16 (q = 0 and q >> 1), r = 0, ntile16 = 1, a ragged last round, fewer blocks than one
round, and more workgroups than rounds."""
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-space-pde-solver_amd", "csrc")

GRIDS = [1, 2, 3, 7, 64, 255, 256, 304]
NTILES = [1, 2, 3, 4, 5, 37, 1023, 1024, 1025, 1100, 4096]
STEPS = [1, 2, 3, 60, 100]

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "block_index.h"

int main(int argc, char** argv) {
    // argv: ngrid grids... ntile ntiles... nstep steps...
    int p = 1;
    auto list = [&](int& n) { n = atoi(argv[p++]); int* v = new int[n]; for (int i = 0; i < n; ++i) v[i] = atoi(argv[p++]); return v; };
    int ng, nt, ns;
    const int* grids = list(ng); const int* tiles = list(nt); const int* steps = list(ns);
    long long checks = 0, bad = 0, carries = 0, plain = 0, parked = 0, shapes = 0;
    for (int gi = 0; gi < ng; ++gi) for (int ti = 0; ti < nt; ++ti) for (int si = 0; si < ns; ++si) {
        const long long grid = grids[gi], ntile16 = tiles[ti], N = steps[si];
        const long long nblk = N * ntile16, nround = (nblk + 3) / 4;
        ++shapes;
        for (long long bid = 0; bid < grid; ++bid) {
            const long long R = bid < nround ? (nround - bid + grid - 1) / grid : 0;      // rounds of this workgroup (the kernels' R)
            for (int sub = 0; sub < 4; ++sub) {
                psp::BlockCursor c = psp::BlockCursor::start((uint32_t)bid, (uint32_t)sub, (uint32_t)grid, (uint32_t)ntile16, (uint32_t)N);
                for (long long it = 0; it <= R + 2; ++it) {
                    const long long b0 = (bid + it * grid) * 4 + sub;
                    const bool valid = b0 < nblk;
                    const long long b = valid ? b0 : nblk - 1;
                    ++checks;
                    if (c.valid != valid || (long long)c.blk != b || (long long)c.t16 != b % ntile16 || (long long)c.n != b / ntile16) {
                        if (bad++ < 20)
                            printf("MISMATCH grid %lld ntile16 %lld N %lld bid %lld sub %d it %lld: cursor (%u, %u, %d, %u) division (%lld, %lld, %d, %lld)\n",
                                   grid, ntile16, N, bid, sub, it, c.t16, c.n, (int)c.valid, c.blk, b % ntile16, b / ntile16, (int)valid, b);
                    }
                    const uint32_t t_before = c.t16;
                    const bool was = c.valid;
                    c.advance();
                    if (was && c.valid) { if (c.t16 < t_before + c.r) ++carries; else ++plain; }
                    if (was && !c.valid) ++parked;
                }
            }
        }
    }
    printf("shapes %lld checks %lld bad %lld carries %lld plain %lld parked %lld\n", shapes, checks, bad, carries, plain, parked);
    return bad == 0 ? 0 : 1;
}
"""


def _hipcc():
    spec = importlib.util.spec_from_file_location("psp_build_for_block_index", os.path.join(ROOT, "path-space-pde-solver_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC


def test_cursor_equals_the_division_form_on_every_workgroup_slot_and_round(tmp_path):
    src, exe = tmp_path / "block_index_walk.cpp", tmp_path / "block_index_walk"
    src.write_text(PROGRAM)
    # host C++ only: the header's __host__ __device__ spelling is for the kernels' translation units
    cc = subprocess.run([_hipcc(), "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    args = []
    for v in (GRIDS, NTILES, STEPS):
        args += [str(len(v))] + [str(x) for x in v]
    run = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=120)
    print(run.stdout[-3000:])
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-1000:]
    tally = dict(zip(run.stdout.split()[-12::2], (int(x) for x in run.stdout.split()[-11::2])))
    assert tally["shapes"] == len(GRIDS) * len(NTILES) * len(STEPS) and tally["bad"] == 0
    # the walk met every branch of advance(): a carry, no carry, and the step out of the store
    assert tally["carries"] > 0 and tally["plain"] > 0 and tally["parked"] > 0 and tally["checks"] > 10 ** 6
