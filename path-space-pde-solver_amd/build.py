"""In-tree build of libpsp_hip.so (hipcc, gfx950 only).

    python path-space-pde-solver_amd/build.py [--force] [-j N]

Three kinds of translation unit under csrc/, linked into csrc/libpsp_hip.so next to the sources so that the
library travels with the tree:

* the C ABI layer (include/psp.h): api_common.hip and one api_<family>.hip per kernel family, over api_common.h;
* one instance unit per kernel family whose kernels are shaped at run time (hjbe_, hjbew_, aff_, genl_*_, pinn_,
  lstat_instance.hip);
* one instance unit per (d, H) line of a .def list for the families compiled per shape (instances.def,
  wide_instances.def, dense_instances.def, gen_instances.def).

A unit is recompiled when one of the files it is made of changes (unit_deps: its #include "..." lines, followed).
hipcc cross-compiles without a GPU.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "build")
LIB = os.path.join(CSRC, "libpsp_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
FLAGS = ["--offload-arch=" + ARCH, "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]


def instances(fname="instances.def"):
    out = []
    with open(os.path.join(CSRC, fname)) as fh:
        for line in fh:
            m = re.match(r"\s*X\(\s*(\d+)\s*,\s*(\d+)\s*\)", line)
            if m:
                out.append((int(m.group(1)), int(m.group(2))))
    return out


def _digest(paths, extra=""):
    h = hashlib.sha256(extra.encode())
    for p in paths:
        with open(p, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def unit_deps(src):
    """Every file a translation unit is made of: the source, then what its `#include "..."` lines name, followed recursively --
    headers, the .def instance lists, include/psp.h.  System headers (<...>) belong to the toolchain, not to the tree."""
    seen, todo = [], [os.path.normpath(src)]
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.append(path)
        with open(path) as fh:
            for name in re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', fh.read(), re.M):
                todo.append(os.path.normpath(os.path.join(os.path.dirname(path), name)))
    return seen


def _compile(src, obj, defs, force):
    stamp = obj + ".sha"
    dig = _digest(unit_deps(src), " ".join(FLAGS + defs))
    if not force and os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read() == dig:
        return obj, False
    cmd = [HIPCC] + FLAGS + defs + ["-c", src, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), r.stderr))
    with open(stamp, "w") as fh:
        fh.write(dig)
    return obj, True


def build(force=False, jobs=None, verbose=True, extra_flags=(), lib_path=None, obj_dir=None):
    """extra_flags / lib_path / obj_dir are for diagnostic variants (e.g. -DPSP_STAMPS into
    csrc/libpsp_hip_stamps.so); the default call builds the shipped library."""
    global FLAGS, OBJ, LIB
    saved = (FLAGS, OBJ, LIB)
    FLAGS = FLAGS + list(extra_flags)
    OBJ = obj_dir or OBJ
    LIB = lib_path or LIB
    try:
        return _build(force, jobs, verbose)
    finally:
        FLAGS, OBJ, LIB = saved


def _build(force, jobs, verbose):
    os.makedirs(OBJ, exist_ok=True)
    # The split of an fp32 operand into its f16 pair (hjb_kernels.h split8) costs two instructions per value only when the SLP
    # vectoriser leaves its two fmas alone: every translation unit but the wide family's is compiled with it off (measured, same
    # box: d = 100 forward -1.8 %, diffusion iteration -3 %, others unchanged; wide d = 500 backward +30 % from spills -- it keeps
    # the round-3 form).
    NOSLP, CLASSIC = ["-fno-slp-vectorize"], ["-DPSP_SPLIT_CLASSIC=1"]
    # (source, object, defines and flags); what a unit depends on is read from its #include lines (unit_deps)
    tasks = [("api_common.hip", "api_common.o", NOSLP),             # error buffer, shared checks and small kernels, Adam, RCCL, psp_loss_stats_*
             ("api_hjb.hip", "api_hjb.o", NOSLP),                   # psp_hjb_*: planner, narrow and wide tables, fused tail, basis, control eval
             ("api_gen.hip", "api_gen.o", NOSLP),                   # psp_gen_*: planner, table, the range guard's two kernels
             ("api_dnet.hip", "api_dnet.o", NOSLP),                 # psp_dnet_*, psp_gradvar_finish: planner, table, gradvar kernels
             ("api_aff.hip", "api_aff.o", NOSLP),                   # psp_aff_*: planner and bucket table
             ("api_genl.hip", "api_genl.o", NOSLP),                 # psp_genl_*: planner, genl_tables_kernel, plain genl_fwd / genl_bwd instances
             ("api_is.hip", "api_is.o", NOSLP),                     # psp_is_*, psp_isw_*: the checks and the argument fill of both rollouts
             ("api_pinn.hip", "api_pinn.o", NOSLP),                 # psp_pinn_*, psp_pinn_pairs_*: planner
             ("hjbe_instance.hip", "hjbe_inst.o", NOSLP),           # psp_is_rollout: every d bucket and control kind in one unit
             ("hjbew_instance.hip", "hjbew_inst.o", NOSLP),         # psp_isw_rollout: every block bucket and control kind, table kernel
             ("aff_instance.hip", "aff_inst.o", NOSLP),             # psp_aff_*: the three d buckets in one unit
             ("genl_eval_instance.hip", "genl_eval_inst.o", NOSLP),     # psp_genl_test_error: both waves-per-tile instances
             ("genl_lq_instance.hip", "genl_lq_inst.o", NOSLP),     # psp_genl_rollout_fwd_lq: three waves-per-tile variants
             ("genl_ul2_instance.hip", "genl_ul2_inst.o", NOSLP),   # psp_genl_rollout_fwd_ul2 (two shapes, three variants), gain staging
             ("genl_eig_instance.hip", "genl_eig_inst.o", NOSLP),   # psp_genl_rollout_fwd_eig: three waves-per-tile variants
             ("genl_adj_instance.hip", "genl_adj_inst.o", NOSLP),   # psp_genl_adjoint_sweep: three waves-per-tile variants
             ("pinn_instance.hip", "pinn_inst.o", NOSLP),           # psp_pinn_*: residual, per-sample finish, adjoint
             ("lstat_instance.hip", "lstat_inst.o", NOSLP)]         # psp_loss_stats_*: the loss estimators' statistics in double
    per_shape = [("hjbd_instance.hip", "dnet_inst", "dense_instances.def", NOSLP, 1 << 30),
                 ("hjb_instance.hip", "inst", "instances.def", NOSLP, 1 << 30),
                 ("hjbw_instance.hip", "wide_inst", "wide_instances.def", CLASSIC, 1 << 30),
                 # the split-product role-specialised backward of the wide instances up to d = 256: its own unit, SLP vectoriser off
                 ("hjbwx_instance.hip", "widex_inst", "wide_instances.def", NOSLP, 256),
                 ("gen_instance.hip", "gen_inst", "gen_instances.def", NOSLP, 1 << 30)]
    for src, stem, deffile, flags, d_max in per_shape:
        tasks += [(src, "%s_%d_%d.o" % (stem, d, H), ["-DPSP_D=%d" % d, "-DPSP_H=%d" % H] + flags)
                  for d, H in instances(deffile) if d <= d_max]
    tasks = [(os.path.join(CSRC, src), os.path.join(OBJ, obj), defs) for src, obj, defs in tasks]
    jobs = jobs or min(6, os.cpu_count() or 2)
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        results = list(ex.map(lambda t: _compile(t[0], t[1], t[2], force), tasks))
    objs = [r[0] for r in results]
    rebuilt = any(r[1] for r in results)
    # drop objects of instances that were removed from instances.def
    keep = set(os.path.basename(o) for o in objs)
    for f in os.listdir(OBJ):
        if f.endswith(".o") and f not in keep:
            os.remove(os.path.join(OBJ, f))
            rebuilt = True
    if rebuilt or force or not os.path.exists(LIB):
        cmd = [HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed: %s\n%s" % (" ".join(cmd), r.stderr))
        if verbose:
            print("built", LIB)
    elif verbose:
        print("up to date:", LIB)
    return LIB


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("-j", type=int, default=None)
    a = ap.parse_args()
    build(force=a.force, jobs=a.j)
    sys.exit(0)
