"""build.py reads what a translation unit depends on from its #include lines (build.unit_deps): a header cannot be forgotten."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "path-space-pde-solver_amd")


def _deps(unit):
    spec = importlib.util.spec_from_file_location("psp_build_for_deps", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    deps = build.unit_deps(os.path.join(PKG, "csrc", unit))
    assert all(os.path.isfile(p) for p in deps) and len(set(deps)) == len(deps)
    assert os.path.samefile(deps[0], os.path.join(PKG, "csrc", unit))
    return {os.path.relpath(p, PKG).replace(os.sep, "/") for p in deps}


def test_gen_instance_lists_its_headers():
    assert {"csrc/gen_kernels.h", "csrc/gh_kinds.h", "csrc/hjb_kernels.h", "csrc/launch.h"} <= _deps("gen_instance.hip")


def test_the_api_unit_lists_the_instance_lists_and_the_header():
    deps = _deps("psp_api.hip")
    assert {"csrc/instances.def", "csrc/gen_instances.def", "csrc/wide_instances.def", "csrc/dense_instances.def",
            "../include/psp.h", "csrc/launch.h"} <= deps


def test_pinn_instance_lists_its_headers():
    deps = _deps("pinn_instance.hip")
    assert {"csrc/pinn_kernels.h", "csrc/gh_kinds.h", "csrc/launch.h"} <= deps
    assert "csrc/hjb_kernels.h" not in deps                          # the PINN kernels do without the rollouts' MFMA machinery
