"""build.py reads what a translation unit depends on from its #include lines (build.unit_deps): a header cannot be forgotten."""
import importlib.util
import os
import re

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


# the units of the C ABI layer: (what each must reach, the kernel headers -- csrc/*_kernels.h -- it may reach)
API_UNITS = {
    "api_common.hip": ({"csrc/lstat_kernels.h", "csrc/hjb_kernels.h"}, {"lstat", "hjb"}),          # hjb_kernels.h: Philox
    "api_hjb.hip": ({"csrc/instances.def", "csrc/wide_instances.def", "csrc/hjb_kernels.h", "csrc/hjbw_kernels.h",
                     "csrc/hjb_basis_kernels.h"}, {"hjb", "hjbw", "hjb_basis"}),
    "api_gen.hip": ({"csrc/gen_instances.def", "csrc/gen_kernels.h", "csrc/gh_kinds.h"}, {"gen", "hjb"}),
    "api_dnet.hip": ({"csrc/dense_instances.def", "csrc/hjbd_kernels.h"}, {"hjbd", "hjbw", "hjb"}),
    "api_aff.hip": ({"csrc/aff_kernels.h"}, {"aff", "hjb"}),
    "api_genl.hip": ({"csrc/genl_kernels.h", "csrc/genl_eval_kernels.h", "csrc/genl_adj_kernels.h", "csrc/gh_kinds.h"},
                     {"genl", "genl_eval", "genl_adj", "gen", "hjb"}),
    "api_is.hip": ({"csrc/hjbe_kernels.h", "csrc/hjbew_kernels.h"}, {"hjbe", "hjbew", "hjb"}),     # hjbe pulls hjb_kernels.h: Philox
    "api_pinn.hip": ({"csrc/pinn_kernels.h", "csrc/gh_kinds.h"}, {"pinn"}),
}
DEF_OWNER = {"csrc/instances.def": "api_hjb.hip", "csrc/wide_instances.def": "api_hjb.hip",
             "csrc/gen_instances.def": "api_gen.hip", "csrc/dense_instances.def": "api_dnet.hip"}


def _kernel_headers(deps):
    return {os.path.basename(p)[:-len("_kernels.h")] for p in deps if p.startswith("csrc/") and p.endswith("_kernels.h")}


def test_the_api_unit_lists_the_instance_lists_and_the_header():
    union = set()
    for unit, (must, _) in API_UNITS.items():
        deps = _deps(unit)
        assert must | {"../include/psp.h", "csrc/launch.h", "csrc/api_common.h"} <= deps, unit
        union |= deps
    assert {"csrc/instances.def", "csrc/gen_instances.def", "csrc/wide_instances.def", "csrc/dense_instances.def",
            "../include/psp.h", "csrc/launch.h"} <= union
    # each instance list is included by the one unit that builds the table from it
    for deffile, owner in DEF_OWNER.items():
        assert [u for u in API_UNITS if deffile in _deps(u)] == [owner], deffile


def test_an_api_unit_reaches_no_kernel_header_of_another_family():
    for unit, (_, may) in API_UNITS.items():
        assert _kernel_headers(_deps(unit)) == may, unit
    # spelled out for the unit whose kernels do without the rollouts' MFMA machinery
    pinn = _kernel_headers(_deps("api_pinn.hip"))
    assert not any(h.startswith(("hjb", "gen")) or h == "aff" for h in pinn)
    # api_common.h is what every unit parses: it brings no kernel header with it
    assert _kernel_headers(_deps("api_common.h")) == set()


def test_every_hip_file_is_a_build_task():
    with open(os.path.join(PKG, "build.py")) as fh:
        named = set(re.findall(r'"(\w+\.hip)"', fh.read()))
    on_disk = {f for f in os.listdir(os.path.join(PKG, "csrc")) if f.endswith(".hip")}
    assert on_disk == named


def test_pinn_instance_lists_its_headers():
    deps = _deps("pinn_instance.hip")
    assert {"csrc/pinn_kernels.h", "csrc/gh_kinds.h", "csrc/launch.h"} <= deps
    assert "csrc/hjb_kernels.h" not in deps                          # the PINN kernels do without the rollouts' MFMA machinery
