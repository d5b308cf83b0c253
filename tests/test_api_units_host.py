"""The C ABI layer is one unit per kernel family (csrc/api_*.hip) over csrc/api_common.h.  Host checks, no GPU: every function of
include/psp.h resolves in the library, the refusals of the query entry points keep their codes and texts, every unit reports
through the one psp_last_error() buffer, and psp_is_query / psp_isw_query fire their shared checks in the same order."""
import ctypes as C
import os
import re

import pytest

from util_cases import psp

nat = psp.native
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_KEEP = (C.c_float * 4)()            # a non-null address; the query entry points read no buffer
PTR = C.addressof(_KEEP)


def call(name, *args):
    rc = getattr(nat.load(), name)(*args)
    return rc, nat.last_error()


def test_every_function_of_the_header_resolves():
    with open(os.path.join(ROOT, "include", "psp.h")) as fh:
        text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S))
    declared = set(re.findall(r"\b(psp_[a-z0-9_]+)\s*\(", text))
    assert len(declared) == 83 and declared == set(nat.SIGNATURES)
    lib = C.CDLL(nat.LIB_PATH)
    assert [n for n in sorted(declared) if not hasattr(lib, n)] == []


def _null_query(name):
    out = {"psp_hjb_query": nat.HjbSizes, "psp_gen_query": nat.GenSizes, "psp_genl_query": nat.GenlSizes,
           "psp_genl_eval_query": nat.GenlEvalSizes, "psp_dnet_query": nat.DnetSizes, "psp_aff_query": nat.AffSizes,
           "psp_isw_query": nat.IswSizes, "psp_pinn_query": nat.PinnSizes, "psp_pinn_pairs_query": nat.PinnSizes}
    if name == "psp_is_query":
        return call(name, None, C.byref(C.c_int32()))
    if name == "psp_pinn_pairs_query":
        return call(name, None, C.byref(out[name]()), C.byref(C.c_int64()))
    return call(name, None, C.byref(out[name]()))


@pytest.mark.parametrize("name", ["psp_hjb_query", "psp_gen_query", "psp_genl_query", "psp_genl_eval_query", "psp_dnet_query",
                                  "psp_aff_query", "psp_is_query", "psp_isw_query", "psp_pinn_query", "psp_pinn_pairs_query"])
def test_a_null_config_is_refused(name):
    call("psp_adam_step", None, None, None, None, 1, 1, 0.1, 0.9, 0.999, 1e-8, None)       # (leaves another message behind)
    assert _null_query(name) == (-1, "null config")


def _refusals():
    """One refused call per unit of the layer, each with a message of its own: name -> (thunk, code, message)."""
    hjb = nat.HjbConfig()
    gen = nat.GenConfig()
    dnet = nat.DnetConfig()
    aff = nat.AffConfig()
    aff.struct_bytes = 0
    ev = nat.GenlEvalConfig()
    isc = nat.IsConfig()
    pinn = nat.PinnConfig()
    return {
        "common": (lambda: call("psp_adam_step", None, None, None, None, 1, 1, 0.1, 0.9, 0.999, 1e-8, None),
                   -1, "null buffer passed to psp_adam_step"),
        "hjb": (lambda: call("psp_hjb_query", C.byref(hjb), C.byref(nat.HjbSizes())), -1, "non-positive d/H/K/N"),
        "gen": (lambda: call("psp_gen_instance_get", -1, C.byref(C.c_int32()), C.byref(C.c_int32())),
                -1, "instance index out of range"),
        "dnet": (lambda: call("psp_gradvar_finish", None, None, None, None, None, None, 1, 1, 1, 1, 2, 0, None, None, None, None, None,
                              None, None), -1, "null buffer passed to psp_gradvar_finish"),
        "aff": (lambda: call("psp_aff_query", C.byref(aff), C.byref(nat.AffSizes())),
                -1, "psp_aff_config.struct_bytes is not sizeof(psp_aff_config)"),
        "genl": (lambda: call("psp_genl_eval_query", C.byref(ev), C.byref(nat.GenlEvalSizes())), -1, "K_points must be positive"),
        "is": (lambda: call("psp_is_query", C.byref(isc), C.byref(C.c_int32())), -1, "non-positive d / K / N"),
        "pinn": (lambda: call("psp_pinn_query", C.byref(pinn), C.byref(nat.PinnSizes())), -1, "psp_pinn: d and K must be positive"),
    }


def test_every_unit_reports_through_the_one_error_buffer():
    r = _refusals()
    assert r["gen"][0]() == r["gen"][1:] and r["dnet"][0]() == r["dnet"][1:]
    units = ["common", "hjb", "pinn", "is", "aff", "genl", "dnet", "gen", "common", "is", "hjb", "genl", "pinn", "aff"]
    for first, second in zip(units, units[1:]):                 # 13 pairs of different units, each message replaced by the next
        assert r[first][0]() == r[first][1:], first
        assert r[second][0]() == r[second][1:], (first, second)
        assert nat.last_error() == r[second][2]


# ---- psp_is_query / psp_isw_query: the checks both share, in the order the code makes them ----------------------------------
def is_config(**kw):
    c = nat.IsConfig()
    c.d, c.K_local, c.N, c.control_kind = 4, 32, 4, 0
    c.K_global, c.k_offset, c.dt, c.sqrt_dt = 32, 0, 0.25, 0.5
    c.drift_kind, c.sigma_kind, c.runcost_kind, c.term_kind, c.noise_mode = 2, 1, 1, 0, 1
    c.sigma_scale = 1.0
    c.x0 = c.drift = c.sigma = c.runcost = c.term = PTR
    for k, v in kw.items():
        setattr(c, k, v)
    return c


GRID = dict(control_kind=3, u_ref=PTR, u_group=PTR, u_row=PTR, u_ntables=2, u_nrows=3, u_ncols=5, u_xb=1.0, u_dx=0.5, u_xhi=2.0)
D_IS = "psp_is_rollout: d = %d is outside the native range d <= 64"
D_ISW = ("psp_isw_rollout: d = %d is outside the native range d <= 256 (a wider tile does not fit one wave's registers without "
         "scratch)")
KIND = "control_kind out of range (PSP_ISC_NONE, PSP_ISC_TABLE, PSP_ISC_LINEAR, PSP_ISC_GRID)"
ENUM = "config enum out of range"
KGLOB = "K_global must cover k_offset + K_local"
X0 = "null x0 in psp_is_config"
NCOLS = "u_ntables / u_nrows / u_ncols must be positive"
UDX = "u_xb / u_dx must be positive"
UGROUP = "control kind PSP_ISC_GRID needs u_group and u_row"
BIG_IS = "psp_is_rollout: the coefficient tables and the u* data of one step do not fit the 160 KiB LDS"
BIG_ISW = "psp_isw_rollout: the u* rows of one step do not fit the 160 KiB LDS"
OK = (0, None)

# (config fields, psp_is_query's answer, psp_isw_query's answer -- None: the same); first the single violations, in the code's order
IS_CASES = [
    ("valid", {}, OK, None),
    ("valid_grid", GRID, OK, None),
    ("d_zero", dict(d=0), (-1, "non-positive d / K / N"), None),
    ("d_65", dict(d=65), (-2, D_IS % 65), OK),
    ("d_257", dict(d=257), (-2, D_IS % 257), (-2, D_ISW % 257)),
    ("control_kind_4", dict(control_kind=4), (-1, KIND), None),
    ("drift_kind_4", dict(drift_kind=4), (-1, ENUM), None),
    ("K_global_small", dict(K_global=31), (-1, KGLOB), None),
    ("x0_null", dict(x0=None), (-1, X0), None),
    ("drift_missing", dict(drift=None), (-1, "drift parameters missing"), None),
    ("sigma_missing", dict(sigma=None), (-1, "sigma matrix missing"), None),
    ("runcost_missing", dict(runcost=None), (-1, "running-cost vector missing"), None),
    ("term_missing", dict(term=None), (-1, "terminal-cost vector missing"), None),
    ("table_without_u_ref", dict(control_kind=1), (-1, "control kinds TABLE / LINEAR / GRID need u_ref"), None),
    ("grid_without_u_group", dict(GRID, u_group=None), (-1, UGROUP), None),
    ("grid_ncols_zero", dict(GRID, u_ncols=0), (-1, NCOLS), None),
    ("grid_dx_zero", dict(GRID, u_dx=0.0), (-1, UDX), None),
    ("grid_too_large", dict(GRID, u_ntables=64, u_ncols=1024), (-3, BIG_IS), (-3, BIG_ISW)),
    # two violations at once: the earlier check answers
    ("d_zero+K_global_small", dict(d=0, K_global=31), (-1, "non-positive d / K / N"), None),
    ("d_257+control_kind_4", dict(d=257, control_kind=4), (-2, D_IS % 257), (-2, D_ISW % 257)),
    ("control_kind_4+drift_kind_4", dict(control_kind=4, drift_kind=4), (-1, KIND), None),
    ("drift_kind_4+K_global_small", dict(drift_kind=4, K_global=31), (-1, ENUM), None),
    ("K_global_small+x0_null", dict(K_global=31, x0=None), (-1, KGLOB), None),
    ("x0_null+drift_missing", dict(x0=None, drift=None), (-1, X0), None),
    ("drift_missing+sigma_missing", dict(drift=None, sigma=None), (-1, "drift parameters missing"), None),
    ("runcost_missing+term_missing", dict(runcost=None, term=None), (-1, "running-cost vector missing"), None),
    ("term_missing+table_without_u_ref", dict(term=None, control_kind=1), (-1, "terminal-cost vector missing"), None),
    ("grid_without_u_group+too_large", dict(GRID, u_group=None, u_ntables=64, u_ncols=1024), (-1, UGROUP), None),
    ("grid_ncols_zero+dx_zero", dict(GRID, u_ncols=0, u_dx=0.0), (-1, NCOLS), None),
    ("grid_dx_zero+too_large", dict(GRID, u_dx=0.0, u_ntables=64, u_ncols=1024), (-1, UDX), None),
]


@pytest.mark.parametrize("fields,want_is,want_isw", [c[1:] for c in IS_CASES], ids=[c[0] for c in IS_CASES])
def test_is_and_isw_query_fire_their_checks_in_order(fields, want_is, want_isw):
    cfg = is_config(**fields)
    for name, out, want in (("psp_is_query", C.c_int32(), want_is), ("psp_isw_query", nat.IswSizes(), want_isw or want_is)):
        call("psp_pinn_query", None, C.byref(nat.PinnSizes()))                                  # "null config", from another unit
        rc, msg = call(name, C.byref(cfg), C.byref(out))
        assert rc == want[0], (name, msg)
        assert msg == (want[1] if rc else "null config")                                        # success leaves the buffer alone


def test_isw_query_checks_its_sizes_struct_before_the_config():
    s = nat.IswSizes()
    s.struct_bytes = 8
    assert call("psp_isw_query", None, C.byref(s)) == (-1, "psp_isw_sizes.struct_bytes = 8, the library's struct has 24 bytes")
    assert call("psp_isw_query", None, None) == (-1, "null sizes passed to psp_isw_query")
    s = nat.IswSizes()
    assert call("psp_isw_query", C.byref(is_config(d=200)), C.byref(s))[0] == 0
    assert (s.struct_bytes, s.lds_bytes, s.workgroups, s.max_d) == (24, 0, 1, 256) and s.table_bytes > 0
