"""Launch plans of libpsp_hip.so against a recorded table (host only: the size queries need no GPU).

Every launch entry point plans through the same code as its size query, and the sizes expose the choices: workgroup counts,
cooperative tiles, waves per tile, slices, whether the hand-written backward covers an instance.  `rows()` walks a grid of
configurations over every compiled instance -- K on both sides of each selection threshold at 256 CUs (1024 / 1040: quad forward;
8192 / 8208: feature-split forward; 16368 / 16384: four cooperative tiles, genl 4 x CUs tiles), every mlp_dtype a family takes,
both noise modes, store_path 1 / 2 / 4, range_flag null and set -- and tests/golden/launch_plans_256cu.json holds what the
library answered when the table was recorded: every field of the sizes struct, or the return code and psp_last_error().
Dimensions a family's plan ignores are swept at one K only, and equal answers are stored once (`rows` indexes `answers`).

Host refactors of the C ABI layer (csrc/api_*.hip, where each family's planner lives) must leave this table as it is.  A deliberate change of a selection rule re-records it:

    python tests/test_launch_plan_golden.py --record
"""
import ctypes as C
import hashlib
import json
import os
import sys

import pytest
import torch

from conftest import GOLDEN_DIR
from util_cases import psp

nat = psp.native
GOLDEN = os.path.join(GOLDEN_DIR, "launch_plans_256cu.json")
KS = (16, 1024, 1040, 8192, 8208, 16368, 16384, 65536)
K_ONE = 16384                    # where the dimensions that do not move a grid are swept
PTR = 0x1000                     # a non-null pointer: no query dereferences one
SWITCHES = ("PSP_FWD_COOP", "PSP_FWD_VARIANT", "PSP_GENL_NW", "PSP_FORCE_WIDE")


def _hjb(d, H, K, mlp=nat.MLP_FP32, noise=nat.NOISE_PHILOX, sp=1, flag=0, **kw):
    c = nat.HjbConfig(d=d, H=H, K_local=K, N=50, K_global=K, dt=0.01, sqrt_dt=0.1, drift_kind=nat.DRIFT_DENSE,
                      sigma_kind=nat.SIGMA_DENSE, term_kind=nat.TERM_DIAG_QUAD, adaptive=1, noise_mode=noise, store_path=sp,
                      sigma_scale=1.0, mlp_dtype=mlp, range_flag=PTR if flag else None)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _gen(d, H, K, mlp=nat.MLP_FP32, noise=nat.NOISE_PHILOX, sp=1, flag=0, **kw):
    c = nat.GenConfig(d=d, H=H, K_local=K, N=25, dt=0.01, sqrt_dt=0.1, T=0.25, sigma_scale=1.0, noise_mode=noise, store_path=sp,
                      mlp_dtype=mlp, range_flag=PTR if flag else None)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _genl(d, K, widths, sigma_kind, noise=nat.NOISE_PHILOX, sp=1, **kw):
    c = nat.GenlConfig(base=_gen(d, 0, K, noise=noise, sp=sp, **kw), has_time=1, n_hidden=len(widths), activation=nat.ACT_TANH,
                       time_scale=1.0, sigma_kind=sigma_kind, sigma=PTR if sigma_kind == nat.GENL_SIGMA_DENSE else None)
    for i, w in enumerate(widths):
        c.widths[i] = w
    return c


NETS = [(16,), (128,), (16,) * 4, (128,) * 4]


def _sweep(mlps, flag_mlp):
    """(mlp, noise, store_path, flag) at one K: every value of each, the flag only where the family reads it."""
    for mlp in mlps:
        for noise in (nat.NOISE_SUPPLIED, nat.NOISE_PHILOX):
            for sp in (1, 2, 4):
                for flag in ((0, 1) if mlp == flag_mlp else (0,)):
                    yield mlp, noise, sp, flag


def rows():
    """[(key, query symbol, config, sizes object)] in a fixed order."""
    out = []
    # ---- HJB rollout (psp_hjb_query): quad / feature-split / tile-per-wave / cooperative forward, backward grid
    hjb_mlps = (nat.MLP_FP32, nat.MLP_BF16_FWD, nat.MLP_F16X3)
    for d, H, fam in nat.instances():
        if fam == 2 and nat.family(d, H) != 2:
            continue                                       # (a wide twin of a narrow instance: served under PSP_FORCE_WIDE only)
        for mlp in hjb_mlps:
            for K in KS:
                out.append(("hjb %d %d K%d m%d" % (d, H, K, mlp), "psp_hjb_query", _hjb(d, H, K, mlp), nat.HjbSizes()))
        for mlp, noise, sp, flag in _sweep(hjb_mlps, nat.MLP_F16X3):
            out.append(("hjb %d %d m%d n%d s%d f%d" % (d, H, mlp, noise, sp, flag), "psp_hjb_query",
                        _hjb(d, H, K_ONE, mlp, noise, sp, flag), nat.HjbSizes()))
        for name, kw in (("runcost", dict(runcost_kind=nat.RUNCOST_DIAG_QUAD)), ("uref", dict(u_ref=PTR, u_l2_out=PTR)),
                         ("plain", dict(drift_kind=nat.DRIFT_ZERO, sigma_kind=nat.SIGMA_IDENTITY)),
                         ("s4 nonadaptive", dict(store_path=4, adaptive=0))):
            out.append(("hjb %d %d %s" % (d, H, name), "psp_hjb_query", _hjb(d, H, K_ONE, nat.MLP_F16X3, flag=1, **kw),
                        nat.HjbSizes()))
    for name, cfg in (("no instance", _hjb(7, 30, 1024)), ("K 0", _hjb(100, 64, 0)), ("drift_kind 4", _hjb(100, 64, 1024, drift_kind=4)),
                      ("store_path 5", _hjb(100, 64, 1024, sp=5)), ("loss_kind 4", _hjb(100, 64, 1024, loss_kind=4)),
                      ("N K 2^31", _hjb(100, 64, 1 << 30, N=64))):
        out.append(("hjb " + name, "psp_hjb_query", cfg, nat.HjbSizes()))
    # ---- GeneralSolver (psp_gen_query): the plan reads K and the matrix mode
    gen_mlps = (nat.MLP_FP32, nat.MLP_BF16_FWD, nat.MLP_BF16, nat.MLP_F16X3)
    for d, H in nat.gen_instances():
        for mlp in gen_mlps:
            for K in KS:
                out.append(("gen %d %d K%d m%d" % (d, H, K, mlp), "psp_gen_query", _gen(d, H, K, mlp), nat.GenSizes()))
        for mlp, noise, sp, flag in _sweep((nat.MLP_F16X3,), nat.MLP_F16X3):
            out.append(("gen %d %d m%d n%d s%d f%d" % (d, H, mlp, noise, sp, flag), "psp_gen_query",
                        _gen(d, H, K_ONE, mlp, noise, sp, flag), nat.GenSizes()))
        out.append(("gen %d %d s0" % (d, H), "psp_gen_query", _gen(d, H, K_ONE, sp=0), nat.GenSizes()))
    for name, cfg in (("no instance", _gen(7, 30, 1024)), ("h_kind 9", _gen(100, 64, 1024, h_kind=9)),
                      ("sphere r 0", _gen(100, 64, 1024, domain_kind=nat.DOM_SPHERE))):
        out.append(("gen " + name, "psp_gen_query", cfg, nat.GenSizes()))
    # ---- DenseNet controls (psp_dnet_query): slices and backward grid from N and K
    for d, H in nat.dnet_instances():
        def dnet(K, mlp=nat.MLP_FP32, noise=nat.NOISE_PHILOX, sp=1, flag=0, **kw):
            c = nat.DnetConfig(base=_hjb(d, H, K, mlp, noise, sp, flag), d_real=d - 3, H_real=H - 2, time_input=1)
            for k, v in kw.items():
                setattr(c, k, v)
            return c
        for mlp in (nat.MLP_FP32, nat.MLP_F16X3):
            for K in KS:
                out.append(("dnet %d %d K%d m%d" % (d, H, K, mlp), "psp_dnet_query", dnet(K, mlp), nat.DnetSizes()))
        for mlp, noise, sp, flag in _sweep((nat.MLP_FP32, nat.MLP_F16X3), nat.MLP_F16X3):
            out.append(("dnet %d %d m%d n%d s%d f%d" % (d, H, mlp, noise, sp, flag), "psp_dnet_query",
                        dnet(K_ONE, mlp, noise, sp, flag), nat.DnetSizes()))
        for name, kw in (("per_step", dict(per_step=1)), ("ul2 linear", dict(ul2_kind=nat.UL2_LINEAR, ul2_tables=PTR)),
                         ("ul2 linear no out", dict(ul2_kind=nat.UL2_LINEAR, ul2_tables=PTR, no_out=1)), ("d_real 0", dict(d_real=0))):
            c = dnet(K_ONE, **{k: v for k, v in kw.items() if k != "no_out"})
            c.base.u_l2_out = None if "no_out" in kw else PTR
            out.append(("dnet %d %d %s" % (d, H, name), "psp_dnet_query", c, nat.DnetSizes()))
    # ---- value nets of any depth (psp_genl_query): one or eight waves per tile, four in the forward at 2 x CUs tiles
    for widths in NETS:
        for sk in (nat.GENL_SIGMA_SCALED, nat.GENL_SIGMA_DENSE):
            tag = "genl %dx%d sk%d" % (len(widths), widths[0], sk)
            for K in KS:
                out.append(("%s K%d" % (tag, K), "psp_genl_query", _genl(10, K, widths, sk), nat.GenlSizes()))
            for noise in (nat.NOISE_SUPPLIED, nat.NOISE_PHILOX):
                for sp in (0, 2, 4):
                    out.append(("%s n%d s%d" % (tag, noise, sp), "psp_genl_query", _genl(10, K_ONE, widths, sk, noise, sp),
                                nat.GenlSizes()))
    for name, cfg in (("d100", _genl(100, K_ONE, (64, 64), 0)), ("d112 wide input", _genl(112, K_ONE, (16,), 0)),
                      ("width 129", _genl(10, K_ONE, (129,), 0)), ("too big for LDS", _genl(100, K_ONE, (128,) * 4, 1))):
        out.append(("genl " + name, "psp_genl_query", cfg, nat.GenlSizes()))
    # ---- K_test_log evaluation (psp_genl_eval_query): the waves-per-tile rule on K_points
    for widths in NETS:
        for K in KS:
            c = nat.GenlEvalConfig(d=10, has_time=1, n_hidden=len(widths), activation=nat.ACT_TANH, time_scale=1.0, K_points=K,
                                   sample_kind=nat.TSAMPLE_BALL, bound_b=1.0, T=1.0, log_slots=4)
            for i, w in enumerate(widths):
                c.widths[i] = w
            out.append(("eval %dx%d K%d" % (len(widths), widths[0], K), "psp_genl_eval_query", c, nat.GenlEvalSizes()))
    out.append(("eval log_slots 0", "psp_genl_eval_query",
                nat.GenlEvalConfig(d=10, n_hidden=1, K_points=16, sample_kind=nat.TSAMPLE_BALL, bound_b=1.0), nat.GenlEvalSizes()))
    # ---- importance sampling (psp_is_query): the LDS carve of (d bucket, control kind, dense drift / sigma)
    for d in (1, 16, 17, 64, 65):
        for ctrl in (nat.ISC_NONE, nat.ISC_TABLE, nat.ISC_LINEAR, nat.ISC_GRID):
            for drift in (nat.DRIFT_ZERO, nat.DRIFT_DENSE):
                for sigma in (nat.SIGMA_IDENTITY, nat.SIGMA_DENSE):
                    c = nat.IsConfig(d=d, K_local=1040, N=50, control_kind=ctrl, K_global=1040, dt=0.01, sqrt_dt=0.1, drift_kind=drift,
                                     sigma_kind=sigma, term_kind=nat.TERM_DIAG_QUAD, noise_mode=nat.NOISE_PHILOX, sigma_scale=1.0,
                                     x0=PTR, drift=PTR, sigma=PTR, term=PTR, u_ref=PTR, u_group=PTR, u_row=PTR,
                                     u_ntables=3, u_nrows=d, u_ncols=129, u_xb=4.0, u_dx=0.0625, u_xhi=4.0)
                    out.append(("is %d c%d a%d s%d" % (d, ctrl, drift, sigma), "psp_is_query", c, C.c_int32()))
    big = nat.IsConfig(d=16, K_local=16, N=5, control_kind=nat.ISC_GRID, K_global=16, dt=0.01, sqrt_dt=0.1, noise_mode=1, x0=PTR, term=PTR,
                       u_ref=PTR, u_group=PTR, u_row=PTR, u_ntables=64, u_nrows=16, u_ncols=1025, u_xb=4.0, u_dx=0.0078125, u_xhi=4.0)
    out.append(("is grid too big", "psp_is_query", big, C.c_int32()))
    out.append(("is sigma_kind 3", "psp_is_query", nat.IsConfig(d=16, K_local=16, N=5, K_global=16, sigma_kind=3, x0=PTR, term=PTR),
                C.c_int32()))
    return out


def _fields(sizes):
    if not isinstance(sizes, C.Structure):
        return [sizes.value]
    vals = []
    for name, _ in sizes._fields_:
        v = getattr(sizes, name)
        vals.extend(list(v) if isinstance(v, C.Array) else [v])
    return vals


def answer(symbol, cfg, sizes):
    """Every field of the sizes struct, or [return code, message]."""
    lib = nat.load()
    rc = getattr(lib, symbol)(C.byref(cfg), C.byref(sizes))
    return [rc, lib.psp_last_error().decode()] if rc else _fields(sizes)


def _grid_digest(grid):
    return hashlib.sha256("\n".join(r[0] for r in grid).encode()).hexdigest()


def _visible_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def record():
    for name in SWITCHES:
        os.environ.pop(name, None)
    assert _visible_cus() == 256
    grid = rows()
    answers, index, which = [], {}, []
    for key, symbol, cfg, sizes in grid:
        a = answer(symbol, cfg, sizes)
        which.append(index.setdefault(json.dumps(a), len(answers)))
        if which[-1] == len(answers):
            answers.append(a)
    with open(GOLDEN, "w") as fh:
        fh.write('{"cus":256,"grid_sha256":"%s",\n"answers":[\n%s\n],\n"rows":%s}\n'
                 % (_grid_digest(grid), ",\n".join(json.dumps(a, separators=(",", ":")) for a in answers),
                    json.dumps(which, separators=(",", ":"))))
    print("%d rows, %d distinct answers, %d bytes" % (len(grid), len(answers), os.path.getsize(GOLDEN)))


def test_size_queries_answer_as_recorded(monkeypatch):
    cus = _visible_cus()
    if cus != 256:
        pytest.skip("the table was recorded for 256 CUs; this device has %d" % cus)
    if os.environ.get("PSP_FORCE_WIDE", "0")[:1] == "1":
        pytest.skip("PSP_FORCE_WIDE=1 (read once per process) serves other instances than the recorded ones")
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    with open(GOLDEN) as fh:
        gold = json.load(fh)
    grid = rows()
    assert gold["cus"] == 256 and len(gold["rows"]) == len(grid) and gold["grid_sha256"] == _grid_digest(grid), \
        "rows() no longer walks the grid the table was recorded on"
    wrong = []
    for (key, symbol, cfg, sizes), i in zip(grid, gold["rows"]):
        got = answer(symbol, cfg, sizes)
        if got != gold["answers"][i]:
            wrong.append((key, got, gold["answers"][i]))
    assert not wrong, "%d of %d rows differ, first (row, answer, recorded): %r" % (len(wrong), len(grid), wrong[:5])


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        record()
