"""utilities.do_importance_sampling_me with simulate_naive=True, control='true' and cross_statistics (reference
utilities.py:287-359) on the composite plan, against the reference's own outputs (tests/golden/make_golden_is_naive.py);
argument handling of psp_is_rollout and the resources of its kernel instances.  No GPU needed."""
import contextlib
import ctypes as C
import glob
import io
import math
import os
import re
import struct

import pytest
import torch

from conftest import load_golden
from util_cases import make_pkg_solver, psp

nat = psp.native
GOLDEN = ["is_naive_dw1d_true", "is_naive_dw4_true", "is_naive_llgc6_true", "is_naive_lqgc3_true", "is_naive_llgc20_approx"]


def _run(name, backend="auto", K=None):
    rec = load_golden(name)
    case = rec["case"]
    torch.set_num_threads(1)
    model = make_pkg_solver(case, "cpu", backend=backend)
    model.train()
    torch.manual_seed(case["is_seed"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = psp.do_importance_sampling_me(model.problem, model, K or case["is_K"], control=case["control"], simulate_naive=True,
                                            verbose=True, delta_t=case["is_delta_t"], cross_statistics=torch.tensor(case["cross"]))
    return rec, out, buf.getvalue()


@pytest.mark.parametrize("name", GOLDEN)
def test_composite_matches_reference(name):
    rec, out, text = _run(name)
    exp = rec["expected"]
    keys = ["mean_naive", "variance_naive", "rel_error_naive", "mean_IS", "variance_IS", "rel_error_IS"]
    assert len(out) == 6
    # bit for bit on the torch build that made the fixture -- except the IS triple of the LLGC cases: the package's LLGC forms
    # u*(t) = -B' expm(A' (T - t)) alpha (and trains the learned control) with its own matrix arithmetic, which differs from the
    # reference's in the last bits; the naive triple and every other case are exact
    if rec["torch"] == torch.__version__:
        exact = keys[:3] if name.startswith("is_naive_llgc") else keys
        assert [out[keys.index(k)] for k in exact] == [exp[k] for k in exact]
        if exact == keys:
            assert text == exp["printed"]
    for k, got in zip(keys, out):
        assert math.isclose(got, exp[k], rel_tol=1e-5 if k.startswith("mean") else 1e-4), (k, got, exp[k])
    crossed = [int(m) for m in re.findall(r"crossed: (\d+)/", text)]
    assert crossed == [exp["crossed_naive"], exp["crossed_IS"]]


def test_return_arity_and_verbose_format(capsys):
    prob = psp.LLGC(d=2, off_diag=0.1, T=0.1, seed=1, device="cpu")
    model = psp.Solver("x", prob, L=0, K=8, delta_t=0.05, time_approx="inner", verbose=False, device="cpu")
    torch.manual_seed(0)
    three = psp.do_importance_sampling_me(prob, model, 64, control="true", verbose=True, delta_t=0.05)
    lines = capsys.readouterr().out.splitlines()
    assert len(three) == 3 and len(lines) == 1
    assert re.fullmatch(r"IS mean: \S+e[+-]\d\d, IS variance: \S+e[+-]\d\d, IS RE \S+e[+-]\d\d", lines[0])
    six = psp.do_importance_sampling_me(prob, model, 64, simulate_naive=True, verbose=True, delta_t=0.05,
                                        cross_statistics=torch.tensor([[0.0]]))
    lines = capsys.readouterr().out.splitlines()
    assert len(six) == 6 and len(lines) == 2
    assert re.fullmatch(r"naive mean: \S+, naive variance: \S+, naive RE \S+, crossed: \d+/64", lines[0])
    assert re.fullmatch(r"IS mean: \S+, IS variance: \S+, IS RE \S+, crossed: \d+/64", lines[1])
    with pytest.raises(NotImplementedError):
        psp.do_importance_sampling_me(prob, model, 64, on_cpu=True)


def test_native_backend_on_cpu_raises_with_reason():
    prob = psp.DoubleWell(d=1, T=0.1, eta=3.0, kappa=5.0, device="cpu")
    prob.compute_reference_solution()
    model = psp.Solver("x", prob, L=0, K=8, delta_t=0.01, time_approx="inner", verbose=False, device="cpu", backend="native")
    with pytest.raises(NotImplementedError) as e:
        psp.do_importance_sampling_me(prob, model, 64, control="true", simulate_naive=True)
    assert "native IS evaluation unavailable: the model is not on a GPU" in str(e.value)


@pytest.fixture(scope="module")
def lib():
    if not nat.is_built():
        import __graft_entry__
        __graft_entry__.build()
    return nat.load()


def test_is_rollout_validates_arguments(lib):
    cfg = nat.IsConfig()
    cfg.d, cfg.K_local, cfg.N, cfg.K_global = 1, 16, 10, 16
    assert lib.psp_is_rollout(C.byref(cfg), None, 1, 0, None, None, None) == -1 and "null" in nat.last_error()
    cfg.d = 70
    assert lib.psp_is_rollout(C.byref(cfg), None, 1, 0, None, None, None) == -2 and "native range" in nat.last_error()
    assert lib.psp_is_query(C.byref(cfg), None) == -2
    cfg.d, cfg.control_kind = 1, 9
    assert lib.psp_is_rollout(C.byref(cfg), None, 1, 0, None, None, None) == -1 and "control_kind" in nat.last_error()
    cfg.control_kind, cfg.K_global = nat.ISC_NONE, 8
    assert lib.psp_is_rollout(C.byref(cfg), None, 1, 0, None, None, None) == -1 and "K_global" in nat.last_error()
    sizes = (C.c_int32 * 1)()
    assert lib.psp_abi_struct_sizes3(C.byref(sizes)) == 0 and sizes[0] == C.sizeof(nat.IsConfig)


def _kernel_descriptors(obj_path):
    """(name, private_segment_fixed_size, vgprs) of every hjbe kernel in the gfx950 code object bundled into a host object."""
    blob = open(obj_path, "rb").read()
    out = []
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    pos = blob.find(magic)
    assert pos >= 0, "no offload bundle in %s" % obj_path
    n = struct.unpack_from("<Q", blob, pos + 24)[0]
    p = pos + 32
    for _ in range(n):
        off, size, idlen = struct.unpack_from("<QQQ", blob, p)
        ident = blob[p + 24:p + 24 + idlen].decode()
        p += 24 + idlen
        if "gfx950" not in ident:
            continue
        elf = blob[pos + off:pos + off + size]
        shoff, = struct.unpack_from("<Q", elf, 0x28)
        shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
        secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
        symtab = next(s for s in secs if s[1] == 2)                   # SHT_SYMTAB
        strtab = secs[symtab[6]]
        for i in range(symtab[5] // 24):
            st_name, _, _, st_shndx, st_value, _ = struct.unpack_from("<IBBHQQ", elf, symtab[4] + 24 * i)
            name = elf[strtab[4] + st_name:elf.index(b"\0", strtab[4] + st_name)].decode()
            if name.endswith(".kd") and "hjbe_rollout_kernel" in name:
                sec = secs[st_shndx]
                kd = sec[4] + (st_value - sec[3])                     # file offset of the 64-byte kernel descriptor
                private = struct.unpack_from("<I", elf, kd + 4)[0]
                rsrc1 = struct.unpack_from("<I", elf, kd + 48)[0]
                out.append((name, private, ((rsrc1 & 0x3F) + 1) * 8))
    return out


def test_no_instance_has_a_private_segment(lib):
    objs = glob.glob(os.path.join(os.path.dirname(nat.LIB_PATH), "build", "hjbe_inst.o"))
    assert objs, "build() leaves csrc/build/hjbe_inst.o"
    kds = _kernel_descriptors(objs[0])
    assert len(kds) == 5 * 4, kds                                     # d buckets 1, 4, 16, 32, 64 x four control kinds
    for name, private, vgprs in kds:
        assert private == 0, (name, private)


def test_is_query_reports_the_lds_budget(lib):
    """psp_is_query holds every check of psp_is_rollout (the caller asks it before any draw): the LDS of a d = 64 rollout with
    dense A, B and gains, and the refusal of grid rows that do not fit."""
    keep = (C.c_float * 8)()
    cfg = nat.IsConfig()
    cfg.d, cfg.K_local, cfg.N, cfg.K_global = 64, 1024, 10, 1024
    cfg.x0 = cfg.term = cfg.drift = cfg.sigma = cfg.u_ref = C.cast(keep, C.c_void_p)
    cfg.drift_kind, cfg.sigma_kind, cfg.control_kind = nat.DRIFT_DENSE, nat.SIGMA_DENSE, nat.ISC_LINEAR
    lds = C.c_int32()
    assert lib.psp_is_query(C.byref(cfg), C.byref(lds)) == 0
    assert lds.value == 4 * (4 * 64 + 3 * 64 * 64 + 64 * 256)         # vectors, A, B, M_n, the lane-private column
    cfg.drift_kind, cfg.sigma_kind, cfg.control_kind = nat.DRIFT_DOUBLE_WELL, nat.SIGMA_IDENTITY, nat.ISC_GRID
    cfg.u_group = cfg.u_row = C.cast(keep, C.c_void_p)
    cfg.u_ntables, cfg.u_nrows, cfg.u_ncols, cfg.u_xb, cfg.u_dx = 2, 10, 999, 2.5, 0.005
    assert lib.psp_is_query(C.byref(cfg), C.byref(lds)) == 0 and lds.value == 4 * (4 * 64 + 2 * 999)
    cfg.u_ncols = 30000
    assert lib.psp_is_query(C.byref(cfg), C.byref(lds)) == -3 and "LDS" in nat.last_error()
