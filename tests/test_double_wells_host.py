"""DoubleWell_OU, DoubleWell_multidim_2, DoubleWell_multidim_3 and LLGC_general_f without a GPU: the classes against the
reference's recorded probes and fixed-seed runs (tests/golden/wells_*.json, composite plan), their native_spec(), which plan
declines them and why, and the per-step u_L2 tables of DoubleWell_OU against problem.u_true."""
import glob
import math
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from util_cases import make_pkg_problem, make_pkg_solver, psp

nat = psp.native
pc = psp.plan_common
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(GOLDEN, "wells_*.json")))
ONE_PER_PROBLEM = ["wells_ou_d3_default", "wells_ou_d20_default", "wells_dw3_d5_default", "wells_radial_d4_default",
                   "wells_radial_d20_default", "wells_llgc_general_f_d3"]


# tests/test_plan_gloo_product.py routes the native plan to CPU stand-ins (tests/fake_kernels.install) and leaves that in place for
# the rest of the process.  The runs here must see the real eligibility checks and the real library whatever ran before: the
# originals -- taken from the defining modules when this file is collected, before any test runs -- are put back for every test.
_REAL = dict(eligibility=psp.plan_native.native_eligibility, load=nat.load)
assert _REAL["eligibility"].__module__ == psp.plan_native.__name__ and _REAL["load"].__module__ == nat.__name__


@pytest.fixture(autouse=True)
def real_routing(monkeypatch):
    monkeypatch.setattr(psp.plan_native, "native_eligibility", _REAL["eligibility"])
    monkeypatch.setattr(psp.solver, "native_eligibility", _REAL["eligibility"])
    monkeypatch.setattr(nat, "load", _REAL["load"])


def test_the_goldens_are_all_there():
    assert len(CASES) == 21 and set(ONE_PER_PROBLEM) <= set(CASES)


def test_the_four_classes_import_like_the_reference():
    import importlib
    import sys
    sys.path.insert(0, os.path.dirname(psp.problems.__file__))
    try:
        flat = importlib.import_module("problems")
        for name in ("DoubleWell_OU", "DoubleWell_multidim_2", "DoubleWell_multidim_3", "LLGC_general_f"):
            assert hasattr(flat, name) and hasattr(psp, name)
    finally:
        sys.path.pop(0)


@pytest.mark.parametrize("name", CASES)
def test_composite_plan_matches_reference(name):
    """As tests/test_composite_golden.py: equal logs on the torch build of the fixtures (detached runs), 1e-5 otherwise."""
    rec = load_golden(name)
    exact = rec["torch"] == torch.__version__ and rec["case"]["solver"].get("detach_forward", False)
    torch.set_num_threads(1)
    model = make_pkg_solver(rec["case"], "cpu")
    model.train()
    assert model.plan_name == "torch"
    exp = rec["expected"]
    assert model.N == exp["N"] and int(model.p) == exp["p"]
    assert len(model.loss_log) == len(exp["loss_log"])
    for got, want in zip(model.loss_log, exp["loss_log"]):
        assert (got == want) if exact else math.isclose(got, want, rel_tol=1e-5)
    if any(v != 0 for v in exp["u_L2_loss"]):
        assert len(model.u_L2_loss) == len(exp["u_L2_loss"])
        for got, want in zip(model.u_L2_loss, exp["u_L2_loss"]):
            assert math.isclose(got, want, rel_tol=1e-5)
    xp = torch.tensor(exp["probe_x"]).reshape(-1, model.d)
    for pr in exp["probes"]:
        with torch.no_grad():
            u = -model.Z_n(xp, pr["t"])
        # (LLGC_general_f: the reference's own parameters are NaN after its first step, and so is the recorded control)
        assert torch.allclose(u, torch.tensor(pr["minus_Z"]).reshape(u.shape), rtol=1e-5, atol=1e-7, equal_nan=True)


@pytest.mark.parametrize("name", ONE_PER_PROBLEM)
def test_coefficient_functions_match_the_recorded_probes(name):
    rec = load_golden(name)
    pb = make_pkg_problem(rec["case"]["problem"], "cpu")
    pr = rec["expected"]["problem_probes"]
    x = torch.tensor(pr["x"]).reshape(-1, pb.d)
    z = torch.tensor(pr["z"]).reshape(-1, pb.d)
    t = torch.tensor(pr["t"])
    assert torch.equal(pb.X_0.cpu(), torch.tensor(pr["X_0"]))
    for key, got in (("b", pb.b(x)), ("g", pb.g(x)), ("h", pb.h(t, x, torch.zeros(x.shape[0]), z)), ("f", pb.f(x, t))):
        want = torch.tensor(pr[key]).reshape(got.shape)
        assert torch.allclose(got, want, rtol=1e-6, atol=1e-7), key
    if pr["u_true"] is not None:
        u = np.asarray(pb.u_true(x, pr["t"]), dtype=np.float64)
        assert list(u.shape) == pr["u_true_shape"]
        assert np.allclose(u.reshape(-1), np.array(pr["u_true"]), rtol=1e-6, atol=1e-9)


def test_reference_tables_match_the_reference():
    for name in ("wells_ou_d3_default", "wells_dw3_d5_default"):
        rec = load_golden(name)
        pb = make_pkg_problem(rec["case"]["problem"], "cpu")
        (w,) = rec["expected"]["ref_tables"]
        assert list(pb.u.shape) == w["shape"]
        probe = pb.u[::max(1, pb.u.shape[0] // 3), ::max(1, pb.u.shape[1] // 5)].reshape(-1)
        assert np.allclose(probe, np.array(w["probe"]), rtol=1e-6, atol=1e-9)
        assert math.isclose(float(pb.u.sum()), w["sum"], rel_tol=1e-6, abs_tol=1e-6)


def test_native_spec_contents():
    ou = psp.DoubleWell_OU(d=4, T=0.2, alpha=0.5, kappa=2.0, device="cpu").native_spec()
    assert ou["drift"][0] == nat.DRIFT_WELL_DIAG == 8 and ou["term"][0] == nat.TERM_QUAD_LINEAR == 8 and ou["split"] == 1
    assert ou["drift"][1].tolist() == [2.0, -5.0, -5.0, -5.0] and ou["term"][1].tolist() == [0.5, 1.0, 1.0, 1.0]
    assert ou["sigma"][0] == nat.SIGMA_IDENTITY and ou["runcost"][0] == nat.RUNCOST_ZERO
    ra = psp.DoubleWell_multidim_2(d=7, T=0.2, alpha=0.5, kappa=2.0, device="cpu").native_spec()
    assert ra["drift"][0] == nat.DRIFT_RADIAL_WELL == 9 and ra["term"][0] == nat.TERM_RADIAL_QUAD == 9
    assert ra["drift"][1].tolist() == [2.0, 3.0, 1.0] and ra["term"][1].tolist() == [0.5, 2.0]
    d3 = psp.DoubleWell_multidim_3(d=3, T=0.2, eta=0.5, kappa=2.0, device="cpu")
    s3 = d3.native_spec()
    assert s3["drift"][0] == nat.DRIFT_DOUBLE_WELL and s3["term"][0] == nat.TERM_SHIFTED_QUAD and "split" not in s3
    assert s3["drift"][1].tolist() == [2.0] * 3 and s3["term"][1].tolist() == [0.5] * 3
    d3.compute_reference_solution(nx=100)
    assert d3.u_true_tables()["group_of_dim"] == [0, 0, 0] and len(d3.u_true_tables()["tables"]) == 1
    assert not hasattr(psp.LLGC_general_f(d=2, T=0.2, device="cpu"), "native_spec")


def test_pad_coeff_gives_the_kernels_a_full_width_buffer():
    """The kernels stage d floats of drift / term whatever the kind: a radial parameter vector is padded, never passed short."""
    pad = psp.native_shapes.ParamPad(4, 30, 16, 32, torch.device("cpu"))
    assert pc.pad_coeff(pad, torch.tensor([1.0, 3.0, 1.0])).tolist() == [1.0, 3.0, 1.0] + [0.0] * 13
    assert pc.pad_coeff(pad, torch.tensor([1.0, 2.0, 3.0, 4.0])).tolist() == [1.0, 2.0, 3.0, 4.0] + [0.0] * 12
    same = psp.native_shapes.ParamPad(16, 32, 16, 32, torch.device("cpu"))
    assert pc.pad_coeff(same, torch.tensor([1.0, 2.0])).numel() == 16
    assert pc.pad_coeff(same, torch.eye(16)).shape == (16, 16)


def _on_gpu(model):
    model.device = torch.device("cuda")          # only its type is read by the eligibility functions; nothing runs on it
    return model


def _solver(pb, **kw):
    kw.setdefault("u_l2_error_flag", False)
    return psp.Solver("w", pb, L=1, K=16, delta_t=0.05, verbose=False, device="cpu", **kw)


@pytest.mark.parametrize("make", [lambda: psp.DoubleWell_OU(d=3, T=0.2, device="cpu"),
                                  lambda: psp.DoubleWell_multidim_2(d=4, T=0.2, device="cpu")])
def test_the_other_plans_decline_with_a_reason_that_names_the_family(make):
    pb = make()
    assert psp.plan_dense_native.dense_eligibility(_on_gpu(_solver(pb))) is None
    inner = _on_gpu(_solver(pb, time_approx="inner"))
    assert "DenseNet-control" in psp.plan_native.native_eligibility(inner)
    value = _on_gpu(_solver(pb, approx_method="value_function", time_approx="inner", detach_forward=True))
    assert "DenseNet-control" in psp.plan_value_native.value_eligibility(value)
    lin = _solver(pb)
    lin.z_n = [psp.function_space.Linear(pb.d, pb.B, torch.eye(pb.d), 0.01) for _ in range(lin.N)]
    lin.update_Phis()
    _on_gpu(lin)
    assert "DenseNet-control" in psp.plan_affine_native.affine_eligibility(lin)
    assert "DenseNet-control" in psp.utilities._native_reason(pb, inner, "approx", False)
    assert "DenseNet-control" in psp.utilities._coeff_reason(pb, lin)
    assert "DenseNet-control" in psp.utilities._affine_is_reason(pb, lin)
    assert psp.utilities._dense_reason(pb, _on_gpu(_solver(pb))) is None
    gv = _on_gpu(_solver(pb, compute_gradient_variance=1))
    assert "compute_gradient_variance" in psp.plan_dense_native.dense_eligibility(gv)


def test_wells_3_stays_in_every_family_it_was_in():
    pb = psp.DoubleWell_multidim_3(d=3, T=0.2, device="cpu")
    assert psp.plan_dense_native.dense_eligibility(_on_gpu(_solver(pb))) is None
    assert psp.plan_native.native_eligibility(_on_gpu(_solver(pb, time_approx="inner"))) is None


def test_llgc_general_f_runs_on_the_composite_plan_with_its_reason():
    pb = psp.LLGC_general_f(d=3, off_diag=0.1, T=0.2, device="cpu")
    why = psp.plan_dense_native.dense_eligibility(_on_gpu(_solver(pb)))
    assert "h is not -|z|^2 / 2" in why
    assert "h is not -|z|^2 / 2" in psp.plan_native.native_eligibility(_on_gpu(_solver(pb, time_approx="inner")))


def test_radial_u_l2_flag_raises_as_the_reference_does():
    """problems.py:726-727 returns zeros(x.shape) = (K, d); the log line transposes it against the (K, d) control (solver.py:493)."""
    pb = psp.DoubleWell_multidim_2(d=4, T=0.2, device="cpu")
    why = psp.plan_dense_native.dense_eligibility(_on_gpu(_solver(pb, u_l2_error_flag=True)))
    assert "u_l2_error_flag=False" in why
    with pytest.raises(RuntimeError, match="must match the size"):
        _solver(pb, u_l2_error_flag=True).train()


@pytest.mark.parametrize("d,N,dt", [(3, 4, 0.05), (20, 4, 0.05), (5, 7, 0.03)])
def test_ou_step_tables_reproduce_u_true(d, N, dt):
    """ul2_reference's per-step tables, read with the kernel's cell arithmetic (tests/ref64_wells.grid_control), against
    problem.u_true in fp32: random states, both clamped ends and the lowered index of the last trajectory."""
    from ref64_wells import grid_control
    pb = psp.DoubleWell_OU(d=d, T=N * dt, alpha=0.7, kappa=1.5, device="cpu")
    pb.gamma = torch.linspace(0.5, 1.5, d - 1).reshape(d - 1, 1)
    pb.gamma[-1] = pb.gamma[0]                     # two coordinates share one constant table
    pb.compute_reference_solution_x_1(nx=300)
    K = 29
    ref = pc.ul2_reference(pb, N, dt, 32, K, 0)
    assert ref["kind"] == nat.UL2_GRID and ref["row"].tolist() == list(range(N)) and ref["nrows"] == N
    assert ref["tables"].shape[0] == 1 + (d - 2 if d > 2 else d - 1) and ref["group"][0] == 0
    assert torch.all(ref["group"][d:] == 0)
    gen = torch.Generator().manual_seed(3)
    X = 1.5 * torch.randn(K, d, generator=gen)
    X[0, 0], X[1, 0], X[2, 0], X[-1, 0] = -7.0, 7.0, 2.5 - 2 * pb.dx, 0.3
    for n in range(N):
        want = torch.tensor(np.asarray(pb.u_true(X, n * dt))).t().float()
        got = grid_control(ref, X, n).float()
        assert torch.equal(got[:, :d], want), n
