"""Randomised differential test of the run-time-shaped value-net kernels (csrc/genl_kernels.h, plan_general_deep.py) against
the CPU oracle, under every execution geometry a draw admits.

Each draw is one GeneralSolver / EllipticSolver case with a value net the templated gen_* kernels do not take: one to four
hidden layers of widths in {1 .. 128}, relu^2 / tanh^2 / tanh in the dense-concat layout or DenseNet_tanh's nn.Linear layout,
input widths 1 .. 112 across the 16-column block edges, ragged batches, horizons past which tiles leave the time loop at
different steps, unbounded / sphere (Dirichlet, Neumann) / box / corner / ball / annulus domains, diffusion and BSDE losses.
make_genl_plan (csrc/api_genl.hip) picks the waves per tile of the forward (1, 4 or 8) and the backward instance
(genl_bwd_kernel<1>, <8, 3> for at most 24 hidden blocks, <8, 4> above); PSP_GENL_NW forces the choice, and every run asserts
the geometry it asked for, so a later change of the heuristic cannot drop coverage silently.  Every run is compared with the
oracle: loss <= 5e-5 relative on the first iteration and <= 1e-4 after, the first iteration's gradient <= 5e-4 max|g|, K_log
exact.  The path store is filled with NaN before the first iteration, so that a slot read without having been written fails
here whatever the allocator hands back."""
import math
import random

import pytest
import torch

from test_general_composite_golden import build as build_pkg
from util_cases import general_oracle_run

WIDTHS = [1, 3, 16, 17, 33, 50, 64, 65, 110, 128]
KINDS = ["densenet", "user_tanh2", "densenet_tanh", "densenet_concat_tanh"]
D_PARABOLIC = [1, 2, 15, 16, 17, 47, 63, 100, 111]            # d_in = d + 1: 2 .. 112, on both sides of every block edge
D_ELLIPTIC = [1, 2, 15, 16, 17, 47, 63, 64, 100, 112]
N_DRAWS = 28


def dev():
    return torch.device("cuda:0")


def _blocks(n):
    return (n + 15) // 16


def geometry(d_in, arch):
    """(HBsum, TB, small) as make_genl_plan computes them: hidden blocks, blocks of the concatenation, one-wave capable."""
    hb = sum(_blocks(h) for h in arch)
    tb = _blocks(d_in) + hb
    return hb, tb, hb <= 8 and tb <= 16


def expected_geometry(d_in, arch, K, nw, cus):
    """(forward waves per tile, backward instance) make_genl_plan picks for PSP_GENL_NW = nw (None: unset)."""
    hb, tb, small = geometry(d_in, arch)
    nt = _blocks(K)
    w = 1 if small and (hb <= 5 or nt >= 4 * cus) else 8
    if nw == "1" and small:
        w = 1
    if nw == "8":
        w = 8
    fwd = 4 if (w == 8 and (nt >= 2 * cus or nw == "4")) else w
    if nw == "8":
        fwd = 8
    bwd = "genl_bwd_kernel<1>" if w == 1 else ("genl_bwd_kernel<8, 3>" if hb <= 24 else "genl_bwd_kernel<8, 4>")
    return fwd, bwd


def geometries(d_in, arch):
    """The PSP_GENL_NW settings a net admits: unset; 1 for a small net; 4 and 8 otherwise."""
    return [None] + (["1"] if geometry(d_in, arch)[2] else ["4", "8"])


def _draw_net(rng):
    while True:
        if rng.random() < 0.2:               # wide and deep: more than 24 hidden blocks, the four-slot backward
            arch = [rng.choice([110, 128]) for _ in range(4)]
        else:
            arch = [rng.choice(WIDTHS) for _ in range(rng.randint(1, 4))]
        kind = rng.choice(KINDS)
        if kind == "densenet" and len(arch) == 2 and arch[0] == arch[1] and arch[0] <= 64:
            continue                         # (the templated gen_* kernels' nets)
        return dict(kind=kind, arch=arch, seed=rng.randint(1, 999))


def _draw(i):
    rng = random.Random(7000 + i)
    fam = ["general", "general_bounded", "elliptic"][i % 3]
    pick = i // 3                            # the problem kinds of a family in turn, the rest drawn
    K = rng.choice([1, 5, 16, 17, 33, 150, 257])
    N = rng.choice([1, 2, 7, 25])
    dt = rng.choice([0.01, 0.02])
    loss = rng.choice(["diffusion", "diffusion", "BSDE"])
    solver = dict(seed=42, delta_t=dt, N=N, lr=0.001, L=rng.choice([2, 3]) if rng.random() < 0.2 else 1, K=K,
                  K_boundary=rng.choice([2, 6, 10]), loss_method=loss, adaptive_forward_process=rng.random() < 0.4)
    attrs, numpy_seed = {}, None
    if fam == "general":
        d = rng.choice(D_PARABOLIC)
        kind = ["DoubleWell_multidim_for_general_solver", "AllenCahn", "HeatEquation"][pick % 3]
        T = (rng.choice([0.4, 1.5]) if N >= 7 else 1.5) * N * dt     # 0.4: every trajectory runs out of time before step N
        if kind.startswith("DoubleWell"):
            kwargs = dict(d=d, d_1=d // 2, d_2=d - d // 2, T=T, eta=0.1, kappa=0.5, modus=rng.choice(["HJB", "linear"]))
        else:
            kwargs = dict(d=d, T=T, seed=42) if kind == "HeatEquation" else dict(d=d, T=T, seed=42, modus="pt")
        solver["alpha"] = [1.0, rng.choice([0.5, 1.0]), 1.0]
    elif fam == "general_bounded":
        d = rng.choice(D_PARABOLIC)
        kind = ["ExponentialOnSphereNonlinearParabolic", "ExponentialOnSphereNonlinearParabolic", "QuadraticOnBox"][pick % 3]
        T = (rng.choice([0.4, 1.5]) if N >= 7 else 1.5) * N * dt
        if kind == "QuadraticOnBox":
            kwargs = dict(d=d, T=T, X_l=-1.0, X_r=rng.choice([0.7, 1.0]), one_boundary=rng.random() < 0.4, scale=1.0,
                          quad_h=rng.random() < 0.5)
        else:
            kwargs = dict(d=d, T=T, alpha=0.2)
            if pick % 3 == 1:
                attrs["boundary_type"] = "Neumann"
        solver["alpha"] = [1.0, 1.0, rng.choice([0.5, 2.0])]
        # (loss_with_stopped only where trajectories stop: the reference's mean over an empty selection is NaN)
        solver["loss_with_stopped"] = N >= 7 and rng.random() < 0.3
    else:
        d = rng.choice(D_ELLIPTIC)
        kind = ["ExponentialOnSphere", "ExponentialOnBallNonlinear", "ExponentialOnBallNonlinearSin", "QuadraticOnBox",
                "square-corner", "Committor"][pick % 6]
        if kind in ("QuadraticOnBox", "square-corner"):
            kwargs = dict(d=d, X_l=-1.0, X_r=1.0, one_boundary=kind == "QuadraticOnBox" and rng.random() < 0.4, parabolic=False,
                          quad_h=rng.random() < 0.5)
            if kind == "square-corner":
                kind, attrs = "QuadraticOnBox", dict(boundary="square-corner", X_corner=0.2)
        elif kind == "Committor":
            kwargs = dict(d=d)
            K = max(K, 33)                   # ('two_spheres': the rejection step must leave a batch)
            solver["K"] = K
        else:
            kwargs = dict(d=d, alpha=0.2)
            if kind != "ExponentialOnSphere" and loss == "diffusion" and rng.random() < 0.4:
                kwargs["boundary_type"] = solver["boundary_type"] = "Neumann"
        solver["alpha"] = [1.0, rng.choice([0.5, 1.0])]
        solver["loss_with_stopped"] = N >= 7 and rng.random() < 0.3
    if kind in ("QuadraticOnBox", "Committor") and d == 1:
        d = 2                                # (the reference's box and annulus samplers need d >= 2)
        kwargs["d"] = 2
        if "d_1" in kwargs:
            kwargs["d_1"], kwargs["d_2"] = 1, 1
    if kind == "QuadraticOnBox":
        numpy_seed = 9
        K = solver["K"] = max(K, 2)          # (the reference takes the terminal batch X[:K_boundary] from the K points)
    solver["K_boundary"] = min(solver["K_boundary"], K)
    if kind == "QuadraticOnBox":
        solver["K_boundary"] = max(2, 2 * (solver["K_boundary"] // 2))
    case = dict(name="genlfuzz%d" % i, family=fam, problem=dict(kind=kind, kwargs=kwargs), solver=solver, net=_draw_net(rng))
    if attrs:
        case["problem"]["attrs"] = attrs
    if numpy_seed is not None:
        case["numpy_seed"] = numpy_seed
    return case


def _d_in(case):
    return case["problem"]["kwargs"]["d"] + (0 if case["family"] == "elliptic" else 1)


def _two_spheres(case):
    return case["problem"]["kind"] == "Committor"


def run_native(case, L=None, nw=None, monkeypatch=None):
    """The native run of a case: the plan is built first and its path store filled with NaN; returns (model, plan, per
    iteration [(gradient, tile step counts)])."""
    if monkeypatch is not None:
        if nw is None:
            monkeypatch.delenv("PSP_GENL_NW", raising=False)
        else:
            monkeypatch.setenv("PSP_GENL_NW", nw)
    over = {} if L is None else dict(L=L)
    prob, model = build_pkg(case, device=dev(), backend="native", **over)
    plan = model._choose_plan()
    assert model.plan_name == "native" and type(plan).__name__ == "GeneralDeepPlan", (case, getattr(model, "plan_reason", None))
    plan.path.fill_(float("nan"))
    seen = []
    step = plan.iteration

    def iteration(l):
        out = step(l)
        seen.append((plan.grad.detach().cpu().clone(), plan._tile_steps().cpu().clone()))
        return out
    plan.iteration = iteration
    model.train()
    assert model._gen_plan is plan
    return model, plan, seen


def check_against_oracle(case, model, seen, ref, what=""):
    assert model.K_log == ref["K_log"], (what, case, model.K_log, ref["K_log"])
    for l, (got, want) in enumerate(zip(model.loss_log, ref["loss_log"])):
        assert math.isclose(got, want, rel_tol=5e-5 if l == 0 else 1e-4, abs_tol=1e-7), (what, case, model.loss_log, ref["loss_log"])
    assert len(model.loss_log) == len(ref["loss_log"])
    g_ref = torch.cat([g.reshape(-1) for g in ref["traces"][0]["grads"]])
    g = seen[0][0]
    assert g.shape == g_ref.shape
    err = float((g - g_ref).abs().max())
    assert err <= 5e-4 * float(g_ref.abs().max()) + 1e-10, (what, case, err, float(g_ref.abs().max()))
    if case["family"] == "elliptic" and not _two_spheres(case) and ref.get("V_L2_log") and any(model.V_L2_log):
        for got, want in zip(model.V_L2_log, ref["V_L2_log"]):
            assert math.isclose(got, want, rel_tol=1e-4, abs_tol=1e-9), (what, case, model.V_L2_log, ref["V_L2_log"])
    return err / max(float(g_ref.abs().max()), 1e-30)


def run_all_geometries(case, monkeypatch, want_nw=None):
    """The case under every geometry it admits (or those of want_nw), each against the same oracle run."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ref = general_oracle_run(case, trace=True)[1]
    d_in, arch = _d_in(case), case["net"]["arch"]
    covered = []
    for nw in (want_nw or geometries(d_in, arch)):
        model, plan, seen = run_native(case, nw=nw, monkeypatch=monkeypatch)
        fwd, bwd = expected_geometry(d_in, arch, plan.K_local, nw, cus)
        assert int(plan.sizes.waves_per_tile) == fwd, (case, nw, int(plan.sizes.waves_per_tile), fwd)
        err = check_against_oracle(case, model, seen, ref, what="PSP_GENL_NW=%s" % nw)
        covered.append("fwd<%d> + %s" % (fwd, bwd))
        print("%s NW=%s: %s, gradient rel err %.1e" % (case["name"], nw, covered[-1], err))
    return covered


def test_draws_cover_the_kernel_family():
    """What the draws reach, without a GPU: every activation / layout, every width, the input block edges, every geometry and
    backward instance, long horizons, and never a net the templated kernels take."""
    kinds, widths, d_ins, geo, depths, problems = set(), set(), set(), set(), set(), set()
    for i in range(N_DRAWS):
        case = _draw(i)
        net = case["net"]
        assert not (net["kind"] == "densenet" and len(net["arch"]) == 2 and net["arch"][0] == net["arch"][1] <= 64)
        kinds.add(net["kind"])
        widths.update(net["arch"])
        depths.add(len(net["arch"]))
        d_ins.add(_d_in(case))
        problems.add((case["problem"]["kind"], str(case["problem"].get("attrs")), case["solver"]["loss_method"]))
        for nw in geometries(_d_in(case), net["arch"]):
            geo.add(expected_geometry(_d_in(case), net["arch"], case["solver"]["K"], nw, 256))
    assert kinds == set(KINDS) and depths == {1, 2, 3, 4}
    assert widths >= {1, 16, 17, 33, 64, 65, 128}, widths
    assert {fwd for fwd, _ in geo} == {1, 4, 8}
    assert {bwd for _, bwd in geo} == {"genl_bwd_kernel<1>", "genl_bwd_kernel<8, 3>", "genl_bwd_kernel<8, 4>"}, geo
    assert min(d_ins) == 1 and max(d_ins) == 112 and {16, 17} <= d_ins, d_ins
    assert ("ExponentialOnSphereNonlinearParabolic", str(dict(boundary_type="Neumann")), "BSDE") in problems
    assert {p[0] for p in problems} >= {"DoubleWell_multidim_for_general_solver", "AllenCahn", "HeatEquation", "QuadraticOnBox",
                                        "ExponentialOnSphereNonlinearParabolic", "ExponentialOnSphere", "Committor",
                                        "ExponentialOnBallNonlinear", "ExponentialOnBallNonlinearSin"}
    assert any(p[1] == str(dict(boundary="square-corner", X_corner=0.2)) for p in problems)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(N_DRAWS))
def test_random_deep_configuration_matches_oracle(i, monkeypatch):
    run_all_geometries(_draw(i), monkeypatch)


# ---- fixed shapes the draws may miss ----------------------------------------------------------------------------------

def _dwell(d, arch, K=40, N=3, loss="diffusion", kind="densenet"):
    return dict(name="dwell_d%d_%s" % (d, "x".join(map(str, arch))), family="general",
                problem=dict(kind="DoubleWell_multidim_for_general_solver",
                             kwargs=dict(d=d, d_1=d // 2, d_2=d - d // 2, T=0.5 * N * 0.01, eta=0.1, kappa=0.5, modus="HJB")),
                solver=dict(seed=42, delta_t=0.01, N=N, lr=0.001, L=1, K=K, K_boundary=6, loss_method=loss,
                            alpha=[1.0, 1.0, 1.0]),
                net=dict(kind=kind, arch=arch, seed=42))


@pytest.mark.gpu
def test_widest_input_and_deepest_widest_net(monkeypatch):
    """d_in = 112 (seven input blocks) with 4 x 128 hidden units: TB = 39, HBsum = 32, the largest register arrays and LDS
    images (genl_bwd_lds_bytes = 145 KiB) -- the backward's <8, 4> instance."""
    from path_space_pde_solver_amd import plan_general_deep as pgd
    case = _dwell(111, [128, 128, 128, 128], loss="BSDE")
    assert geometry(112, case["net"]["arch"])[:2] == (32, 39)
    prob, model = build_pkg(case, device=dev(), backend="native")
    assert pgd.deep_eligibility(model) is None
    assert "<8, 4>" in run_all_geometries(case, monkeypatch)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("arch", [[128, 128, 128], [128, 128, 128, 16]])
def test_backward_instance_boundary(arch, monkeypatch):
    """HBsum = 24 runs the three-slot eight-wave backward, HBsum = 25 the four-slot one."""
    case = dict(_dwell(20, arch, K=33, N=7), problem=dict(kind="AllenCahn", kwargs=dict(d=20, T=0.04, seed=42, modus="pt")))
    covered = run_all_geometries(case, monkeypatch, want_nw=[None])
    assert covered == ["fwd<8> + genl_bwd_kernel<8, %d>" % (3 if sum(_blocks(h) for h in arch) <= 24 else 4)]


@pytest.mark.gpu
def test_one_unit_net_on_a_sphere_with_early_exits(monkeypatch):
    case = dict(name="sphere_width1", family="general_bounded",
                problem=dict(kind="ExponentialOnSphereNonlinearParabolic", kwargs=dict(d=5, T=0.3, alpha=0.5)),
                solver=dict(seed=42, delta_t=0.01, N=25, lr=0.001, L=2, K=150, K_boundary=10, loss_method="diffusion",
                            alpha=[1.0, 1.0, 1.0]),
                net=dict(kind="densenet", arch=[1], seed=42))
    model, plan, seen = run_native(case)
    steps = seen[0][1]
    assert int(steps.min()) < int(steps.max())             # tiles left the loop at different steps
    assert run_all_geometries(case, monkeypatch) == ["fwd<1> + genl_bwd_kernel<1>"] * 2


@pytest.mark.gpu
def test_four_wave_forward_at_a_batch_that_fills_the_chip():
    """No override: at ceil(K / 16) >= 2 CUs the plan runs the four-wave forward with the eight-wave backward."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    K = 32 * cus + 8                                        # ragged: the last tile holds 8 trajectories
    case = dict(name="allencahn_fill", family="general",
                problem=dict(kind="AllenCahn", kwargs=dict(d=10, T=0.015, seed=42, modus="pt")),
                solver=dict(seed=42, delta_t=0.01, N=3, lr=0.001, L=1, K=K, K_boundary=10, loss_method="BSDE",
                            adaptive_forward_process=True, alpha=[1.0, 1.0, 1.0]),
                net=dict(kind="densenet", arch=[64, 64, 64], seed=42))
    # (BSDE: Y starts at the forward's V(X_0) and the control is its grad_x V, so an error of the four-wave forward reaches the
    #  loss directly; the diffusion loss would see it only through V(X_N) - V(X_0) over three short steps)
    model, plan, seen = run_native(case)
    assert int(plan.sizes.waves_per_tile) == 4
    assert expected_geometry(11, [64, 64, 64], K, None, cus) == (4, "genl_bwd_kernel<8, 3>")
    assert int(seen[0][1].min()) < int(seen[0][1].max())
    check_against_oracle(case, model, seen, general_oracle_run(case, trace=True)[1])


# ---- the BSDE loss with a Neumann boundary on the deep plan ----------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["densenet", "densenet_tanh"])
def test_bsde_neumann_takes_frozen_points_of_tiles_that_left_early(kind):
    """The Neumann residual takes grad_x V at the state of the LAST executed loop step (solver.py:1182-1183): for a tile whose
    trajectories all stopped before it, their frozen (X_N, t_N) -- the genl forward never writes those slots."""
    from conftest import load_golden
    case = dict(load_golden("expsphere_d3_bsde_neumann")["case"], net=dict(kind=kind, arch=[20, 20, 20], seed=42))
    assert case["solver"]["K"] >= 64 and case["solver"]["L"] == 3
    model, plan, seen = run_native(case)
    steps = seen[0][1]
    assert int(steps.min()) < int(steps.max())             # some tiles left before the last loop step: the case bites
    check_against_oracle(case, model, seen, general_oracle_run(case, trace=True)[1])
