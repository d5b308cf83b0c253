"""The configurations behind tests/golden/hjb_plan_decisions.json: what HjbNativePlan (plan_native.py) decides for each.

`CASES` are small Solver configurations (N = 5 everywhere: the decisions read K, d, H and the switches, never the step count)
with K on both sides of every size rule at 256 CUs -- 1024 / 1040 (quad forward), 8192 / 8208 (two 16-trajectory tiles per CU: state
basis, matrix mode, store_path 4, hipGraph replay), 16384 --, both kernel families, every mlp_dtype, the switches of the plan and
the chunked path store.  `observe(plan)` is the row of a built plan; `outcome(fn)` is that row or, where the constructor refuses,
the exception.  tests/test_gpu_hjb_plan_table.py builds the plans on the device, tests/test_hjb_plan_decisions_host.py asks
plan_native.decide() for the same rows without one.
"""
from util_cases import make_pkg_problem, psp

T, DT = 0.05, 0.01                      # N = 5


def _llgc(d, off=0.01):
    return dict(kind="LLGC", kwargs=dict(d=d, off_diag=off, T=T, seed=42))


def _lqgc(d, off=0.1):
    return dict(kind="LQGC", kwargs=dict(d=d, off_diag=off, T=T, seed=42, delta_t=DT))


def _dwell(d):
    grid = dict(delta_t=DT, xb=2.5, nx=100)
    return dict(kind="DoubleWell_multidim", kwargs=dict(d=d, d_1=d // 2, d_2=d - d // 2, T=T, eta=0.05, kappa=1.0),
                calls=[("compute_reference_solution", grid), ("compute_reference_solution_2", grid)])


BASE = dict(lr=1e-3, L=1, delta_t=DT, loss_method="log-variance", time_approx="inner", adaptive_forward_process=True,
            detach_forward=True, u_l2_error_flag=False, seed=42)


def _case(name, problem, widths, K, noise="philox", **solver):
    return dict(name=name, problem=problem, widths=widths, noise=noise, solver=dict(BASE, K=K, **solver))


NARROW, PADDED, ILL = (_llgc(100), (64, 64)), (_llgc(12, 0.1), (30, 30)), (_llgc(20, 0.3), (30, 30))
WIDE128, WIDE200 = (_llgc(128), (64, 64)), (_llgc(200), (64, 64))

CASES = [
    # ---- narrow family, d = 100, H = 64: K across every size rule
    _case("d100 K1024", *NARROW, 1024), _case("d100 K1040", *NARROW, 1040), _case("d100 K8192", *NARROW, 8192),
    _case("d100 K8208", *NARROW, 8208), _case("d100 K16384", *NARROW, 16384),
    # ---- every mlp_dtype, on both sides of the two-tiles-per-CU rule
    _case("d100 K8208 fp32", *NARROW, 8208, mlp_dtype="fp32"), _case("d100 K8208 f16x3", *NARROW, 8208, mlp_dtype="f16x3"),
    _case("d100 K8208 bf16", *NARROW, 8208, mlp_dtype="bf16"), _case("d100 K8192 f16x3", *NARROW, 8192, mlp_dtype="f16x3"),
    # ---- range guard, path noise, hipGraph replay, supplied noise
    _case("d100 K8208 unguarded", *NARROW, 8208, range_guard=False),
    _case("d100 K8208 path_noise store", *NARROW, 8208, path_noise="store"),
    _case("d100 K8208 graph True", *NARROW, 8208, use_graph=True), _case("d100 K8208 graph False", *NARROW, 8208, use_graph=False),
    _case("d100 K8192 graph True", *NARROW, 8192, use_graph=True), _case("d100 K8192 graph False", *NARROW, 8192, use_graph=False),
    _case("d100 K8208 reference noise", *NARROW, 8208, noise="reference"),
    # ---- state basis
    _case("d100 K8192 basis sigma", *NARROW, 8192, state_basis="sigma"), _case("d100 K8208 basis x", *NARROW, 8208, state_basis="x"),
    _case("d20 ill-conditioned K8208", *ILL, 8208),
    _case("d128 basis sigma", *WIDE128, 8208, state_basis="sigma"),                    # (raises ValueError)
    # ---- a padded instance (d = 12, H = 30)
    _case("d12 K1024", *PADDED, 1024), _case("d12 K8208", *PADDED, 8208),
    # ---- wide family
    _case("d128 K1024", *WIDE128, 1024), _case("d128 K8208", *WIDE128, 8208),
    _case("d200 K8192", *WIDE200, 8192), _case("d200 K8208", *WIDE200, 8208), _case("d200 K16384", *WIDE200, 16384),
    _case("d200 K8208 fp32", *WIDE200, 8208, mlp_dtype="fp32"), _case("d200 K8208 bf16", *WIDE200, 8208, mlp_dtype="bf16"),
    # ---- forward process and losses
    _case("d100 K8208 attached", *NARROW, 8208, detach_forward=False), _case("d100 K1024 attached", *NARROW, 1024, detach_forward=False),
    _case("d100 K8208 relative entropy", *NARROW, 8208, loss_method="relative_entropy"),
    _case("d100 K8208 relative entropy attached", *NARROW, 8208, loss_method="relative_entropy", detach_forward=False),
    _case("d100 K8208 variance", *NARROW, 8208, loss_method="variance"),
    _case("d100 K1024 cross entropy", *NARROW, 1024, loss_method="cross_entropy"),
    _case("d100 K8208 non-adaptive", *NARROW, 8208, adaptive_forward_process=False),
    _case("d100 K8208 random X_0", *NARROW, 8208, random_X_0=True),
    _case("d100 K1024 moment learn Y_0", *NARROW, 1024, loss_method="moment", learn_Y_0=True),
    # ---- the three u_L2 kinds
    _case("d100 K8208 u_L2 x-independent", *NARROW, 8208, u_l2_error_flag=True),
    _case("d200 K16384 u_L2 x-independent", *WIDE200, 16384, u_l2_error_flag=True),
    _case("lqgc d12 K8208 u_L2 linear", _lqgc(12), (30, 30), 8208, u_l2_error_flag=True),
    _case("dwell d6 K1040 u_L2 grid", _dwell(6), (30, 30), 1040, u_l2_error_flag=True),
    # ---- K-chunking: forced, from a budget (ragged and in whole launch waves), both modes
    _case("d100 K2064 fp32 two chunks", *NARROW, 2064, mlp_dtype="fp32", path_chunks=2),
    _case("d100 K2064 fp32 two chunks recompute", *NARROW, 2064, mlp_dtype="fp32", path_chunks=2, chunk_mode="recompute"),
    _case("d100 K16384 budget 32 MiB", *NARROW, 16384, path_budget_bytes=32 << 20),
    _case("d100 K65536 budget 128 MiB", *NARROW, 65536, path_budget_bytes=128 << 20),
    _case("d100 K8208 attached two chunks", *NARROW, 8208, detach_forward=False, path_chunks=2),
    _case("d100 K8208 u_L2 two chunks", *NARROW, 8208, u_l2_error_flag=True, path_chunks=2),
    _case("lqgc d12 K8208 u_L2 two chunks", _lqgc(12), (30, 30), 8208, u_l2_error_flag=True, path_chunks=2),   # (raises PlanUnsupported)
    _case("d100 K8208 variance two_gradient", *NARROW, 8208, loss_method="variance", path_chunks=2,
          chunk_mode="two_gradient"),                                                                           # (raises PlanUnsupported)
]
NAMES = [c["name"] for c in CASES]
assert len(set(NAMES)) == len(NAMES)


def build_solver(case, device):
    prob = make_pkg_problem(case["problem"], device)
    return psp.Solver(case["name"], prob, verbose=False, device=device, backend="native", noise=case["noise"],
                      widths=tuple(case["widths"]), **case["solver"])


def observe(plan):
    """What the plan decided, from the attributes bench.py, solver.py and the tests read."""
    ul2 = [n for n in ("ul2", "ul2_gain", "ul2_tab") if getattr(plan, n) is not None]
    assert len(ul2) <= 1
    return dict(state_basis=plan.state_basis, state_basis_reason=plan.state_basis_reason, matrix_mode=plan.matrix_mode,
                range_guard=plan.range_flag is not None, regen_xi=bool(plan.regen_xi), family=int(plan.family),
                d_pad=int(plan.d_pad), H_pad=int(plan.H_pad), store_path=int(plan.cfg.store_path),
                sigma_kind=int(plan.cfg.sigma_kind), mlp_dtype=int(plan.cfg.mlp_dtype), n_chunks=int(plan.n_chunks),
                chunk_mode=plan.chunk_mode, chunk_K=int(plan.chunk_K), graph_wanted=bool(plan._graph_wanted()),
                ul2=ul2[0] if ul2 else None, path_bytes=int(plan.sizes.path_bytes),
                fwd_partial_bytes=int(plan.sizes.fwd_partial_bytes), grad_partial_bytes=int(plan.sizes.grad_partial_bytes))


def outcome(fn):
    """fn() -- a row -- or the refusal: the configurations a constructor turns down stay in the table with their message."""
    try:
        return fn()
    except (psp.plan_native.PlanUnsupported, ValueError) as e:
        return dict(raises=type(e).__name__, message=str(e))
