"""plan_native.decide() without a device: the recorded table of tests/test_gpu_hjb_plan_table.py, and the rules the table cannot hold.

decide() is host arithmetic and size queries; the library plans for 256 CUs when no device is visible, so with `cus` set to the
count the table was recorded on it must answer every row of tests/golden/hjb_plan_decisions.json (all but `graph_wanted`, which
the plan forms from the solver's present use_graph on every iteration -- its size rule, launch_bound, is tested directly below).
"""
import pytest
import torch

from hjb_plan_cases import CASES, NARROW, _case, build_solver, observe, outcome
from test_gpu_hjb_plan_table import SWITCHES, load_table
from util_cases import psp

pn, nat, pc = psp.plan_native, psp.native, psp.plan_common
CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def decide(case, cus, K_local=None, world=1, query_rc=nat.query_rc):
    """(decision, solver) of a case on `world` ranks, this rank holding K_local (default: all K) trajectories."""
    s = build_solver(case, CPU)
    spec = s.problem.native_spec()
    cfg = nat.HjbConfig()
    pc.fill_hjb_base(cfg, s, spec, s.noise, s.K if K_local is None else K_local, 0)
    return pn.decide(s, spec, cfg, s.K if K_local is None else K_local, world, cus, None, query_rc), s


def row(dec):
    """The fields of hjb_plan_cases.observe that a decision carries."""
    return dict(state_basis=dec.state_basis, state_basis_reason=dec.state_basis_reason, matrix_mode=dec.matrix_mode,
                range_guard=dec.range_guard, regen_xi=dec.regen_xi, family=dec.family, d_pad=dec.d_pad, H_pad=dec.H_pad,
                store_path=dec.store_path, sigma_kind=dec.sigma_kind, mlp_dtype=dec.mlp_dtype, n_chunks=dec.n_chunks,
                chunk_mode=dec.chunk_mode, chunk_K=dec.chunk_K, ul2=dec.ul2_mode, path_bytes=int(dec.sizes.path_bytes),
                fwd_partial_bytes=int(dec.sizes.fwd_partial_bytes), grad_partial_bytes=int(dec.sizes.grad_partial_bytes))


# ---- the table --------------------------------------------------------------------------------------------------------------
def test_decide_answers_the_recorded_table():
    gold = load_table()
    planned = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    if gold["cus"] != planned:
        pytest.skip("the table was recorded on %d CUs; the library's size queries plan for %d here" % (gold["cus"], planned))
    wrong = []
    for case in CASES:
        got = outcome(lambda: row(decide(case, gold["cus"])[0]))
        want = {k: v for k, v in gold["rows"][case["name"]].items() if k != "graph_wanted"}
        if got != want:
            wrong.append((case["name"], {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}))
    assert not wrong, "%d of %d rows differ (row, {field: (decide, recorded)}): %r" % (len(wrong), len(CASES), wrong[:5])


# ---- the two-tiles-per-CU rule ------------------------------------------------------------------------------------------------
def test_launch_bound_is_two_tiles_per_cu():
    assert pn.launch_bound(8192, 256) and not pn.launch_bound(8208, 256)
    assert pn.launch_bound(8177, 256) and pn.launch_bound(1, 256)            # (a ragged last tile counts as one)
    assert pn.launch_bound(32, 1) and not pn.launch_bound(33, 1)
    assert not pn.launch_bound(16, None)                                     # no device: no size rule


def test_state_basis_follows_the_even_share_and_the_rest_follows_k_local():
    """Two ranks.  The basis is chosen from K / world, so that every rank of a job picks the same one; the matrix mode and
    store_path 4 belong to this rank's own launches and read K_local."""
    dec, _ = decide(_case("share above, rank below", *NARROW, 16400), 256, K_local=8192, world=2)     # share 8200: 513 tiles
    assert (dec.state_basis, dec.matrix_mode, dec.store_path, dec.regen_xi) == ("sigma", "fp32", 1, False)
    dec, _ = decide(_case("share below, rank above", *NARROW, 16384), 256, K_local=8208, world=2)     # share 8192: 512 tiles
    assert dec.state_basis == "x" and dec.state_basis_reason.startswith("launch-bound size")
    assert (dec.matrix_mode, dec.store_path, dec.regen_xi) == ("f16x3", 4, True)
    dec, _ = decide(_case("one rank", *NARROW, 16384), 256)                                             # the same K on one rank
    assert (dec.state_basis, dec.matrix_mode, dec.store_path) == ("sigma", "f16x3", 4)


# ---- no device --------------------------------------------------------------------------------------------------------------
HOST_NAMES = ("d100 K8208", "d100 K8208 f16x3", "d12 K8208", "d200 K16384 u_L2 x-independent", "lqgc d12 K8208 u_L2 linear",
              "dwell d6 K1040 u_L2 grid", "d100 K2064 fp32 two chunks", "d100 K16384 budget 32 MiB",
              "d100 K8208 attached two chunks", "d100 K8208 variance")
HOST_CASES = [dict(c, noise="reference") for c in CASES if c["name"] in HOST_NAMES]      # (the stand-in kernels have no Philox)


@pytest.mark.parametrize("case", HOST_CASES, ids=[c["name"] for c in HOST_CASES])
def test_without_a_device_no_size_rule_applies_and_the_plan_agrees(case, monkeypatch):
    """cus = None: the plan a machine without a GPU builds (as tests/test_plan_gloo_product.py does, on stand-in kernels)."""
    monkeypatch.setattr(pn, "native_eligibility", lambda solver: None)       # (the real check refuses a CPU device)
    dec, s = decide(case, None)
    plan = pn.HjbNativePlan(s, noise=s.noise)
    assert plan.cus is None and not plan._graph_wanted()
    seen = observe(plan)
    assert {k: v for k, v in seen.items() if k != "graph_wanted"} == row(dec)
    assert dec.matrix_mode == ("fp32" if case["solver"].get("mlp_dtype", "auto") == "auto" else case["solver"]["mlp_dtype"])
    assert not dec.regen_xi and dec.store_path in (1, 2, 3) and not dec.state_basis_reason.startswith("launch-bound")
    assert plan.path.numel() * 4 == dec.alloc_sizes.path_bytes and plan.cfg.d == dec.d_pad and plan.cfg.H == dec.H_pad


# ---- queries the library refuses ----------------------------------------------------------------------------------------------
def refusing(pred):
    """nat.query_rc, except that a config `pred` holds for is refused; .asked collects every config queried."""
    def query_rc(cfg):
        query_rc.asked.append(nat.HjbConfig.from_buffer_copy(cfg))
        return (1, nat.HjbSizes(), "refused by the test") if pred(cfg) else nat.query_rc(cfg)
    query_rc.asked = []
    return query_rc


BIG = _case("d100 K8208", *NARROW, 8208)


def test_a_refused_split_product_query_falls_back_to_fp32():
    stub = refusing(lambda c: c.mlp_dtype == nat.MLP_F16X3)
    dec, _ = decide(BIG, 256, query_rc=stub)
    ref, _ = decide(_case("fp32", *NARROW, 8208, mlp_dtype="fp32"), 256)
    assert any(c.mlp_dtype == nat.MLP_F16X3 for c in stub.asked)
    assert (dec.matrix_mode, dec.mlp_dtype, dec.range_guard) == ("fp32", nat.MLP_FP32, False)
    assert row(dec) == row(ref)                                              # store_path 4 and the sizes of the fp32 plan


def test_a_refused_guarded_query_leaves_the_split_products_unguarded():
    stub = refusing(lambda c: bool(c.range_flag))
    dec, _ = decide(BIG, 256, query_rc=stub)
    ref, _ = decide(_case("unguarded", *NARROW, 8208, range_guard=False), 256)
    assert sum(bool(c.range_flag) for c in stub.asked) == 1                  # asked once; every later query is unguarded again
    assert (dec.matrix_mode, dec.range_guard) == ("f16x3", False) and row(dec) == row(ref)


def test_a_refused_store_path_4_keeps_the_noise_in_the_store():
    stub = refusing(lambda c: c.store_path == 4)
    dec, _ = decide(BIG, 256, query_rc=stub)
    ref, _ = decide(_case("store", *NARROW, 8208, path_noise="store"), 256)
    assert any(c.store_path == 4 for c in stub.asked)
    assert (dec.store_path, dec.regen_xi) == (1, False) and row(dec) == row(ref)


def test_sigma_basis_on_the_wide_family_chooses_the_instance_again_in_the_x_basis():
    """state_basis='sigma' on a configuration whose narrow instances the library refuses: the wide family has no one-product forward,
    so the plan goes back to the x basis and chooses its instance again with the problem's own sigma kind."""
    stub = refusing(lambda c: c.d <= pn.STATE_BASIS_MAX_D)
    dec, s = decide(_case("sigma, narrow refused", *NARROW, 8192, state_basis="sigma"), 256, query_rc=stub)
    assert (dec.state_basis, dec.state_basis_reason) == ("x", "the configuration runs on the wide kernel family")
    assert (dec.family, dec.d_pad, dec.H_pad, dec.sigma_kind) == (2, 128, 64, nat.SIGMA_DENSE)
    first_wide = [c for c in stub.asked if c.d == 128][:2]
    assert [c.sigma_kind for c in first_wide] == [nat.SIGMA_IDENTITY, nat.SIGMA_DENSE]
    ref, _ = decide(_case("x, narrow refused", *NARROW, 8192, state_basis="x"), 256, query_rc=refusing(lambda c: c.d <= 112))
    assert row(dec)["path_bytes"] == row(ref)["path_bytes"] and dec.matrix_mode == ref.matrix_mode == "f16x3"
