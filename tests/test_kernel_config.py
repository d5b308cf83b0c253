"""kernel_config.py: a catalogue problem and its value net become kernel config fields in one place.  Expected values are written
out from include/psp.h (the enums' numbers) and problems.py (the problems' attributes), not taken from the fillers; nothing here
needs a GPU or the built library (the eligibility tests hand the plans a recording stand-in for it)."""
import ctypes as C
import math

import pytest
import torch

from util_cases import psp
from path_space_pde_solver_amd import kernel_config as kc
from path_space_pde_solver_amd import plan_general_deep as pgd
from path_space_pde_solver_amd import plan_eigen_native as pen
from path_space_pde_solver_amd import plan_pinn_native as ppn
from path_space_pde_solver_amd import plan_value_native as pvn
from path_space_pde_solver_amd import device_test_log as dtl

nat = psp.native
F32 = lambda v: torch.tensor(v, dtype=torch.float32).item()      # noqa: E731


class _Solver:
    """The attributes the fillers read."""

    def __init__(self, problem, N=7, delta_t=0.02, adaptive=False):
        self.problem, self.d, self.N = problem, problem.d, N
        self.delta_t, self.sq_delta_t = torch.tensor(delta_t), torch.sqrt(torch.tensor(delta_t))
        self.adaptive_forward_process = adaptive


def _filled(problem, elliptic, **kw):
    base = nat.GenConfig()
    kc.fill_problem(base, _Solver(problem, **kw), problem.general_native_spec(), elliptic, 48, 16, 'reference')
    # the part every problem shares: the batch, the step, the switches
    assert (base.K_local, base.N, base.k_offset, base.d_real, base.store_path) == (48, kw.get('N', 7), 16, problem.d, 1)
    assert base.dt == F32(kw.get('delta_t', 0.02)) and base.sqrt_dt == F32(math.sqrt(F32(kw.get('delta_t', 0.02))))
    assert base.noise_mode == 0 and base.adaptive == (1 if kw.get('adaptive') else 0)       # PSP_NOISE_SUPPLIED
    assert base.d == 0 and not base.drift and not base.range_flag and base.mlp_dtype == 0   # the callers' business
    return base


def test_fill_problem_quadratic_on_box():
    pb = psp.QuadraticOnBox(d=3, T=0.5, X_l=-1.0, X_r=1.5, scale=1.25, device='cpu')
    base = _filled(pb, False, adaptive=True)
    assert (base.domain_kind, base.dom_a, base.dom_b) == (2, -1.0, 1.5)                     # PSP_DOM_BOX
    assert (base.h_kind, base.drift_kind, base.dwell_form) == (1, 0, 0)                     # PSP_GH_QUAD, PSP_DRIFT_ZERO
    assert base.sigma_scale == 1.25 and base.T == 0.5 and list(base.h_par) == [0.0] * 4
    base = nat.GenConfig()
    kc.fill_problem(base, _Solver(pb), pb.general_native_spec(), False, 8, 0, 'philox')
    assert base.noise_mode == 1                                                             # PSP_NOISE_PHILOX
    one = psp.QuadraticOnBox(d=2, one_boundary=True, parabolic=False, device='cpu')
    assert _filled(one, True).domain_kind == 3 and _filled(one, False).domain_kind == 4     # PSP_DOM_BOX_UPPER_ALL / _ANY


def test_fill_problem_double_well_stopping():
    pb = psp.DoubleWell_stopping(d=1, device='cpu')
    base = _filled(pb, True)
    assert (base.h_kind, base.drift_kind, base.dwell_form) == (7, 3, 1)                     # PSP_GH_AFFINE_EXP, PSP_DRIFT_DOUBLE_WELL
    assert list(base.h_par) == [1.0, 0.0, -0.5, 0.0]                                        # h = 1 - |z|^2 / 2 (problems.py)
    assert base.sigma_scale == 1.0 and base.T == float('inf')
    # the exit problem's domain (problems.py: 'square' with one boundary, [-2, 1]); the elliptic solvers stop at the upper face
    assert (base.domain_kind, base.dom_a, base.dom_b) == (3, -2.0, 1.0)                     # PSP_DOM_BOX_UPPER_ALL


def test_fill_problem_on_the_ball():
    pb = psp.ExponentialOnBallNonlinearSin(d=4, device='cpu')
    base = _filled(pb, True)
    assert (base.domain_kind, base.dom_a) == (1, F32(pb.boundary_distance))                 # PSP_DOM_SPHERE
    assert base.h_kind == 5 and list(base.h_par) == [F32(pb.alpha), 4.0, 0.0, 0.0]          # PSP_GH_EXPBALL_SIN
    assert base.sigma_scale == F32(math.sqrt(2.0))


def test_fill_problem_helmholtz():
    pb = psp.Helmholtz(d=2, device='cpu')
    base = _filled(pb, True)
    assert base.h_kind == 8 and base.drift_kind == 0                                        # PSP_GH_SINE_SOURCE
    assert list(base.h_par) == [0.0, F32(math.pi), F32(4.0 * math.pi), 1.0]                 # (0, a_1 pi, a_2 pi, k^2)
    assert (base.domain_kind, base.dom_a, base.dom_b) == (2, -1.0, 1.0) and base.sigma_scale == F32(math.sqrt(2.0))


def test_fill_problem_committor():
    pb = psp.Committor(d=3, device='cpu')
    base = _filled(pb, True)
    assert base.domain_kind == 5 and (base.dom_a, base.dom_b) == (1.0, 2.0) and base.dom_a < base.dom_b     # PSP_DOM_ANNULUS
    assert (base.h_kind, base.drift_kind, base.sigma_scale) == (0, 0, 1.0)


@pytest.mark.parametrize("make", [nat.GenlConfig, nat.PinnConfig, nat.GenlEvalConfig])
def test_fill_value_net(make):
    relu2 = pgd.value_net_spec(psp.DenseNet(d_in=4, d_out=1, lr=1e-3, arch=[5, 3], seed=1), 4)
    cfg = make()
    kc.fill_value_net(cfg, relu2, True)
    assert (cfg.has_time, cfg.n_hidden, list(cfg.widths)) == (1, 2, [5, 3, 0, 0])
    assert (cfg.activation, cfg.linear_layout) == (0, 0)                                    # PSP_ACT_RELU2, (in, out) weights
    tanh = pgd.value_net_spec(psp.DenseNet_tanh(d_in=3, d_out=1, lr=1e-3, arch=[6, 5, 4, 7], seed=1), 3)
    cfg = make()
    kc.fill_value_net(cfg, tanh, False)
    assert (cfg.has_time, cfg.n_hidden, list(cfg.widths)) == (0, 4, [6, 5, 4, 7])
    assert (cfg.activation, cfg.linear_layout) == (2, 1)                                    # PSP_ACT_TANH, nn.Linear weights
    if hasattr(cfg, 'time_first'):
        assert (cfg.time_first, cfg.time_scale) == (0, 0.0)                                 # the value-function ansatz's alone


def test_activation_table_is_one_object():
    assert kc.ACT == {'relu2': 0, 'tanh2': 1, 'tanh': 2}                                    # PSP_ACT_*
    assert pgd._ACT is kc.ACT and dtl._ACT is kc.ACT


def test_upload():
    g = torch.Generator().manual_seed(5)
    M = torch.randn(3, 4, generator=g, dtype=torch.float64)
    keep = []
    t = kc.upload(M.t(), (4, 3), torch.device('cpu'), keep, 'the matrix must be (4, 3)')
    assert keep == [t] and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() != M.data_ptr()
    back = list((C.c_float * 12).from_address(t.data_ptr()))
    assert back == [F32(M[j, i].item()) for i in range(4) for j in range(3)]                # row-major by value
    kc.upload([1.0, 2.0], None, torch.device('cpu'), keep, 'x')
    assert len(keep) == 2 and keep[1].tolist() == [1.0, 2.0]
    # the messages of the two callers that check a shape
    with pytest.raises(ValueError) as e:
        pvn._upload(torch.zeros(2, 3), (2, 2), torch.device('cpu'), keep, 'sigma')
    assert str(e.value) == 'native_spec(): sigma must have shape (2, 2), got (2, 3)' and len(keep) == 2
    gcfg = nat.GenlConfig()
    gcfg.base.d = 2
    with pytest.raises(ValueError) as e:
        psp.plan_general_native.set_sigma(gcfg, {'sigma': torch.zeros(2, 3)}, torch.device('cpu'), keep)
    assert str(e.value) == 'general_native_spec(): sigma must be a (2, 2) matrix, got (2, 3)' and len(keep) == 2


def test_value_net_limits_reason():
    assert (nat.GENL_MAX_HIDDEN_LAYERS, nat.GENL_MAX_WIDTH, nat.GENL_MAX_INPUT) == (4, 128, 112)
    wide = 'V is wider than the native value-net kernels take (hidden <= 128, input <= 112)'
    short = 'outside 1-4 hidden layers of <= 128 units, input <= 112'
    assert kc.value_net_limits_reason([3, 8, 8, 8, 8, 1]) == (None, None, None)
    assert kc.value_net_limits_reason([3, 8, 8, 8, 8, 8, 1]) == \
        ('V has 5 hidden layers (the native value-net kernels take 1 to 4)', None, short)
    assert kc.value_net_limits_reason([3, 128, 1]) == (None, None, None)
    assert kc.value_net_limits_reason([3, 129, 1]) == (None, wide, short)
    assert kc.value_net_limits_reason([112, 8, 1]) == (None, None, None)
    assert kc.value_net_limits_reason([113, 8, 1]) == (None, wide, short)


# ---- the probe an eligibility function sends to the library is the configuration its plan builds ------------------------------

def _snapshot(s):
    """Every field of a ctypes struct that is no pointer, nested structs flattened."""
    out = {}
    for name, typ in s._fields_:
        v = getattr(s, name)
        if typ is C.c_void_p:
            out[name + ' is set'] = bool(v)
        elif isinstance(v, C.Structure):
            out.update(_snapshot(v))
        else:
            out[name] = list(v) if isinstance(v, C.Array) else v
    return out


def _n_params(cfg):
    d_in = getattr(cfg, 'base', cfg).d + cfg.has_time
    dims, fan, n = [d_in] + list(cfg.widths)[:cfg.n_hidden] + [1], 0, 0
    for i in range(len(dims) - 1):
        fan += dims[i]
        n += (fan + 1) * dims[i + 1]
    return n


class _RecordingLibrary:
    """Stands in for libpsp_hip.so: every call succeeds, a size query reports the parameter count (and room for the small
    batches of these tests) and is recorded."""

    def __init__(self):
        self.queries = []

    def psp_last_error(self):
        return b''

    def __getattr__(self, name):
        def call(*args):
            structs = [a._obj for a in args if hasattr(a, '_obj')]
            cfg = next((o for o in structs if isinstance(o, (nat.GenlConfig, nat.PinnConfig))), None)
            for o in structs:
                if isinstance(o, (nat.GenlSizes, nat.PinnSizes)):
                    o.n_params = _n_params(cfg)
                    if isinstance(o, nat.GenlSizes):
                        o.table_bytes = o.path_bytes = o.ahat_bytes = o.grad_partial_bytes = 1 << 16
                    self.queries.append((name, _snapshot(cfg)))
            return 0
        return call


@pytest.fixture
def lib(monkeypatch):
    fake = _RecordingLibrary()
    monkeypatch.setattr(nat, 'load', lambda: fake)
    monkeypatch.setattr(nat, 'is_built', lambda: True)
    return fake


class _OnGpu:
    """A solver as an eligibility check sees it on a GPU machine (nothing is run there)."""
    device = torch.device('cuda')

    def __init__(self, s):
        self._s = s

    def __getattr__(self, name):
        return getattr(self._s, name)


BATCH = ('K_local', 'N', 'k_offset')


def _agree(probe, plan, but=BATCH):
    assert probe.keys() == plan.keys()
    assert {k: v for k, v in probe.items() if k not in but} == {k: v for k, v in plan.items() if k not in but}
    assert (probe['K_local'], probe['N']) == (16, 1)


def _tanh_net(d_in, arch):
    return psp.DenseNet_tanh(d_in=d_in, d_out=1, lr=1e-3, arch=arch, seed=1)


def test_deep_eligibility_probes_the_plans_config(lib):
    pb = psp.DoubleWell_stopping(d=1, device='cpu')                                         # (a drift vector: a pointer)
    model = psp.EllipticSolver(problem=pb, name='t', verbose=False, device='cpu', K=40, N=9, adaptive_forward_process=True)
    model.V = _tanh_net(1, [8, 6, 8])
    assert pgd.deep_eligibility(model) is None
    plan = pgd.GeneralDeepPlan(model)
    (q1, probe), (q2, built) = lib.queries
    assert q1 == q2 == 'psp_genl_query' and built == _snapshot(plan.gcfg)
    _agree(probe, built)
    assert (built['K_local'], built['N'], built['h_kind'], built['drift is set'], built['activation']) == (40, 9, 7, True, 2)


def test_deep_eligibility_probes_a_dense_sigma(lib):
    pb = psp.ExponentialOnBallNonlinearSinHessian(d=3, device='cpu')
    model = psp.EllipticSolver(problem=pb, name='t', verbose=False, device='cpu', K=32, N=4)
    model.V = _tanh_net(3, [8, 8])
    assert pgd.deep_eligibility(model) is None
    plan = pgd.GeneralDeepPlan(model)
    _agree(lib.queries[0][1], lib.queries[1][1])
    assert lib.queries[0][1]['sigma_kind'] == 1 and lib.queries[0][1]['sigma is set'] and plan.gcfg.base.h_kind == 6


def test_eigen_eligibility_probes_the_plans_config(lib):
    pb = psp.FokkerPlanckEigenvalue(d=3, device='cpu')
    model = psp.EigenvalueSolver(pb, 't', verbose=False, device='cpu', K=48, N=5)
    assert pen.eigen_eligibility(_OnGpu(model)) is None
    plan = pen.EigenDeepPlan(model)
    (q1, probe), (q2, built) = lib.queries
    assert q1 == q2 == 'psp_genl_query_eig' and built == _snapshot(plan.gcfg)
    _agree(probe, built)
    assert (built['h_kind'], built['drift_kind'], built['domain_kind'], built['has_time']) == (16, 16, 2, 0)


def test_pinn_eligibility_probes_the_plans_config(lib):
    pb = psp.ExponentialOnSphereNonlinearParabolic(d=2, device='cpu')
    model = psp.GeneralSolver(problem=pb, name='t', verbose=False, device='cpu', K=24, loss_method='PINN', pinn_time_h='native')
    model.V = _tanh_net(3, [8, 8])
    assert 'GPU' in ppn.pinn_eligibility(model)                                             # (the device is asked last)
    plan = ppn.PinnNativePlan(model)
    names = [q[0] for q in lib.queries]
    assert names == ['psp_genl_query', 'psp_pinn_pairs_query', 'psp_pinn_pairs_query']
    assert lib.queries[1][1] == lib.queries[2][1] == _snapshot(plan.cfg)                    # K and all: the pair work area depends on it
    assert (plan.cfg.K, plan.cfg.h_kind, plan.cfg.has_time, plan.cfg.h_par[3]) == (24, 5, 1, 1.0)     # PSP_GH_EXPBALL_SIN, reads t


def test_value_eligibility_probes_the_plans_config(lib, monkeypatch):
    pb = psp.LQGC(d=3, off_diag=0.1, T=0.5, delta_t=0.05, device='cpu')
    model = psp.Solver('t', pb, K=40, delta_t=0.05, approx_method='value_function', time_approx='inner', detach_forward=True,
                       u_l2_error_flag=False, verbose=False, device='cpu', seed=1)
    assert pvn.value_eligibility(_OnGpu(model)) is None
    monkeypatch.setattr(pvn, 'value_eligibility', lambda s: None)                           # (the constructor asks again: the device)
    plan = pvn.ValueNativePlan(model)
    (q1, probe), (q2, built) = lib.queries[:2]
    assert (q1, q2) == ('psp_genl_query_ul2', 'psp_genl_query_lq')                          # (no log: the same check)
    assert built['d'] == plan.gcfg.base.d == 3 and built['K_local'] == 40                   # (the plan adds output pointers later)
    # the eligibility check does not read the step (the stub solvers of the host tests carry none): dt and what follows from it
    # are the plan's alone, as are time_first / time_scale (kernel_config.fill_value_net)
    _agree(probe, built, but=BATCH + ('dt', 'sqrt_dt', 'noise_mode', 'time_first', 'time_scale'))
    assert (built['sigma_kind'], built['sigma is set'], built['h_kind'], built['per_sample_weights']) == (1, True, 1, 1)
