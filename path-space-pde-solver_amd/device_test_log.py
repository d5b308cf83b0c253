"""The K_test_log diagnostic on the device (psp_genl_test_error, csrc/genl_eval_kernels.h): host side.

``eval_reason`` says why a problem cannot be served (None: it can), ``DeviceTestLog`` owns the scratch and the (L, 4) fp64 log of
one (net, problem, K) and enqueues the two kernels -- no host sync until ``read``.  Used by the native plans of GeneralSolver /
EllipticSolver (``test_log='device'``) and by ``utilities.compute_test_error_native``.

The sampler's stream (include/psp.h): Philox4x32-7, key (seed & 0xffffffff, (seed >> 32) ^ 0x54455354), counter
(point index, c1, c2, iteration) -- disjoint from every training stream, which key on the seed itself.
"""
import ctypes as C

import torch

try:
    from . import kernel_config as kc
    from . import native as nat
    from .problems import coefficients_overridden
except ImportError:
    import kernel_config as kc
    import native as nat
    from problems import coefficients_overridden

_ACT = kc.ACT


def domain_spec(problem):
    """(sample kind, bound_a, bound_b) of the problem's domain, or a reason string."""
    b = getattr(problem, 'boundary', None)
    if b in ('sphere', 'unbounded'):
        return nat.TSAMPLE_BALL, 0.0, float(problem.boundary_distance)
    if b == 'two_spheres':
        return nat.TSAMPLE_ANNULUS, float(problem.boundary_distance_1), float(problem.boundary_distance_2)
    if b in ('square', 'unbounded_square'):
        return nat.TSAMPLE_BOX, float(problem.X_l), float(problem.X_r)
    return 'the device test log does not sample the domain %r' % (b,)


def eval_reason(problem):
    """Why the device test log cannot serve this problem (its solution or its domain), else None."""
    fn = getattr(problem, 'native_vtrue_spec', None)
    if fn is None:
        if hasattr(problem, 'psi') or hasattr(type(problem), 'compute_reference_solution'):
            return ('problem has no native_vtrue_spec(): its v_true reads a table (compute_reference_solution()); the device '
                    'test log has closed forms only, the table stays on the host log')
        return 'problem has no native_vtrue_spec() (no closed-form v_true in the native catalogue)'
    if coefficients_overridden(problem, names=('v_true',)) is not None:
        return 'problem.v_true is not the catalogue implementation native_vtrue_spec() describes'
    dom = domain_spec(problem)
    return dom if isinstance(dom, str) else None


def eval_config(net_spec, problem, K, modus, slots=1, k_offset=0):
    """psp_genl_eval_config of a value net (plan_general_deep.value_net_spec) on a problem eval_reason() accepts."""
    cfg = nat.GenlEvalConfig()
    cfg.d = int(problem.d)
    kc.fill_value_net(cfg, net_spec, modus == 'parabolic')
    cfg.K_points, cfg.k_offset = int(K), int(k_offset)
    cfg.sample_kind, cfg.bound_a, cfg.bound_b = domain_spec(problem)
    cfg.T = float(getattr(problem, 'T', 0.0)) if cfg.has_time else 0.0
    vt = problem.native_vtrue_spec()
    cfg.vtrue_kind = int(vt['kind'])
    for i, v in enumerate(vt['par']):
        cfg.vtrue_par[i] = float(v)
    cfg.log_slots = int(slots)
    return cfg


def eval_query(cfg):
    """(sizes, '') or (None, the library's reason)."""
    sizes = nat.GenlEvalSizes()
    lib = nat.load()
    if lib.psp_genl_eval_query(C.byref(cfg), C.byref(sizes)) != 0:
        return None, lib.psp_last_error().decode()
    return sizes, ''


class DeviceTestLog:
    def __init__(self, net_spec, problem, K, modus, device, slots=1):
        self.lib = nat.load()
        self.dev = torch.device(device)
        self.cfg = eval_config(net_spec, problem, K, modus, slots)
        sizes, why = eval_query(self.cfg)
        if sizes is None:
            raise ValueError(why)
        self.sizes = sizes
        self.tables = torch.empty(sizes.table_bytes // 4, dtype=torch.float32, device=self.dev)
        self.partial = torch.empty(sizes.partial_bytes // 8, dtype=torch.float64, device=self.dev)
        self.begin(slots)

    def begin(self, slots):
        """A fresh log of `slots` rows (one per iteration of a train() call)."""
        self.cfg.log_slots = int(slots)
        self.log = torch.zeros(int(slots), 4, dtype=torch.float64, device=self.dev)
        self.used = 0

    def enqueue(self, flat_params, seed, iteration, slot, stream, dumps=None):
        """Both kernels on `stream`; nothing is read back.  dumps: optional dict of device tensors x, t, v, v_true, keep."""
        assert flat_params.dtype == torch.float32 and flat_params.numel() == self.sizes.n_params
        d = dumps or {}
        nat.check(self.lib.psp_genl_test_error(
            C.byref(self.cfg), nat.ptr(flat_params), None, None, int(seed) & 0xFFFFFFFFFFFFFFFF, int(iteration),
            nat.ptr(self.tables), nat.ptr(self.partial), nat.ptr(self.log), int(slot), None,
            nat.ptr(d.get('x')), nat.ptr(d.get('t')), nat.ptr(d.get('v')), nat.ptr(d.get('v_true')), nat.ptr(d.get('keep')),
            stream), 'psp_genl_test_error')
        self.used = max(self.used, int(slot) + 1)

    def read(self):
        """One read-back: (L2, abs, rel) lists of the slots written so far -- the means over the kept points, as
        compute_test_error forms them."""
        rows = self.log[:self.used].cpu().numpy()
        cnt = rows[:, 3]
        return [(rows[:, i] / cnt).tolist() for i in range(3)]
