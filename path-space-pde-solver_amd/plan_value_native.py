"""Native (HIP) plan for Solver.train with approx_method='value_function' (reference solver.py:93-97, 334-339, 438-440).

The ansatz is a value net Y_n(x) = V([t, x]) (DenseNet(d+1 -> 1), time_approx='inner'); the control enters through
Z_n = sigma grad_x V(X_n, n) (autograd with create_graph=True in the reference), Y starts at V(X_0, 0), and the loss is the
usual path-space loss of D = Y_N - g(X_N) plus the consistency term mean_k sum_{n=1}^{N-1} (V(X_n, n) - Y_n)^2
(`additional_loss`, solver.py:438-440, 499).  That is exactly the work of the GeneralSolver kernels (csrc/gen_kernels.h:
value net, reverse sweep for grad_x V, tangent pass for the theta-gradient of Z), with two additions made for this plan:
  * psp_gen_config.v_steps_out / y_steps_out : V(X_n, n) and the running Y at every step (the consistency term);
  * psp_gen_config.per_sample_weights        : the backward kernel takes the weight of the tangent part and the
                                               coefficient of grad_theta V PER SAMPLE (n, k) instead of per trajectory.
With the state path detached (detach_forward=True, or a non-adaptive forward process)
    dL/dtheta = sum_{m,k} WS[m,k] d(increment_m)/dtheta + sum_{n,k} AV[n,k] grad_theta V(X_n, n),
    WS[m] = w^D - (2/K) sum_{n=m+1}^{N-1} r_n,   AV[0] = WS[0],  AV[n] = (2/K) r_n  (1 <= n <= N-1),  r_n = V(X_n,n) - Y_n,
    w^D_k = dLoss/dD_k (log-variance: (2/K)(D_k - mean D), moment: (2/K) D_k).
Details that differ from GeneralSolver and are absorbed by the parameter index map (native_shapes.GenParamPad):
the net input is [t, x] with time FIRST (solver.py:343-344) and the reference feeds the STEP INDEX n as the time
(Y_n(X, n), solver.py:336, 439), while the kernel's time register holds n * dt: the time rows are moved to the kernels' last
input row and scaled by 1/dt on the way in (and the gradient on the way out).

Linear-quadratic coefficients (LLGC with off-diagonal entries, LQGC: a dense sigma B, a dense drift matrix A, the running cost
f(x) = sum_i p_i x_i^2): the ansatz takes Z = B grad_x V -- not B^T grad_x V as GeneralSolver does --, and h sees f at the state
AFTER the move (solver.py:338, 471-478).  Such cases always run on the run-time-shaped kernels (csrc/genl_kernels.h,
genl_fwd_kernel<NW, true, true>), whatever the net, through psp_genl_query_lq / psp_genl_rollout_fwd_lq with a psp_genl_coeffs
beside the config (``lq_coeffs``); the backward call and the weights above are the same, because the kernel stores the tangent
direction U = B^T u and f does not depend on the parameters while the state path is detached.

The u_L2 log (solver.py:471-475, 491-494; on by default whenever the problem has u_true): sum_n |-Z_n - u*(X_{n+1}, n dt)|^2 dt per
trajectory, accumulated inside the forward kernel (genl_fwd_kernel<.., LOGU>) from the description of u* that
plan_common.ul2_reference builds once per plan -- a table of u*(t_n) (LLGC), the gains of a u* linear in x (LQGC, staged
into the table scratch once by psp_genl_ul2_stage), the double wells' grid tables -- through psp_genl_query_ul2 /
psp_genl_rollout_fwd_ul2 with a psp_genl_ul2 beside the config and the coefficients.  Only the run-time-shaped family has log
instances (the templated (d, H) family does not: its instance list would double), so with the flag on EVERY net runs there
(input <= 112); with the flag off nothing changes: the same family selection, the same calls.

Gradients through the state path (adaptive_forward_process=True with detach_forward=False -- the constructor defaults; solver.py:
456-469 keeps c = -Z attached): refused unless Solver(value_state_path='native').  With it the plan is forward (unchanged),
psp_genl_adjoint_sweep, backward (unchanged).  At a fixed sample the loss still sees theta only through V(X_n, n) and
grad_x V(X_n, n), so the backward kernel's form  sum_{n,k} grad_theta [a_{n,k} V + grad_x V . U_{n,k}]  holds; what changes is
which a and U a sample gets.  The sweep (csrc/genl_adj_kernels.h, one workgroup per 16-trajectory tile, n = N-1 .. 0) runs the
adjoint lambda of the states from lambda_N = -w^D grad g(X_N) -- formed here by autograd on X_N, so the kernel does not know the
terminal cost --, the weights mu_n (mu_{n+1} = WS[n] above) and a_n (= AV above), rewrites the stored directions with
U_n = mu_{n+1} U_fwd - dt B^T (mu_{n+1} Z_n + B^T Lam) and fills the coefficient and tangent-weight arrays of the backward.
Only the run-time-shaped family has a sweep: every net goes through _deep_net(..., force=True), as with the log.
"""
import ctypes as C

import torch

try:
    from . import kernel_config as kc
    from . import native as nat
    from . import native_shapes as shapes
    from . import sharding
    from . import plan_common as pc
    from .function_space import DenseNet
    from .plan_common import PlanUnsupported
    from .plan_native import _overridden
except ImportError:
    import kernel_config as kc
    import native as nat
    import native_shapes as shapes
    import sharding
    import plan_common as pc
    from function_space import DenseNet
    from plan_common import PlanUnsupported
    from plan_native import _overridden


def value_eligibility(solver):
    """None if Solver(approx_method='value_function') can run on the GeneralSolver kernels, else the reason."""
    s = solver
    if s.device.type != 'cuda':
        return 'device is %s (the HIP rollout needs a GPU)' % s.device
    if s.approx_method != 'value_function' or s.time_approx != 'inner':
        return "only approx_method='value_function' with time_approx='inner' (with 'outer' the reference itself fails)"
    if s.loss_method not in ('log-variance', 'moment'):
        return "loss_method %r is not native for the value-function ansatz (log-variance, moment)" % s.loss_method
    attached = state_path_attached(s)
    if attached and getattr(s, 'value_state_path', 'torch') != 'native':
        return "detach_forward=False back-propagates through the state path (not native for the value-function ansatz by " \
               "default; value_state_path='native' runs the adjoint sweep of the run-time-shaped kernels)"
    if s.learn_Y_0:
        return 'learn_Y_0 has no meaning for the value-function ansatz (Y_0 = V(X_0, 0))'
    if s.burgers_drift or s.compute_gradient_variance > 0 or s.log_gradient \
            or s.metastability_logs is not None or s.IS_variance_K > 0:
        return 'per-step / per-iteration diagnostics (gradient logs, metastability, in-loop IS) are not native here'
    log = bool(s.u_l2_error_flag)
    if log:
        reason = pc.ul2_unsupported(s.problem, s.N, s.delta_t_np)
        if reason is not None:
            return reason
    nets = getattr(s, 'y_n', None)
    if not isinstance(nets, list) or len(nets) != 1:
        return 'y_n is not a single value net'
    V = nets[0]
    dims = getattr(V, 'nn_dims', None)
    deep = _deep_net(s, V)
    if deep is None and (not isinstance(V, DenseNet) or dims is None or len(dims) != 4 or dims[1] != dims[2] or dims[3] != 1
                         or dims[0] != s.d + 1):
        return 'the value net is neither a DenseNet(%d -> 1) with two equal hidden widths nor a dense-concat net the ' \
               'run-time-shaped kernels take (%s)' % (s.d + 1, _deep_net(s, V, why=True))
    spec_fn = getattr(s.problem, 'native_spec', None)
    spec = spec_fn() if spec_fn is not None else None
    if spec is None:
        return 'problem has no native_spec() (coefficients outside the native catalogue)'
    if nat.dnet_only_kind(spec) is not None:
        return nat.dnet_only_kind(spec)
    over = _overridden(s.problem)
    if over is not None:
        return 'problem.%s is not the catalogue implementation native_spec() describes' % over
    if spec['runcost'][0] not in (nat.RUNCOST_ZERO, nat.RUNCOST_DIAG_QUAD):
        return 'running cost kind %r is not built into the value-net kernels (zero / diagonal quadratic are)' % (spec['runcost'][0],)
    if not nat.is_built():
        raise nat.NativeLibraryError('libpsp_hip.so is not built; run __graft_entry__.build()')
    if needs_lq(spec) or log or attached:
        # a dense sigma, a dense drift matrix or a running cost -- or the u_L2 log or the adjoint sweep of the state path, which the
        # templated kernels do not carry: the run-time-shaped family only, whatever the net
        net = _deep_net(s, V, force=True)
        if net is None and needs_lq(spec):
            return 'a dense sigma / dense drift / running cost runs on the run-time-shaped value-net kernels only, and the ' \
                   'value net (input %d) is %s' % (s.d + 1, _deep_net(s, V, why=True, force=True))
        if net is None and not log:
            return "the adjoint sweep of the state path (value_state_path='native') runs on the run-time-shaped value-net " \
                   'kernels only, and the value net (input %d) is %s' % (s.d + 1, _deep_net(s, V, why=True, force=True))
        if net is None:
            return 'the u_L2 log (u_l2_error_flag=True) runs on the run-time-shaped value-net kernels only -- the templated ' \
                   '(d, H) kernels have no log instances --, and the value net (input %d) is %s; pass u_l2_error_flag=False ' \
                   'for the native plan' % (s.d + 1, _deep_net(s, V, why=True, force=True))
        keep = []                                         # (a query validates the pointers, it reads nothing)
        g = value_config(s, spec, net)[0]
        q = lq_coeffs(g, spec, torch.device('cpu'), keep)
        kc.probe(g)
        u = None
        if log:                                           # (a query reads no pointer: any non-null value stands for the buffers)
            probe = C.addressof(_PROBE)
            u = nat.GenlUl2(struct_bytes=C.sizeof(nat.GenlUl2), kind=pc.ul2_kind(s.problem), u_l2_out=probe, u_ref=probe,
                            tables=probe, group=probe, row=probe, ntables=1, nrows=1, ncols=1, xb=1.0, dx=1.0, K_global=1)
        lib = nat.load()
        qr, ur = C.byref(q) if q is not None else None, C.byref(u) if u is not None else None
        if attached:                                      # the sweep's images count as well
            adj = nat.GenlAdj(struct_bytes=C.sizeof(nat.GenlAdj))
            rc = lib.psp_genl_query_adj(C.byref(g), qr, ur, C.byref(adj), C.byref(nat.GenlSizes()))
        else:
            rc = lib.psp_genl_query_ul2(C.byref(g), qr, ur, C.byref(nat.GenlSizes()))
        if rc != 0:                                       # (the 160 KiB LDS rule)
            return lib.psp_last_error().decode()
        return None
    if deep is None and not shapes.gen_candidates(s.d, dims[1]):
        return 'no compiled kernel instance covers d=%d, H=%d (see csrc/gen_instances.def)' % (s.d, dims[1])
    return None


_PROBE = C.c_float(0.0)


def state_path_attached(solver):
    """Whether the loss back-propagates through the state path: the control -Z in the drift stays attached (solver.py:456-469)."""
    return bool(solver.adaptive_forward_process and not solver.detach_forward)


def needs_lq(spec):
    """Whether a native_spec() carries a coefficient only the linear-quadratic instances of the run-time-shaped kernels take."""
    return (spec['sigma'][0] == nat.SIGMA_DENSE or spec['drift'][0] == nat.DRIFT_DENSE
            or spec['runcost'][0] == nat.RUNCOST_DIAG_QUAD)


def value_config(s, spec, net):
    """(psp_genl_config or None, its base / the psp_gen_config) of the ansatz for a problem's ``native_spec()``: what does not
    depend on the batch and the step.  net: the ``_deep_net`` description (the run-time-shaped kernels) or None (the templated ones).
    ``lq_coeffs`` adds sigma and drift of a run-time-shaped config, kernel_config.fill_run the discretisation."""
    g = nat.GenlConfig() if net is not None else None
    cfg = g.base if g is not None else nat.GenConfig()
    if g is not None:
        cfg.d = s.d
        kc.fill_value_net(g, net, True)
    cfg.T = float('inf')                                  # no freezing: every trajectory takes all N steps (solver.py:440)
    cfg.d_real = s.d
    cfg.sigma_scale = float(spec['sigma'][2])
    cfg.drift_kind = spec['drift'][0]
    cfg.h_kind = nat.GH_QUAD                              # h = -|z|^2 / 2 (problems.py:46, 211, 321); f(x) travels in psp_genl_coeffs
    cfg.adaptive, cfg.store_path = (1 if s.adaptive_forward_process else 0), 1
    cfg.domain_kind, cfg.per_sample_weights = nat.DOM_NONE, 1
    return g, cfg


def _upload(M, shape, device, keep, what):
    return kc.upload(M, shape, device, keep, 'native_spec(): %s must have shape %s' % (what, shape))


def lq_coeffs(gcfg, spec, device, keep):
    """psp_genl_config.sigma_kind / sigma / base.sigma_scale / base.drift_kind / base.drift and the psp_genl_coeffs beside it from
    a problem's ``native_spec()`` (gcfg.base.d set).  Matrices and vectors are uploaded row-major in fp32 and kept alive in
    ``keep``.  Returns the nat.GenlCoeffs, or None where the spec needs none (identity sigma, element-wise drift, f = 0: the
    plain entry points' behaviour, Z = s grad_x V either way)."""
    d = int(gcfg.base.d)
    cfg = gcfg.base
    cfg.sigma_scale = float(spec['sigma'][2])
    if spec['sigma'][0] == nat.SIGMA_DENSE:
        gcfg.sigma_kind, gcfg.sigma = nat.GENL_SIGMA_DENSE, _upload(spec['sigma'][1], (d, d), device, keep, 'sigma').data_ptr()
    else:
        gcfg.sigma_kind, gcfg.sigma = nat.GENL_SIGMA_SCALED, None
    q = nat.GenlCoeffs(struct_bytes=C.sizeof(nat.GenlCoeffs), z_kind=nat.GENL_Z_SIGMA)
    kind, val = spec['drift']
    if kind == nat.DRIFT_DENSE:
        cfg.drift_kind, cfg.drift = nat.DRIFT_ZERO, None
        q.drift_matrix = _upload(val, (d, d), device, keep, 'the drift matrix').data_ptr()
    else:
        cfg.drift_kind = kind
        cfg.drift = _upload(val, (d,), device, keep, 'the drift vector').data_ptr() if val is not None else None
    if spec['runcost'][0] == nat.RUNCOST_DIAG_QUAD:
        q.runcost_kind = nat.RUNCOST_DIAG_QUAD
        q.runcost = _upload(spec['runcost'][1], (d,), device, keep, 'the running-cost vector').data_ptr()
    return q if needs_lq(spec) else None


def _deep_net(solver, V, why=False, force=False):
    """The dense-concat description of a value net that is NOT the two-equal-hidden-layer relu^2 DenseNet of the templated kernels
    (any depth 1-4, widths <= 128, relu^2 / tanh^2 / tanh: csrc/genl_kernels.h), or None (why=True: the reason instead).
    force: also for a net the templated kernels would take (the linear-quadratic coefficients run on this family only)."""
    try:
        from . import plan_general_deep as pgd
    except ImportError:
        import plan_general_deep as pgd
    spec = pgd.value_net_spec(V, solver.d + 1)
    if isinstance(spec, str):
        return spec if why else None
    dims = spec['dims']
    templated = (isinstance(V, DenseNet) and len(dims) == 4 and dims[1] == dims[2] and spec['act'] == 'relu2'
                 and bool(shapes.gen_candidates(solver.d, dims[1])))
    if templated and not force:
        return 'the templated kernels take it' if why else None
    short = kc.value_net_limits_reason(dims)[2]
    if short is not None:
        return short if why else None
    return 'ok' if why else spec


class ValueNativePlan:
    def __init__(self, solver, noise='reference'):
        reason = value_eligibility(solver)
        if reason is not None:
            raise PlanUnsupported(reason)
        s = solver
        self.s, self.noise, self.lib, self.dev = s, noise, nat.load(), s.device
        dev = self.dev
        self.dist, self.rank, self.world, lo, hi = pc.local_shard(s.K)
        self.lo, self.hi, self.K_local = lo, hi, hi - lo
        self.net = s.y_n[0]
        self.key = None
        self.H = self.net.nn_dims[1]
        spec = s.problem.native_spec()
        self.log = bool(s.u_l2_error_flag)                # the u_L2 log: the run-time-shaped family, whatever the net
        self.attached = state_path_attached(s)            # the adjoint sweep of the state path: the run-time-shaped family as well
        self.adj = None                                   # its psp_genl_adj
        self.deep = _deep_net(s, self.net, force=needs_lq(spec) or self.log or self.attached)     # value nets of other depths / activations: csrc/genl_kernels.h
        # registration order W1,b1,W2,b2,.. (include/psp.h)
        self.params = list(self.net.W) if self.deep is None else list(self.deep['params'])
        self.flat = pc.rehome_params(self.params, dev)
        self.P = self.flat.numel()
        self._keep = []
        self.coeffs = None                                # psp_genl_coeffs (dense sigma / drift matrix / running cost), deep plans only
        self.ul2, self.ul2_cfg = None, None               # per-trajectory u_L2 (K_local) and its psp_genl_ul2, with the log on
        gcfg, cfg = value_config(s, spec, self.deep)
        if gcfg is not None:
            self.gcfg = gcfg
        kc.fill_run(cfg, s, self.K_local, lo, noise)
        drift_vec = spec['drift'][1]
        if self.deep is not None:
            self.coeffs = lq_coeffs(self.gcfg, spec, dev, self._keep)
        elif drift_vec is not None:
            unpadded = []                                 # (the size query validates the pointer: the unpadded vector will do)
            cfg.drift = nat.ptr(kc.upload(drift_vec, None, dev, unpadded, 'the drift vector'))
        f32 = torch.float32
        self.Kpad = 16 * ((self.K_local + 15) // 16)
        if self.deep is not None:
            try:
                from .plan_general_deep import _IdentityPad
            except ImportError:
                from plan_general_deep import _IdentityPad
            g = self.gcfg
            g.time_first, g.time_scale = 1, 1.0 / cfg.dt               # input [t, x], and t is the step index (solver.py:336-338, 439)
            sz = nat.GenlSizes()
            if self.log:
                self._make_ul2()
            if self.attached:
                self.adj = nat.GenlAdj(struct_bytes=C.sizeof(nat.GenlAdj))
                rc = self.lib.psp_genl_query_adj(C.byref(g), self._coeffs_ref(), C.byref(self.ul2_cfg) if self.log else None,
                                                 C.byref(self.adj), C.byref(sz))
            elif self.log:
                rc = self.lib.psp_genl_query_ul2(C.byref(g), self._coeffs_ref(), C.byref(self.ul2_cfg), C.byref(sz))
            else:
                rc = self.lib.psp_genl_query_lq(C.byref(g), self._coeffs_ref(), C.byref(sz))
            if rc != 0:
                raise PlanUnsupported(self.lib.psp_last_error().decode())
            assert sz.n_params == self.P, (sz.n_params, self.P)
            self.d_pad, self.H_pad = s.d, self.H
            self.pad = _IdentityPad(self.P)
            self.flat_k = self.flat
            self.tables = torch.empty(sz.table_bytes // 4, dtype=f32, device=dev)
            if self.ul2_cfg is not None:                  # PSP_UL2_LINEAR: the gains go into the table scratch once
                nat.check(self.lib.psp_genl_ul2_stage(C.byref(g), self._coeffs_ref(), C.byref(self.ul2_cfg), nat.ptr(self.tables),
                                                      nat.stream_ptr(dev)), 'psp_genl_ul2_stage')
            self.ahat_buf = torch.zeros((sz.ahat_bytes + 3) // 4, dtype=f32, device=dev)      # coefficients, then the tiles' step counts
            self.ahat = self.ahat_buf[:(s.N + 1) * self.Kpad].view(s.N + 1, self.Kpad)
        else:
            chosen, why = shapes.gen_choose(cfg, s.d, self.H)
            if chosen is None:
                raise PlanUnsupported(why)
            self.d_pad, self.H_pad, sz = chosen
            self.pad = shapes.GenParamPad(s.d, self.H, self.d_pad, self.H_pad, dev, time_input=True, time_first=True,
                                          time_scale=1.0 / cfg.dt)
            if drift_vec is not None:
                cfg.drift = nat.ptr(kc.upload(self.pad.vec(drift_vec.detach().to(device=dev, dtype=torch.float32)), None, dev,
                                              self._keep, 'the drift vector'))
            assert sz.n_params == self.pad.Pp, (sz.n_params, self.pad.Pp)
            self.flat_k = self.pad.new_padded_params()
            self.ahat = torch.zeros(s.N + 1, self.Kpad, dtype=f32, device=dev)       # written by the forward, then overwritten by AV
        self.sizes = sz
        self.path = torch.empty(sz.path_bytes // 4, dtype=f32, device=dev)
        self.ws = torch.zeros(s.N + 1, self.Kpad, dtype=f32, device=dev)
        if self.adj is not None:                          # the sweep's inputs: mu_n, a_n, the terminal adjoint; its dLoss/dX_0
            self.mu = torch.zeros(s.N + 1, self.Kpad, dtype=f32, device=dev)
            self.resid = torch.zeros(s.N + 1, self.Kpad, dtype=f32, device=dev)
            self.lamN = torch.zeros(self.K_local, s.d, dtype=f32, device=dev)
            self.lam0 = torch.zeros(self.K_local, s.d, dtype=f32, device=dev)
            self.adj.mu, self.adj.resid_coeff = self.mu.data_ptr(), self.resid.data_ptr()
            self.adj.lam_N, self.adj.lam0_out = self.lamN.data_ptr(), self.lam0.data_ptr()
        self.vsteps = torch.zeros(s.N, self.Kpad, dtype=f32, device=dev)
        self.ysteps = torch.zeros(s.N, self.Kpad, dtype=f32, device=dev)
        cfg.v_steps_out, cfg.y_steps_out = nat.ptr(self.vsteps), nat.ptr(self.ysteps)
        self.cfg = cfg
        self.grad_partial = torch.empty(sz.grad_partial_bytes // 4, dtype=f32, device=dev)
        self.VN = torch.empty(self.K_local, dtype=f32, device=dev)
        self.YN = torch.empty(self.K_local, dtype=f32, device=dev)
        self.tN = torch.empty(self.K_local, dtype=f32, device=dev)
        self.XN_k = torch.empty(self.K_local, self.d_pad, dtype=f32, device=dev)
        self.D = torch.empty(self.K_local, dtype=f32, device=dev)
        self.kcount = torch.zeros(1, dtype=torch.int64, device=dev)
        self.t0 = torch.zeros(self.K_local, dtype=f32, device=dev)
        self.grad = torch.empty(self.P, dtype=f32, device=dev)
        self.grad_k = self.grad if self.deep is not None else torch.empty(self.pad.Pp, dtype=f32, device=dev)
        self.m = torch.zeros(self.P, dtype=f32, device=dev)
        self.v = torch.zeros(self.P, dtype=f32, device=dev)
        self.sums = torch.zeros(2, dtype=torch.float64, device=dev)
        self.x0_row = s.X_0.detach().to(device=dev, dtype=f32).reshape(1, -1)
        self.step = 0
        self.events = None

    def _make_ul2(self):
        """psp_genl_ul2 from plan_common.ul2_reference (unpadded: the kernel reads (N, d) / (N, d, d) / (d) arrays)."""
        s, dev = self.s, self.dev
        try:
            ref = pc.ul2_reference(s.problem, s.N, s.delta_t_np, s.d, s.K, self.lo)
        except ValueError as e:
            raise PlanUnsupported(str(e))
        if ref is None:
            raise PlanUnsupported(pc.ul2_unsupported(s.problem, s.N, s.delta_t_np))

        def up(t, dtype=torch.float32):
            t = t.detach().to(device=dev, dtype=dtype).contiguous()
            self._keep.append(t)
            return t.data_ptr()

        self.ul2 = torch.zeros(self.K_local, dtype=torch.float32, device=dev)
        u = nat.GenlUl2(struct_bytes=C.sizeof(nat.GenlUl2), kind=ref['kind'], K_global=int(s.K))
        u.u_l2_out = self.ul2.data_ptr()
        if ref['kind'] == nat.UL2_TABLE:
            u.u_ref = up(ref['table'])
        elif ref['kind'] == nat.UL2_LINEAR:
            u.tables = up(ref['gains'])
        else:
            u.tables = up(ref['tables'])
            u.group, u.row = up(ref['group'], torch.int32), up(ref['row'], torch.int32)
            u.ntables, u.nrows, u.ncols = ref['tables'].shape[0], ref['nrows'], ref['ncols']
            u.xb, u.dx, u.xhi = ref['xb'], ref['dx'], ref['xhi']
        self.ul2_ref, self.ul2_cfg = ref, u

    def _coeffs_ref(self):
        return C.byref(self.coeffs) if self.coeffs is not None else None

    def iteration(self, l, loss_out, ul2_out=None):
        s, lib, cfg, dev = self.s, self.lib, self.cfg, self.dev
        st = nat.stream_ptr(dev)
        K, N = float(s.K), s.N
        lo, hi = self.lo, self.hi
        # ---- initial state and noise in the reference's order (solver.py:364-382)
        xi, x0 = pc.draw_noise(s, l, self.noise, lo, self.K_local, self.d_pad, dev)
        if xi is not None:
            xi = xi[1:]                                           # the kernels' slot n = the reference's xi[:, :, n + 1]
        if x0 is None:                                            # these kernels take one start point per trajectory
            x0 = self.pad.last_dim(self.x0_row.repeat(self.K_local, 1))
        flat_k = self.flat if self.deep is not None else self.pad.scatter_params(self.flat, self.flat_k)
        self.kcount.zero_()
        ev = None
        if self.events is not None:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
        if self.ul2_cfg is not None:
            nat.check(lib.psp_genl_rollout_fwd_ul2(C.byref(self.gcfg), self._coeffs_ref(), C.byref(self.ul2_cfg), nat.ptr(self.flat),
                                                   nat.ptr(x0), nat.ptr(self.t0), nat.ptr(xi), int(s.seed) & 0xFFFFFFFFFFFFFFFF, l,
                                                   nat.ptr(self.tables), nat.ptr(self.path), nat.ptr(self.ahat_buf), nat.ptr(self.VN),
                                                   nat.ptr(self.YN), nat.ptr(self.XN_k), nat.ptr(self.tN), nat.ptr(self.kcount), st),
                      'psp_genl_rollout_fwd_ul2')
        elif self.deep is not None:
            nat.check(lib.psp_genl_rollout_fwd_lq(C.byref(self.gcfg), self._coeffs_ref(), nat.ptr(self.flat), nat.ptr(x0),
                                                  nat.ptr(self.t0), nat.ptr(xi), int(s.seed) & 0xFFFFFFFFFFFFFFFF, l,
                                                  nat.ptr(self.tables), nat.ptr(self.path), nat.ptr(self.ahat_buf), nat.ptr(self.VN),
                                                  nat.ptr(self.YN), nat.ptr(self.XN_k), nat.ptr(self.tN), nat.ptr(self.kcount), st),
                      'psp_genl_rollout_fwd_lq')
        else:
            nat.check(lib.psp_gen_rollout_fwd(C.byref(cfg), nat.ptr(flat_k), nat.ptr(x0), nat.ptr(self.t0), nat.ptr(xi),
                                              int(s.seed) & 0xFFFFFFFFFFFFFFFF, l, nat.ptr(self.path), nat.ptr(self.ahat),
                                              nat.ptr(self.VN), nat.ptr(self.YN), nat.ptr(self.XN_k), nat.ptr(self.tN),
                                              nat.ptr(self.kcount), st), 'psp_gen_rollout_fwd')
        if ev is not None:
            ev[1].record()
        # ---- loss (solver.py:164-168, 499) and the per-sample weights
        XN = self.XN_k[:, :s.d]
        torch.sub(self.YN, s.problem.g(XN).to(torch.float32), out=self.D)
        Dd = self.D.double()
        r = (self.vsteps - self.ysteps)[:, :self.K_local]
        r[0].zero_()                                              # the term starts at n = 1 (solver.py:438)
        stats = [Dd.sum(), (Dd * Dd).sum(), (r.double() ** 2).sum()]
        if self.ul2 is not None:                                  # the local sum of the log rides on the same collective
            stats.append(self.ul2.double().sum())
        stats = torch.stack(stats)
        sharding.allreduce_sum_(stats)                            # collective 1
        if self.ul2 is not None and ul2_out is not None:
            ul2_out[l:l + 1] = (stats[3:4] / K).to(torch.float32)  # mean over the GLOBAL K, no host sync
        self.sums.copy_(stats[:2])
        loss = sharding.loss_from_sums(self.sums, s.K, s.loss_method) + stats[2] / K
        loss_out[l] = loss.to(torch.float32)
        wD = sharding.loss_weights(self.D, self.sums, s.K, s.loss_method)            # (K_local)
        tail = torch.flip(torch.cumsum(torch.flip(r, [0]), 0), [0])                 # tail[m] = sum_{n >= m} r_n
        ws, av = self.ws, self.ahat
        if self.adj is not None:                                  # the sweep writes ws and av from mu (= WS shifted by one) and a_n
            ws, av = self.mu[1:], self.resid
        ws.zero_()
        av.zero_()
        # WS[m] = w^D - (2/K) sum_{n > m} r_n  (m = 0..N-1);  AV[0] = WS[0] + ... = w^D - (2/K) sum_{n >= 1} r_n
        ws[:N - 1, :self.K_local] = wD.unsqueeze(0) - (2.0 / K) * tail[1:]
        ws[N - 1, :self.K_local] = wD
        av[1:N, :self.K_local] = (2.0 / K) * r[1:]
        av[0, :self.K_local] = ws[0, :self.K_local]
        if self.adj is not None:
            # lambda_N = -w^D grad g(X_N) by autograd on X_N (the kernel stays independent of the terminal cost), then the sweep:
            # it rewrites the stored directions and fills the coefficient and tangent-weight arrays the backward reads
            with torch.enable_grad():
                xN = XN.detach().clone().requires_grad_(True)
                dg, = torch.autograd.grad(s.problem.g(xN).sum(), xN)
            torch.mul(dg.to(torch.float32), -wD.unsqueeze(1), out=self.lamN)
            ws = self.ws
            nat.check(lib.psp_genl_adjoint_sweep(C.byref(self.gcfg), self._coeffs_ref(), C.byref(self.adj), nat.ptr(self.flat),
                                                 nat.ptr(self.tables), nat.ptr(self.path), nat.ptr(self.ahat_buf), nat.ptr(ws), st),
                      'psp_genl_adjoint_sweep')
        if ev is not None:
            ev[2].record()
        if self.deep is not None:
            nat.check(lib.psp_genl_rollout_bwd(C.byref(self.gcfg), nat.ptr(self.flat), nat.ptr(self.tables), nat.ptr(self.path),
                                               nat.ptr(self.ahat_buf), nat.ptr(ws), None, nat.ptr(self.grad_partial),
                                               nat.ptr(self.grad), st), 'psp_genl_rollout_bwd')
        else:
            nat.check(lib.psp_gen_rollout_bwd(C.byref(cfg), nat.ptr(flat_k), nat.ptr(self.path), nat.ptr(av), nat.ptr(ws), None,
                                              nat.ptr(self.grad_partial), nat.ptr(self.grad_k), st), 'psp_gen_rollout_bwd')
            self.pad.gather_grad(self.grad_k, self.grad)
        if ev is not None:
            ev[3].record()
            self.events.append(ev)
        sharding.allreduce_sum_(self.grad)                        # collective 2
        self.step += 1
        pc.adam_step(lib, self.flat, self.grad, self.m, self.v, self.P, self.step,
                     pc.adam_hyper(self.net, s.lr, PlanUnsupported), st)
        return loss
