"""Native execution plan for Solver.train with a linear, affine or constant control per time step: time_approx='outer' with
``model.z_n`` a list of N function_space.Linear / Affine / Constant modules (reference function_space.py:24-63; the notebook
`Ornstein-Uhlenbeck - quadratic costs - linear ansatz.ipynb` swaps N Linear modules into the solver).

The control family is Z_n(x) = M_n x + c_n:

    module              M_n                              c_n     trainable      chain rule back to the module
    Linear(d, B, Q)     G_n F_n, G_n = Q_n^-1 B_n^T      -       F_n (d x d)    dF_n = G_n^T dM_n
    Affine(d)           A_n                              b_n     A_n, b_n       identity
    Constant(d)         -                                c_n     c_n            identity

The kernels (csrc/aff_kernels.h behind psp_aff_*, include/psp.h) see the effective maps (M, c) zero padded to the d bucket and
return (dM, dc).  G_n and the chain rule stay here as batched torch ops on the device (tiny, no host sync); with G_n = I (the
notebook) the product is skipped, so M is F bit for bit.

Per iteration (reference solver.py:430-514):
    psp_aff_rollout_fwd      D_k, X_N, Y_N, the u_L2 log and the path store [X_n | image]
    psp_aff_terminal_reduce  (sum D, sum D^2)                                           [all-reduce 1]
    psp_aff_adjoint_sweep    only with adaptive_forward_process=True and detach_forward=False: the image becomes dL/dZ_n / sqrt(dt)
    psp_aff_rollout_bwd      per (step, slice) partial (dM_n, dc_n); slices summed in order  [all-reduce 2]
    psp_adam_step            one fused Adam over the concatenation of all parameter sets
"""
import ctypes as C

import torch

try:
    from . import native as nat
    from . import sharding
    from . import plan_common as pc
    from .function_space import Affine, Constant, Linear
    from .plan_common import PlanUnsupported, ul2_kind, ul2_reference, ul2_unsupported
    from .plan_native import _overridden
except ImportError:
    import native as nat
    import sharding
    import plan_common as pc
    from function_space import Affine, Constant, Linear
    from plan_common import PlanUnsupported, ul2_kind, ul2_reference, ul2_unsupported
    from plan_native import _overridden

_LOSSES = ('log-variance', 'moment', 'variance', 'cross_entropy', 'relative_entropy')
_CLASSES = (Linear, Affine, Constant)
MAX_D = 64
_BUCKETS = (16, 32, 64)                  # csrc/aff_instance.hip (psp_aff_instance_get lists the same)


def bucket_for(d):
    for b in _BUCKETS:
        if d <= b:
            return b
    return None


def control_class(z_n):
    """Linear, Affine or Constant if z_n is a non-empty list of modules of exactly that class whose forward is the class's own,
    else None."""
    if not isinstance(z_n, list) or not z_n:
        return None
    cls = type(z_n[0])
    if cls not in _CLASSES:
        return None
    for m in z_n:
        if type(m) is not cls or 'forward' in vars(m):
            return None
    return cls


def _plain_adam(mods):
    """None if every module carries a plain torch.optim.Adam with the same hyper-parameters, else the reason."""
    hyp = None
    for m in mods:
        opt = getattr(m, 'optim', None)
        if opt is None or type(opt) is not torch.optim.Adam or len(opt.param_groups) != 1:
            return 'every module of z_n must carry its own plain torch.optim.Adam (function_space.py); found %s' % (
                type(opt).__name__ if opt is not None else 'no optimiser')
        g = opt.param_groups[0]
        if g.get('weight_decay', 0) or g.get('amsgrad', False) or g.get('maximize', False):
            return 'the native Adam implements weight_decay = 0, amsgrad = False, maximize = False'
        h = (float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']))
        if hyp is not None and h != hyp:
            return 'the per-step modules carry different Adam settings; the fused native Adam needs one'
        hyp = h
    return None


def affine_eligibility(solver):
    """None if the solver can run on this plan, else a human-readable reason."""
    s = solver
    if s.device.type != 'cuda':
        return 'device is %s (the HIP rollout needs a GPU)' % s.device
    return affine_configuration_reason(s)


def affine_configuration_reason(s):
    """Everything affine_eligibility checks except the device (so that it can be tested without a GPU)."""
    if s.approx_method != 'control':
        return "only approx_method='control' is native for a linear / affine / constant control"
    if s.time_approx != 'outer':
        return "a linear / affine / constant control needs time_approx='outer' (the modules take x, not [t, x])"
    cls = control_class(getattr(s, 'z_n', None))
    if cls is None:
        return 'z_n is not a list of modules of exactly one of Linear, Affine, Constant with the class forward'
    if len(s.z_n) != s.N:
        return "time_approx='outer' needs one module per time step (%d modules, N = %d)" % (len(s.z_n), s.N)
    if s.d > MAX_D:
        return 'd = %d is outside the native range d <= %d of the linear-control kernels' % (s.d, MAX_D)
    if s.loss_method not in _LOSSES:
        return 'loss_method %r is not native for a linear control (%s are)' % (s.loss_method, ', '.join(_LOSSES))
    if s.loss_method == 'relative_entropy' and not s.adaptive_forward_process:
        return 'relative_entropy with a non-adaptive forward process is not native for a linear control'
    if s.burgers_drift or s.compute_gradient_variance > 0 or s.log_gradient or s.metastability_logs is not None:
        return 'per-step / per-iteration diagnostics (burgers_drift, gradient logs / variances, metastability) are not native here'
    if getattr(s, 'mlp_dtype', 'auto') not in ('auto', 'fp32'):
        return "mlp_dtype=%r: the linear-control kernels compute in fp32 only ('auto' or 'fp32')" % s.mlp_dtype
    spec_fn = getattr(s.problem, 'native_spec', None)
    if spec_fn is None or spec_fn() is None:
        return 'problem has no native_spec() (coefficients outside the native catalogue)'
    if nat.dnet_only_kind(spec_fn()) is not None:
        return nat.dnet_only_kind(spec_fn())
    over = _overridden(s.problem)
    if over is not None:
        return 'problem.%s is not the catalogue implementation native_spec() describes' % over
    if s.u_l2_error_flag:
        kind = ul2_kind(s.problem)
        if kind == nat.UL2_GRID:
            return ('the u_L2 log against grid tables (PSP_UL2_GRID: u_true_tables()) is not built for linear controls; '
                    'pass u_l2_error_flag=False for the native plan')
        reason = ul2_unsupported(s.problem, s.N, s.delta_t_np)
        if reason is not None:
            return reason
    for m in s.z_n:
        for p in m.parameters():
            if p.shape not in ((s.d, s.d), (1, s.d), (s.d,)) or p.dtype != torch.float32:
                return 'a module of z_n has a parameter of shape %s; the control must map R^%d to R^%d' % (tuple(p.shape), s.d, s.d)
    reason = _plain_adam(s.z_n + ([s.y_0] if s.learn_Y_0 else []))
    if reason is not None:
        return reason
    need = path_store_bytes(s)
    budget = s.path_budget_bytes
    if budget is not None and need > budget:
        return ('the path store needs %d bytes, path_budget_bytes is %d; the linear-control plan does not chunk' % (need, budget))
    return None


def path_store_bytes(s):
    _, world = sharding.dist_info()[1:]
    return int(s.N) * (int(s.K) // max(1, world)) * 2 * bucket_for(s.d) * 4


def linear_gains(mods, dev):
    """(N, d, d) G_n = Q_n^-1 B_n^T of a list of Linear modules on `dev`, or None when every G_n is exactly the identity."""
    G = torch.stack([torch.mm(torch.as_tensor(m.Q, dtype=torch.float32).to(dev).inverse(),
                              torch.as_tensor(m.B, dtype=torch.float32).to(dev).t()) for m in mods])
    eye = torch.eye(G.shape[1], device=dev).expand_as(G)
    return None if bool(torch.equal(G, eye)) else G.contiguous()


def effective_map(G, F):
    """M_n = G_n F_n (G None: F itself)."""
    return F if G is None else torch.bmm(G, F)


def chain_rule(G, dM):
    """dF_n = G_n^T dM_n (G None: dM itself)."""
    return dM if G is None else torch.bmm(G.transpose(1, 2), dM)


def step_index(model, N_eval, delta_t):
    """The module the reference evaluates at step n of a grid of N_eval steps of delta_t: Z_n(X, n delta_t) takes the index
    ceil(t / model.delta_t) in fp32 (solver.py:360-362) and clamps it to the list (solver.py:352-353)."""
    dt32 = model.delta_t.detach().cpu()
    out = []
    for n in range(N_eval):
        t = torch.as_tensor(n * delta_t, dtype=torch.float32)
        out.append(max(0, min(int(torch.ceil(t / dt32)), model.N - 1)))
    return out


def is_control_tables(model, N_eval, delta_t):
    """What psp_is_rollout needs to evaluate u = -Z_n on a grid of N_eval steps (include/psp.h PSP_ISC_*):
    (ISC_LINEAR, (N_eval, d, d) gains -M_idx(n)) for a Linear list, (ISC_TABLE, (N_eval, d) rows -c_idx(n)) for a Constant list,
    None for anything else (Affine has both parts: the reference-control rollout has no such kind)."""
    cls = control_class(getattr(model, 'z_n', None))
    if cls not in (Linear, Constant) or model.time_approx != 'outer' or model.approx_method != 'control':
        return None
    dev = model.device
    idx = torch.tensor(step_index(model, N_eval, delta_t), dtype=torch.long, device=dev)
    with torch.no_grad():
        if cls is Linear:
            F = torch.stack([m.F.detach() for m in model.z_n]).to(dev)
            M = effective_map(linear_gains(model.z_n, dev), F)
            return nat.ISC_LINEAR, (-M.index_select(0, idx)).contiguous()
        c = torch.stack([m.c.detach() for m in model.z_n]).to(dev)
        return nat.ISC_TABLE, (-c.index_select(0, idx)).contiguous()


class AffineNativePlan:
    def __init__(self, solver, noise='reference'):
        reason = affine_eligibility(solver)
        if reason is not None:
            raise PlanUnsupported(reason)
        s = solver
        if not nat.is_built():
            raise nat.NativeLibraryError('libpsp_hip.so is not built; run __graft_entry__.build()')
        self.s, self.noise, self.lib, self.dev = s, noise, nat.load(), s.device
        dev = self.dev
        self.dist, self.rank, self.world, lo, hi = pc.local_shard(s.K)
        self.K_local, self.k_offset = hi - lo, lo
        self.mods = list(s.z_n)
        self.net = s.z_n
        self.cls = control_class(s.z_n)
        self.has_matrix, self.has_bias = self.cls is not Constant, self.cls is not Linear
        d, N = s.d, s.N
        self.d_pad = DB = bucket_for(d)
        self.G = linear_gains(self.mods, dev) if self.cls is Linear else None
        self._flatten()
        spec = s.problem.native_spec()
        self._keep = []

        def padded(t):
            """vector (d) -> (DB), matrix (d, d) -> (DB, DB), zero padded fp32 on the device"""
            if t is None:
                return None
            t = torch.as_tensor(t).detach().to(device=dev, dtype=torch.float32)
            out = torch.zeros(*([DB] * t.dim()), dtype=torch.float32, device=dev)
            out[tuple(slice(0, n) for n in t.shape)] = t
            self._keep.append(out)
            return out

        cfg = nat.AffConfig()
        cfg.struct_bytes = C.sizeof(nat.AffConfig)
        b = cfg.base
        b.d, b.H = DB, 0
        self.generic_loss, self.relent, self.attached = pc.fill_hjb_base(b, s, spec, noise, self.K_local, self.k_offset)
        b.mlp_dtype = nat.MLP_FP32
        b.drift = nat.ptr(padded(spec['drift'][1]))
        b.sigma = nat.ptr(padded(spec['sigma'][1]))
        b.runcost = nat.ptr(padded(spec['runcost'][1]))
        b.term = nat.ptr(padded(spec['term'][1]))
        cfg.d_real, cfg.has_matrix, cfg.has_bias = d, int(self.has_matrix), int(self.has_bias)
        self.cfg = cfg
        f32 = torch.float32
        self.ul2 = None
        if s.u_l2_error_flag:
            try:
                ref = ul2_reference(s.problem, N, s.delta_t_np, DB, s.K, self.k_offset)
            except ValueError as e:
                raise PlanUnsupported(str(e))
            self.ul2 = torch.zeros(self.K_local, dtype=f32, device=dev)
            b.u_l2_out = nat.ptr(self.ul2)
            cfg.ul2_kind = ref['kind']
            t = ref['table'] if ref['kind'] == nat.UL2_TABLE else ref['gains']
            t = t.to(device=dev, dtype=f32).contiguous()
            self._keep.append(t)
            cfg.ul2_ref = nat.ptr(t)
        sizes = nat.AffSizes()
        rc = self.lib.psp_aff_query(C.byref(cfg), C.byref(sizes))
        if rc != 0:
            raise PlanUnsupported('psp_aff_query: ' + nat.last_error())
        self.sizes = sizes
        self.slices, self.PP = int(sizes.slices), int(sizes.padded_params)
        self.Mpad = torch.zeros(N, DB, DB, dtype=f32, device=dev) if self.has_matrix else None
        self.cpad = torch.zeros(N, DB, dtype=f32, device=dev) if self.has_bias else None
        self.path = torch.empty(sizes.path_bytes // 4, dtype=f32, device=dev)
        self.fwd_partial = torch.empty(sizes.fwd_partial_bytes // 8, dtype=torch.float64, device=dev)
        self.partial = torch.zeros(N * self.slices, self.PP, dtype=f32, device=dev)
        self.D = torch.empty(self.K_local, dtype=f32, device=dev)
        self.Yn = torch.empty(self.K_local, dtype=f32, device=dev) if self.generic_loss else None
        self.w = torch.empty(self.K_local, dtype=f32, device=dev) if self.generic_loss else None
        self.w_bwd = torch.empty(self.K_local, dtype=f32, device=dev)
        if self.attached:
            self.XN_k = torch.empty(self.K_local, DB, dtype=f32, device=dev)
            self.mu = torch.zeros(self.K_local, dtype=f32, device=dev)
            self.nu = torch.zeros(self.K_local, dtype=f32, device=dev)
            self.wT = torch.zeros(self.K_local, dtype=f32, device=dev)
        self.sums = torch.zeros(2, dtype=torch.float64, device=dev)
        self.grad = torch.zeros(self.P, dtype=f32, device=dev)
        self.m = torch.zeros(self.P, dtype=f32, device=dev)
        self.v = torch.zeros(self.P, dtype=f32, device=dev)
        self.x0_vec = padded(s.X_0.detach().reshape(-1))
        self.step = 0
        for i, mod in enumerate(self.mods):                  # continue an optimiser that already carries state
            o = i * self.Pset
            self.step = max(self.step, sharding.adam_state_import(self._params_of(mod), self.m[o:o + self.Pset],
                                                                  self.v[o:o + self.Pset], mod.optim))
        self.learn_y0 = bool(s.learn_Y_0)
        if self.learn_y0:                                    # (its state is exported after training, not imported here)
            self.y0 = pc.Y0Adam(s.y_0, dev, import_state=False)
            self.y0_param = self.y0.param

    # ------------------------------------------------------------------------------------
    def _params_of(self, mod):
        if self.cls is Linear:
            return [mod.F]
        if self.cls is Affine:
            return [mod.A, mod.b]
        return [mod.c]

    def _flatten(self):
        """All parameter sets as views of ONE flat fp32 buffer [set 0 | set 1 | ...]: the modules (state_dict, Z_n,
        save_networks) keep working on live values, the fused Adam sees one vector."""
        per = [self._params_of(m) for m in self.mods]
        self.Pset = sum(p.numel() for p in per[0])
        self.P = self.Pset * len(per)
        self.flat = pc.rehome_params([p for params in per for p in params], self.dev)

    def _stage_maps(self):
        """(M, c) of every step from the live parameters, zero padded to the bucket."""
        d, N = self.s.d, self.s.N
        sets = self.flat.view(N, self.Pset)
        if self.has_matrix:
            F = sets[:, :d * d].reshape(N, d, d)
            self.Mpad[:, :d, :d].copy_(effective_map(self.G, F))
        if self.has_bias:
            self.cpad[:, :d].copy_(sets[:, self.Pset - d:])

    def _gradient(self, w):
        """psp_aff_rollout_bwd, the slices of every step summed in order, the chain rule back to the modules' parameters."""
        s, d, N, DB = self.s, self.s.d, self.s.N, self.d_pad
        nat.check(self.lib.psp_aff_rollout_bwd(C.byref(self.cfg), nat.ptr(self.path), nat.ptr(w), nat.ptr(self.partial),
                                               nat.stream_ptr(self.dev)), 'psp_aff_rollout_bwd')
        g = self.partial.view(N, self.slices, self.PP)
        g = g.sum(1) if self.slices > 1 else g[:, 0]
        out = self.grad.view(N, self.Pset)
        if self.has_matrix:
            dM = g[:, :DB * DB].view(N, DB, DB)[:, :d, :d]
            out[:, :d * d].copy_(chain_rule(self.G, dM.contiguous()).reshape(N, d * d))
        if self.has_bias:
            out[:, self.Pset - d:].copy_(g[:, DB * DB:DB * DB + d])
        return self.grad

    def iteration(self, l, loss_out, ul2_out=None):
        s, lib, cfg = self.s, self.lib, self.cfg
        st = nat.stream_ptr(self.dev)
        seed = int(s.seed) & 0xFFFFFFFFFFFFFFFF
        xi, x0 = pc.draw_noise(s, l, self.noise, self.k_offset, self.K_local, self.d_pad, self.dev)
        x0_t = x0 if x0 is not None else self.x0_vec
        self._stage_maps()
        nat.check(lib.psp_aff_rollout_fwd(C.byref(cfg), nat.ptr(self.Mpad), nat.ptr(self.cpad), nat.ptr(x0_t),
                                          self.d_pad if x0 is not None else 0, nat.ptr(self.y0_param) if self.learn_y0 else None,
                                          nat.ptr(xi), seed, l, nat.ptr(self.path), nat.ptr(self.D),
                                          nat.ptr(self.XN_k) if self.attached else None, nat.ptr(self.Yn),
                                          nat.ptr(self.fwd_partial), st), 'psp_aff_rollout_fwd')
        nat.check(lib.psp_aff_terminal_reduce(C.byref(cfg), nat.ptr(self.fwd_partial), nat.ptr(self.sums), st),
                  'psp_aff_terminal_reduce')
        sharding.allreduce_sum_(self.sums)                        # collective 1: 16 bytes
        if self.generic_loss:
            loss, w = sharding.generic_loss_weights(s.loss_method, s.adaptive_forward_process, self.D, self.Yn, s.K, self.w)
        else:
            loss = sharding.loss_from_sums(self.sums, s.K, s.loss_method)
            w = None if self.relent else sharding.loss_weights(self.D, self.sums, s.K, s.loss_method)
        loss_out[l] = loss.to(torch.float32)
        if self.ul2 is not None and ul2_out is not None:
            pc.log_mean_ul2(self.ul2, s.K, ul2_out, l)
        if self.attached:
            # the sweep leaves dL/dZ_n / sqrt(dt) in the image slot of the path store
            wT = pc.attached_weights(s.loss_method, self.relent, s.K, w, self.Yn, self.mu, self.nu, self.wT)
            nat.check(lib.psp_aff_adjoint_sweep(C.byref(cfg), nat.ptr(self.Mpad), nat.ptr(self.path), nat.ptr(self.XN_k),
                                                nat.ptr(self.mu), nat.ptr(self.nu) if self.relent else None, nat.ptr(wT), st),
                      'psp_aff_adjoint_sweep')
            self.w_bwd.fill_(1.0)
        elif self.relent:
            # detached relative entropy: dL/dZ_n = Z_n dt / K, and the image is Z_n  ->  weight sqrt(dt) / K
            self.w_bwd.fill_(float(cfg.base.sqrt_dt) / float(s.K))
        else:
            self.w_bwd.copy_(w)
        self._gradient(self.w_bwd)
        sharding.allreduce_sum_(self.grad)                        # collective 2
        self.step += 1
        pc.adam_step(lib, self.flat, self.grad, self.m, self.v, self.P, self.step,
                     pc.adam_hyper(self.mods, s.lr, PlanUnsupported), st)
        if self.learn_y0:
            self.y0.step(lib, self.sums, s.K, s.loss_method, self.w if self.generic_loss else None, self.step,
                         pc.adam_hyper(s.y_0, s.lr, PlanUnsupported), st)
        return loss

    def export_optimizer_state(self):
        """Called by Solver._train_native when training returns: every module's own Adam sees the moments this plan kept."""
        for i, mod in enumerate(self.mods):
            o = i * self.Pset
            sharding.adam_state_export(self._params_of(mod), self.m[o:o + self.Pset], self.v[o:o + self.Pset], self.step,
                                       getattr(mod, 'optim', None))
        if self.learn_y0:
            self.y0.export(self.step)
