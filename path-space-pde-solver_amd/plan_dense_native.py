"""Native execution plan for Solver.train with a DenseNet control (reference function_space.py:116-140):

  * time_approx='outer' -- the reference's constructor default (solver.py:88): N nets DenseNet(d -> d), one per
    time step, each with its own Adam (solver.py:142-162, 194-200);
  * time_approx='inner' with a DenseNet(d+1 -> d) swapped into z_n (notebook extension point).

Per iteration (reference solver.py:430-514):
    psp_dnet_rollout_fwd     hand-written HIP rollout (csrc/hjbd_kernels.h): D_k, the terminal sums and the two flat
                             batches the gradient needs, X_n and the xi image, each (N, K, d) row-major
    psp_dnet_terminal_reduce (sum D, sum D^2)                      [all-reduce 1]
    parameter gradient       detach_forward=True makes dL/dZ_n[k] = w_k sqrt(dt) image_n[k], so the gradient
                             of every net is that of a plain feed-forward batch: the stored relu activations and ~12 library
                             GEMMs (batched over the time steps; 'inner' shares one net across the batch), written
                             analytically below -- no autograd graph                    [all-reduce 2]
    psp_adam_step            one fused Adam over the concatenation of all parameter sets (identical to the reference's
                             per-net Adams: same lr, betas and step count)
The rollout is the sequential, launch-bound part of the reference (N steps x ~70 eager kernels) and is the hand-written
kernel; the gradient is GEMM-shaped and is left to rocBLAS.
Gradients THROUGH the state path (adaptive_forward_process=True with detach_forward=False: the reference's constructor
defaults, solver.py:23-24, 451-469) and the relative-entropy loss (:179-180, 484-486) run natively on the instances the
hand-written backward covers: the rollout leaves xi - sqrt(dt) Z (or Z) in the xi slot of the register images,
psp_dnet_adjoint_sweep (csrc/hjbd_kernels.h: hjbd_adj_kernel) walks the adjoint recursion backwards in time with the
Jacobian of the dense-concat net and overwrites the slot with dL/dZ_n / sqrt(dt), and the backward kernel runs with unit
weights -- the scheme of plan_native.py / psp_hjb_adjoint_sweep.
The u_L2 log (solver.py:471-472, 491-494; on by default whenever the problem has u_true) is accumulated per trajectory inside
the forward kernel from a description of u* built once per plan by ul2_reference (plan_common.py): a table of u*(t_n), the gains M_n of
a u* linear in x, or the double wells' grid tables with the reference's index arithmetic.
The gradient-variance diagnostic (Solver(compute_gradient_variance=m), solver.py:234-281, 496-497) runs on the same images for
time_approx='outer': DenseNativePlan.gradient_moments forms the first and second moments of the per-trajectory gradients from
psp_dnet_rollout_bwd / psp_dnet_rollout_bwd_sq launches and psp_gradvar_finish instead of 2 K N backward passes.
"""
import ctypes as C
import os

import torch

try:
    from . import native as nat
    from . import native_shapes as shapes
    from . import sharding
    from . import plan_common as pc
    from .function_space import DenseNet
    from .plan_common import PlanUnsupported, ul2_kind, ul2_reference, ul2_unsupported  # noqa: F401  (importable from here too)
    from .plan_native import _overridden
except ImportError:
    import native as nat
    import native_shapes as shapes
    import sharding
    import plan_common as pc
    from function_space import DenseNet
    from plan_common import PlanUnsupported, ul2_kind, ul2_reference, ul2_unsupported  # noqa: F401
    from plan_native import _overridden

_LOSSES = ('log-variance', 'moment', 'variance', 'cross_entropy', 'relative_entropy')


def _nets(solver):
    return list(solver.z_n) if solver.time_approx == 'outer' else [solver.z_n]


def _instance_for(d, H):
    cands = [(D, Hh) for (D, Hh) in nat.dnet_instances() if D >= d and Hh >= H]
    return min(cands, key=lambda t: (t[0] * t[0] + 3 * t[0] * t[1], t[1])) if cands else None


def dense_eligibility(solver):
    """None if the solver can run on this plan, else a human-readable reason."""
    if solver.device.type != 'cuda':
        return 'device is %s (the HIP rollout needs a GPU)' % solver.device
    if solver.approx_method != 'control':
        return "only approx_method='control' is native"
    if solver.loss_method not in _LOSSES:
        return 'loss_method %r is not native for a DenseNet control (%s are)' % (solver.loss_method, ', '.join(_LOSSES))
    if solver.loss_method == 'relative_entropy' and not solver.adaptive_forward_process:
        return 'relative_entropy with a non-adaptive forward process is not native for a DenseNet control'
    if solver.burgers_drift or solver.log_gradient or solver.metastability_logs is not None:
        return 'per-step / per-iteration diagnostics (gradient logs, metastability) are not native here'
    if solver.u_l2_error_flag:
        reason = ul2_unsupported(solver.problem, solver.N, solver.delta_t_np)
        if reason is not None:
            return reason
    nets = _nets(solver)
    outer = solver.time_approx == 'outer'
    if outer and len(nets) != solver.N:
        return "time_approx='outer' needs one net per time step"
    d_in = solver.d + (0 if outer else 1)
    dims0 = getattr(nets[0], 'nn_dims', None)
    for net in nets:
        dims = getattr(net, 'nn_dims', None)
        if not isinstance(net, DenseNet) or dims is None or len(dims) != 4 or dims[1] != dims[2] \
                or dims[0] != d_in or dims[3] != solver.d or dims != dims0:
            return 'control is not a DenseNet(%d -> %d) with two equal hidden widths' % (d_in, solver.d)
    spec_fn = getattr(solver.problem, 'native_spec', None)
    if spec_fn is None or spec_fn() is None:
        return getattr(solver.problem, 'native_plan_reason', None) or \
            'problem has no native_spec() (coefficients outside the native catalogue)'
    over = _overridden(solver.problem)
    if over is not None:
        return 'problem.%s is not the catalogue implementation native_spec() describes' % over
    if not nat.is_built():
        raise nat.NativeLibraryError('libpsp_hip.so is not built; run __graft_entry__.build()')
    if _instance_for(solver.d, dims0[1]) is None:
        return 'no compiled DenseNet-control instance covers d=%d, H=%d (csrc/dense_instances.def)' % (solver.d, dims0[1])
    if solver.compute_gradient_variance > 0:
        if nat.dnet_only_kind(spec_fn()) is not None:
            return ('compute_gradient_variance is not native for the per-coordinate / radial double-well kinds (the squared '
                    "backward's terminal term is not extended to them)")
        return gradient_variance_unsupported(solver, _instance_for(solver.d, dims0[1]))
    return None


def gradient_variance_unsupported(solver, instance, world=None):
    """None if DenseNativePlan.gradient_moments covers compute_gradient_variance > 0 for this solver on the (d, H) `instance`, else
    the precise reason (the composite plan then runs the reference's per-trajectory backward passes)."""
    if solver.time_approx != 'outer':
        return ("compute_gradient_variance indexes one net per time step (reference solver.py:248): it needs time_approx='outer'")
    if solver.loss_method not in ('moment', 'log-variance'):
        return ("compute_gradient_variance is defined for loss_method 'moment' and 'log-variance' only (the reference fails on %r)"
                % solver.loss_method)
    if solver.adaptive_forward_process and solver.detach_forward:
        return ('compute_gradient_variance with adaptive_forward_process=True and detach_forward=True differentiates g(X_N), which '
                'does not depend on the parameters there: the composite plan raises autograd\'s error as the reference does')
    if instance[0] > 128:
        return ('the native gradient moments run on the hand-written DenseNet-control backward, which covers d <= 128 '
                '(instance (%d, %d))' % tuple(instance))
    if os.environ.get('PSP_DENSE_BWD', 'kernel') == 'gemm':
        return 'the native gradient moments run on the hand-written DenseNet-control backward (PSP_DENSE_BWD=gemm is set)'
    if world is None:
        world = sharding.dist_info()[2]
    if world > 1:
        return 'the native gradient moments are single-rank (world size %d)' % world
    return None


def gradvar_combine(S, Q, S2, S1, Gg, K, loss_method, sum_c, sum_c2):
    """What psp_gradvar_finish computes from the slice-summed, gathered sums (torch, float64 in, fp32 out): (mean, var, rel,
    mean(rel)).  S = S[c], Q = Q[c], S2 = S[c^2], S1 = S[1] (log-variance), Gg (moment; None: 0).  var is clamped at 0 before the
    root, rel = sqrt(var) / mean in fp32 with NaN -> 0; inf and negative values stay."""
    K = float(K)
    if loss_method == 'log-variance':
        B = S1.double() / K
    else:
        B = Gg.double() if Gg is not None else torch.zeros_like(S, dtype=torch.float64)
    S2 = S2.double() if S2 is not None else torch.zeros_like(S, dtype=torch.float64)
    sf = 2.0 * (S.double() - B * sum_c)
    sf2 = 4.0 * (Q.double() - 2.0 * B * S2 + B * B * sum_c2)
    var = ((sf2 - sf * sf / K) / (K - 1.0)).clamp_min(0.0)
    mean32, var32 = (sf / K).to(torch.float32), var.to(torch.float32)
    rel = torch.sqrt(var32) / mean32
    rel[rel != rel] = 0
    return mean32, var32, rel, rel.double().mean().to(torch.float32)


class DenseNativePlan:
    def __init__(self, solver, noise='reference'):
        reason = dense_eligibility(solver)
        if reason is not None:
            raise PlanUnsupported(reason)
        s = solver
        self.s, self.noise, self.lib, self.dev = s, noise, nat.load(), s.device
        dev = self.dev
        self.dist, self.rank, self.world, lo, hi = pc.local_shard(s.K)
        self.K_local, self.k_offset = hi - lo, lo
        self.outer = s.time_approx == 'outer'
        self.nets = _nets(s)
        self.net = s.z_n                              # identity check in Solver._choose_plan
        self.B = len(self.nets)                       # parameter sets
        self.H = self.nets[0].nn_dims[1]
        self.di = s.d + (0 if self.outer else 1)
        self._flatten()
        self.d_pad, self.H_pad = _instance_for(s.d, self.H)
        self.pad = shapes.ParamPad(s.d, self.H, self.d_pad, self.H_pad, dev)      # used for the problem data / x0 / noise only
        spec = s.problem.native_spec()
        self._keep = []

        def dev_f32(t):
            if t is None:
                return None
            t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
            self._keep.append(t)
            return t

        cfg = nat.DnetConfig()
        b = cfg.base
        b.d, b.H = self.d_pad, self.H_pad
        self.generic_loss, self.relent, self.attached = pc.fill_hjb_base(b, s, spec, noise, self.K_local, self.k_offset)
        pad = self.pad
        b.drift = nat.ptr(dev_f32(pc.pad_coeff(pad, spec['drift'][1]))) if spec['drift'][1] is not None else None
        b.sigma = nat.ptr(dev_f32(pad.drift_or_sigma(spec['sigma'][1]))) if spec['sigma'][1] is not None else None
        b.runcost = nat.ptr(dev_f32(pad.vec(spec['runcost'][1]))) if spec['runcost'][1] is not None else None
        b.term = nat.ptr(dev_f32(pc.pad_coeff(pad, spec['term'][1])))
        cfg.d_real, cfg.H_real = s.d, self.H
        cfg.time_input, cfg.per_step = (0 if self.outer else 1), (1 if self.outer else 0)
        self.cfg = cfg
        # u_L2 log (solver.py:491-494): the description of u* goes to the device once; the kernel writes one float per trajectory
        self.ul2 = None
        if s.u_l2_error_flag:
            try:
                ref = ul2_reference(s.problem, s.N, s.delta_t_np, self.d_pad, s.K, self.k_offset)
            except ValueError as e:
                raise PlanUnsupported(str(e))
            self.ul2 = torch.zeros(self.K_local, dtype=torch.float32, device=dev)
            b.u_l2_out = nat.ptr(self.ul2)
            cfg.ul2_kind = ref['kind']
            if ref['kind'] == nat.UL2_TABLE:          # (16 floats of slack: include/psp.h u_ref)
                b.u_ref = nat.ptr(dev_f32(torch.cat([ref['table'].reshape(-1), torch.zeros(16)])))
            elif ref['kind'] == nat.UL2_LINEAR:
                cfg.ul2_tables = nat.ptr(dev_f32(ref['gains']))
            else:
                cfg.ul2_tables = nat.ptr(dev_f32(ref['tables']))
                for key in ('group', 'row'):
                    t = ref[key].to(device=dev).contiguous()
                    self._keep.append(t)
                    setattr(cfg, 'ul2_' + key, nat.ptr(t))
                cfg.ul2_ntables, cfg.ul2_nrows, cfg.ul2_ncols = ref['tables'].shape[0], ref['nrows'], ref['ncols']
                cfg.ul2_xb, cfg.ul2_dx, cfg.ul2_xhi = ref['xb'], ref['dx'], ref['xhi']
        sizes = nat.DnetSizes()
        # matrix products of the forward rollout: 'f16x3' = fp32-grade split products on the f16 matrix pipe (csrc/hjbd_kernels.h
        # hjbd_fwd_kernel<.., X3>; same parity bounds); 'auto' (the default) takes it where its images fit the LDS
        want = getattr(s, 'mlp_dtype', 'auto')
        if want == 'bf16':
            raise PlanUnsupported("mlp_dtype='bf16' exists for MySequential controls only")
        b.mlp_dtype = nat.MLP_F16X3 if want in ('auto', 'f16x3') else nat.MLP_FP32
        if self.lib.psp_dnet_query(C.byref(cfg), C.byref(sizes)) != 0:
            if want == 'f16x3':
                nat.check(self.lib.psp_dnet_query(C.byref(cfg), C.byref(sizes)), 'psp_dnet_query')
            b.mlp_dtype = nat.MLP_FP32
        self.matrix_mode = 'f16x3' if b.mlp_dtype == nat.MLP_F16X3 else 'fp32'
        # range guard of the split-product rollout (include/psp.h: psp_hjb_config.range_flag)
        self.range_flag = None
        if b.mlp_dtype == nat.MLP_F16X3 and getattr(s, 'range_guard', True):
            self.range_flag = torch.zeros(4, dtype=torch.int32, device=dev)
            b.range_flag = nat.ptr(self.range_flag)
        nat.check(self.lib.psp_dnet_query(C.byref(cfg), C.byref(sizes)), 'psp_dnet_query')
        assert sizes.n_params_per_set == self.Pset, (sizes.n_params_per_set, self.Pset)
        f32 = torch.float32
        self.tables = torch.empty(sizes.table_bytes // 4, dtype=f32, device=dev)
        if self.ul2 is not None:            # u_L2 log, kind 1: the gain tables go into the table scratch once
            nat.check(self.lib.psp_dnet_ul2_stage(C.byref(cfg), nat.ptr(self.tables), nat.stream_ptr(dev)), 'psp_dnet_ul2_stage')
        self.fwd_partial = torch.empty(sizes.fwd_partial_bytes // 8, dtype=torch.float64, device=dev)
        # gradient: the hand-written kernel (csrc/hjbd_kernels.h, hjbd_bwd_kernel) where the instance is covered, else the
        # library-GEMM formulation on row-major stores (PSP_DENSE_BWD=gemm forces the latter: cross-check / timing)
        self.kernel_bwd = bool(sizes.bwd_supported) and os.environ.get('PSP_DENSE_BWD', 'kernel') != 'gemm'
        self._gidx = None                                        # padded -> real gather index of a parameter set ('outer')
        if (self.attached or self.relent) and not self.kernel_bwd:
            raise PlanUnsupported('the adjoint sweep of a DenseNet control works on the register images of the hand-written '
                                  'backward, which does not cover the (%d, %d) instance' % (self.d_pad, self.H_pad))
        if self.attached or self.relent:
            self.w_bwd = torch.empty(self.K_local, dtype=f32, device=dev)
        if self.attached:
            self.XN_k = torch.empty(self.K_local, self.d_pad, dtype=f32, device=dev)
            self.mu = torch.zeros(self.K_local, dtype=f32, device=dev)
            self.nu = torch.zeros(self.K_local, dtype=f32, device=dev)
            self.wT = torch.zeros(self.K_local, dtype=f32, device=dev)
        if self.kernel_bwd:
            self.images = torch.empty(sizes.image_bytes // 4, dtype=f32, device=dev)
            self.partial = torch.zeros(s.N * sizes.slices, sizes.padded_params, dtype=f32, device=dev)
            self.wpad = torch.zeros(16 * ((self.K_local + 15) // 16), dtype=f32, device=dev)
            self.slices, self.PP = int(sizes.slices), int(sizes.padded_params)
            cfg.images_out = nat.ptr(self.images)
            self.PX = self.PXI = self.PR1 = self.PR2 = None
        else:
            self.PX = torch.empty(s.N, self.K_local, s.d, dtype=f32, device=dev)
            self.PXI = torch.empty(s.N, self.K_local, s.d, dtype=f32, device=dev)
            self.PR1 = torch.empty(s.N, self.K_local, self.H, dtype=f32, device=dev)   # relu(z1), relu(z2) from the rollout
            self.PR2 = torch.empty(s.N, self.K_local, self.H, dtype=f32, device=dev)
            cfg.r1_out, cfg.r2_out = nat.ptr(self.PR1), nat.ptr(self.PR2)
        self.D = torch.empty(self.K_local, dtype=f32, device=dev)
        self.Yn = torch.empty(self.K_local, dtype=f32, device=dev) if self.generic_loss else None
        self.w = torch.empty(self.K_local, dtype=f32, device=dev) if self.generic_loss else None
        self.sums = torch.zeros(2, dtype=torch.float64, device=dev)
        self.grad = torch.zeros(self.P, dtype=f32, device=dev)
        self.m = torch.zeros(self.P, dtype=f32, device=dev)
        self.v = torch.zeros(self.P, dtype=f32, device=dev)
        self.x0_vec = dev_f32(pad.vec(s.X_0.detach().to(dev)))
        self.tn = (torch.arange(s.N, device=dev, dtype=f32) * b.dt)        # fp32 n * dt, as the kernel forms it
        self.step = 0
        self.events = None
        # gradient-variance diagnostic (Solver(compute_gradient_variance=m)): moments of the latest logged iteration, and the
        # device log Solver._train_native reads back with the losses
        self.gv_mean = self.gv_var = self.gv_rel = None
        self.gv_log, self.gv_count = None, 0
        self._gv = None
        self.learn_y0 = bool(s.learn_Y_0)
        if self.learn_y0:
            self.y0 = pc.Y0Adam(s.y_0, dev, import_state=False)
            self.y0_param = self.y0.param
        # sample chunk of the gradient GEMMs: bounds their temporaries (~(2H + 2d) floats per sample)
        self.chunk = max(1, (1 << 21) // max(1, self.K_local)) if not self.outer else s.N

    # ------------------------------------------------------------------------------------
    def _flatten(self):
        """All parameter sets as views of ONE flat fp32 buffer [set 0 | set 1 | ...] (include/psp.h layout per set):
        state_dict / save_networks / Z_n keep working on live values, the fused Adam sees one vector."""
        per = [list(net.W) for net in self.nets]                     # registration order W1,b1,W2,b2,W3,b3
        self.Pset = sum(p.numel() for p in per[0])
        self.P = self.Pset * len(per)
        self.flat = pc.rehome_params([p for params in per for p in params], self.dev)
        di, H, d = self.di, self.H, self.nets[0].nn_dims[3]
        o, self.off = 0, {}
        for name, shape in (('W1', (di, H)), ('b1', (H,)), ('W2', (di + H, H)), ('b2', (H,)),
                            ('W3', (di + 2 * H, d)), ('b3', (d,))):
            n = 1
            for v in shape:
                n *= v
            self.off[name] = (o, n, shape)
            o += n

    def _set_view(self, buf, name):
        """(B, *shape) strided view of one tensor of every parameter set inside a flat (B * Pset) buffer."""
        o, n, shape = self.off[name]
        return buf.view(self.B, self.Pset)[:, o:o + n].reshape(self.B, *shape) if self.B == 1 else \
            buf.view(self.B, self.Pset)[:, o:o + n].unflatten(1, shape)

    # ------------------------------------------------------------------------------------
    def _gradient_kernel(self, w):
        """hjbd_bwd_kernel: per (step, slice) partial gradients in the instance's padded layout -> real shapes."""
        s, H, di, d, N = self.s, self.H, self.di, self.s.d, self.s.N
        D, Hp = self.d_pad, self.H_pad
        self.wpad[:self.K_local].copy_(w)
        nat.check(self.lib.psp_dnet_rollout_bwd(C.byref(self.cfg), nat.ptr(self.flat), nat.ptr(self.images), nat.ptr(self.wpad),
                                                nat.ptr(self.partial), nat.stream_ptr(self.dev)), 'psp_dnet_rollout_bwd')
        g = self.partial.view(N, self.slices, self.PP).sum(1)          # (N, PP): one padded gradient per time step
        if self.outer:
            # one parameter set per time step: the real rows / columns of every set are ONE gather through an index built once
            # (round 3 cut them out with a dozen strided slices and three torch.cat per iteration -- 35 device copies)
            if self._gidx is None:
                self._gidx = self._gather_index()
            torch.index_select(g, 1, self._gidx, out=self.grad.view(N, self.Pset))
            return self.grad
        o = 0
        W1 = g[:, o:o + D * Hp].view(N, D, Hp)[:, :d, :H]; o += D * Hp
        b1 = g[:, o:o + Hp][:, :H]; o += Hp
        W2 = g[:, o:o + (D + Hp) * Hp].view(N, D + Hp, Hp); o += (D + Hp) * Hp
        b2 = g[:, o:o + Hp][:, :H]; o += Hp
        W3 = g[:, o:o + (D + 2 * Hp) * D].view(N, D + 2 * Hp, D); o += (D + 2 * Hp) * D
        b3 = g[:, o:o + D][:, :d]
        W2r = torch.cat([W2[:, :d, :H], W2[:, D:D + H, :H]], 1)                                  # rows [x | h1]
        W3r = torch.cat([W3[:, :d, :d], W3[:, D:D + H, :d], W3[:, D + Hp:D + Hp + H, :d]], 1)    # rows [x | h1 | h2]
        grad = self.grad
        if self.outer:
            out = torch.cat([W1.reshape(N, -1), b1, W2r.reshape(N, -1), b2, W3r.reshape(N, -1), b3], 1)       # per-step sets
            grad.copy_(out.reshape(-1))
        else:                                                     # one net: sum over the steps; the time input is row 0 of
            t = self.tn.view(N, 1)                                # every layer's input block: its gradient is sum_n t_n db_n
            W1s = torch.cat([(t * b1).sum(0, keepdim=True), W1.sum(0)], 0)
            W2s = torch.cat([(t * b2).sum(0, keepdim=True), W2r.sum(0)], 0)
            W3s = torch.cat([(t * b3).sum(0, keepdim=True), W3r.sum(0)], 0)
            grad.copy_(torch.cat([W1s.reshape(-1), b1.sum(0), W2s.reshape(-1), b2.sum(0), W3s.reshape(-1), b3.sum(0)]))
        return grad

    def _gather_index(self):
        """Padded position (inside one per-step partial gradient of hjbd_bwd_kernel) of every real parameter of a set, in the
        DenseNet's registration order W1, b1, W2, b2, W3, b3 (weights (in, out); W2 rows [x | h1], W3 rows [x | h1 | h2])."""
        H, d, D, Hp = self.H, self.s.d, self.d_pad, self.H_pad
        ar = lambda n: torch.arange(n, device=self.dev)
        o, parts = 0, []
        parts.append((o + ar(d).view(-1, 1) * Hp + ar(H).view(1, -1)).reshape(-1)); o += D * Hp
        parts.append(o + ar(H)); o += Hp
        rows2 = torch.cat([ar(d), D + ar(H)])
        parts.append((o + rows2.view(-1, 1) * Hp + ar(H).view(1, -1)).reshape(-1)); o += (D + Hp) * Hp
        parts.append(o + ar(H)); o += Hp
        rows3 = torch.cat([ar(d), D + ar(H), D + Hp + ar(H)])
        parts.append((o + rows3.view(-1, 1) * D + ar(d).view(1, -1)).reshape(-1)); o += (D + 2 * Hp) * D
        parts.append(o + ar(d))
        idx = torch.cat(parts)
        assert idx.numel() == self.Pset, (idx.numel(), self.Pset)
        return idx

    # ---- gradient-variance diagnostic ---------------------------------------------------------------------------------------
    def begin_gradient_log(self, L):
        """Called by Solver._train_native before the first iteration: one device slot per logged iteration."""
        m = int(self.s.compute_gradient_variance)
        self.gv_count = 0
        self.gv_log = torch.zeros((L + m - 1) // m, dtype=torch.float32, device=self.dev) if m > 0 else None

    def _gv_buffers(self):
        if self._gv is None:
            reason = gradient_variance_unsupported(self.s, (self.d_pad, self.H_pad), self.world)
            if reason is None and not self.kernel_bwd:
                reason = 'the native gradient moments run on the hand-written DenseNet-control backward'
            if reason is not None:
                raise PlanUnsupported(reason)
            N, f32, dev = self.s.N, torch.float32, self.dev
            g = dict(part=[torch.zeros_like(self.partial) for _ in range(4)],
                     mean=torch.zeros(N, self.Pset, dtype=f32, device=dev), var=torch.zeros(N, self.Pset, dtype=f32, device=dev),
                     rel=torch.zeros(N, self.Pset, dtype=f32, device=dev), step_sums=torch.zeros(N, dtype=torch.float64, device=dev),
                     csums=torch.zeros(2, dtype=torch.float64, device=dev), scalar=torch.zeros(1, dtype=f32, device=dev),
                     ones=torch.ones(self.K_local, dtype=f32, device=dev))
            if self.attached:
                g.update(snap=torch.empty_like(self.images), Gg=torch.zeros(N, self.Pset, dtype=f32, device=dev),
                         one=torch.ones(self.K_local, dtype=f32, device=dev), zero=torch.zeros(self.K_local, dtype=f32, device=dev),
                         e0=torch.zeros(self.K_local, dtype=f32, device=dev))
                g['e0'][0] = 1.0                              # global trajectory 0 (single rank: k_offset = 0)
            if self._gidx is None:
                self._gidx = self._gather_index()
            self._gv = g
        return self._gv

    def _gv_launch(self, name, w, partial):
        self.wpad[:self.K_local].copy_(w)
        nat.check(getattr(self.lib, name)(C.byref(self.cfg), nat.ptr(self.flat), nat.ptr(self.images), nat.ptr(self.wpad),
                                          nat.ptr(partial), nat.stream_ptr(self.dev)), name)

    def _gv_sweep(self, mu, wT):
        nat.check(self.lib.psp_dnet_adjoint_sweep(C.byref(self.cfg), nat.ptr(self.flat), nat.ptr(self.images), nat.ptr(self.XN_k),
                                                  nat.ptr(mu), None, nat.ptr(wT), nat.ptr(self.tables), nat.stream_ptr(self.dev)),
                  'psp_dnet_adjoint_sweep')

    def gradient_moments(self, out=None):
        """The reference's get_gradient_variances (solver.py:234-281) from sums over the trajectories instead of 2 K N backward
        passes.  Call after the forward of an iteration (self.D, self.sums, the images).  With G_k = dY_N[k] / dtheta_n (rank one per
        layer), S[c] = sum_k c_k G_k (hjbd_bwd_kernel, w = c) and Q[c] = sum_k c_k^2 G_k o G_k (hjbd_bwd_kernel<.., SQ>, w = c):
            moment,       c = r:           sum f = 2 (S[r] - Gg sum r)        sum f^2 = 4 (Q[r] - 2 Gg S[r^2] + Gg^2 sum r^2)
            log-variance, s = r - mean r:  sum f = 2 (S[s] - Gbar sum s)      sum f^2 = 4 (Q[s] - 2 Gbar S[s^2] + Gbar^2 sum s^2),  Gbar = S[1] / K
        (Gg cancels for log-variance).  Images: non-adaptive -- the forward's image is dY_k / dZ_n / sqrt(dt) already; attached -- the
        images are snapshotted, one adjoint sweep with mu = 1 and an explicit wT = 0 (NULL would mean nu - mu, i.e. Y - g) turns the xi
        slot into the G images, a second sweep from the restored snapshot with mu = 0, wT = e_0 gives Gg (the reference differentiates
        g at trajectory 0 for every k), and the snapshot is restored before the training sweep, whose gradient is therefore
        bit-identical to a run without the diagnostic.  psp_gradvar_finish reduces the slices and combines in double; results in
        self.gv_mean / gv_var / gv_rel (N, Pset), the scalar mean(rel) into `out` (a 1-element device tensor).  No host sync."""
        s, g = self.s, self._gv_buffers()
        K = float(s.K)
        moment = s.loss_method == 'moment'
        r = self.D
        c = r if moment else r - (self.sums[0] / K).to(r.dtype)
        cd = c.double()
        g['csums'][0], g['csums'][1] = cd.sum(), (cd * cd).sum()
        pS, pQ, pS2, pS1 = g['part']
        Gg = None
        if self.attached:
            g['snap'].copy_(self.images)
            if moment:
                self._gv_sweep(g['zero'], g['e0'])
                self._gv_launch('psp_dnet_rollout_bwd', g['ones'], pS)
                torch.index_select(pS.view(s.N, self.slices, self.PP).sum(1), 1, self._gidx, out=g['Gg'])
                Gg = g['Gg']
                self.images.copy_(g['snap'])
            self._gv_sweep(g['one'], g['zero'])
        self._gv_launch('psp_dnet_rollout_bwd', c, pS)
        self._gv_launch('psp_dnet_rollout_bwd_sq', c, pQ)
        need_S2 = (not moment) or Gg is not None
        if need_S2:
            self._gv_launch('psp_dnet_rollout_bwd', c * c, pS2)
        if not moment:
            self._gv_launch('psp_dnet_rollout_bwd', g['ones'], pS1)
        if self.attached:
            self.images.copy_(g['snap'])
        nat.check(self.lib.psp_gradvar_finish(nat.ptr(pS), nat.ptr(pQ), nat.ptr(pS2) if need_S2 else None,
                                              nat.ptr(pS1) if not moment else None, nat.ptr(Gg), nat.ptr(self._gidx), s.N, self.slices,
                                              self.PP, self.Pset, s.K, nat.LOSS_MOMENT if moment else nat.LOSS_LOG_VARIANCE,
                                              nat.ptr(g['csums']), nat.ptr(g['mean']), nat.ptr(g['var']), nat.ptr(g['rel']),
                                              nat.ptr(g['step_sums']), nat.ptr(g['scalar']), nat.stream_ptr(self.dev)),
                  'psp_gradvar_finish')
        self.gv_mean, self.gv_var, self.gv_rel = g['mean'], g['var'], g['rel']
        if out is not None:
            out.copy_(g['scalar'])
        return g['scalar']

    def _gradient(self, w):
        if self.kernel_bwd:
            return self._gradient_kernel(w)
        return self._gradient_gemm(w)

    def _gradient_gemm(self, w):
        """grad of sum_{n,k} G_n[k] . Z_n(X_n[k]) over all parameter sets, G = w_k sqrt(dt) image (row-major stores)."""
        s, H, di, d = self.s, self.H, self.di, self.s.d
        N, K = s.N, self.K_local
        grad = self.grad
        grad.zero_()
        W2, W3 = self._set_view(self.flat, 'W2'), self._set_view(self.flat, 'W3')
        gW1, gb1, gW2, gb2, gW3, gb3 = (self._set_view(grad, k) for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'))
        # row blocks of the dense-concat weights: [input | h1 | h2]; every product below works on one block, so the
        # concatenated activations [u, h1, h2] are never materialised (the torch.cat copies were a quarter of this function)
        W2h = W2[:, di:, :]
        W3h1T, W3h2T = W3[:, di:di + H, :].transpose(1, 2), W3[:, di + H:, :].transpose(1, 2)     # (B, d, H)
        W2hT = W2h.transpose(1, 2)
        scale = (w * float(self.cfg.base.sqrt_dt)).view(1, K, 1)
        for n0 in range(0, N, self.chunk):
            n1 = min(N, n0 + self.chunk)
            X = self.PX[n0:n1]
            G = self.PXI[n0:n1] * scale                           # (n, K, d)
            # batch = time steps in both modes: 'outer' pairs step n with its own net, 'inner' broadcasts the one net over
            # the steps and sums the per-step weight gradients (rocBLAS handles n reductions over K rows far better than
            # one tall-skinny reduction over n K rows)
            if self.outer:
                U, sl = X, slice(n0, n1)
            else:
                U, sl = torch.cat([self.tn[n0:n1].view(-1, 1, 1).expand(n1 - n0, K, 1), X], 2), slice(0, 1)
            red = (lambda t: t) if self.outer else (lambda t: t.sum(0, keepdim=True))
            UT = U.transpose(1, 2)
            r1, r2 = self.PR1[n0:n1], self.PR2[n0:n1]             # stored by the rollout kernel (no recomputed forward)
            h1, h2 = r1 * r1, r2 * r2
            gW3[sl][:, :di] += red(torch.matmul(UT, G))
            gW3[sl][:, di:di + H] += red(torch.matmul(h1.transpose(1, 2), G))
            gW3[sl][:, di + H:] += red(torch.matmul(h2.transpose(1, 2), G))
            gb3[sl] += red(G.sum(1))
            dz2 = torch.matmul(G, W3h2T[sl]) * (2.0 * r2)
            gW2[sl][:, :di] += red(torch.matmul(UT, dz2))
            gW2[sl][:, di:] += red(torch.matmul(h1.transpose(1, 2), dz2))
            gb2[sl] += red(dz2.sum(1))
            dz1 = (torch.matmul(G, W3h1T[sl]) + torch.matmul(dz2, W2hT[sl])) * (2.0 * r1)
            gW1[sl] += red(torch.matmul(UT, dz1))
            gb1[sl] += red(dz1.sum(1))
        return grad

    def iteration(self, l, loss_out, ul2_out=None):
        s, lib, cfg = self.s, self.lib, self.cfg
        st = nat.stream_ptr(self.dev)
        seed = int(s.seed) & 0xFFFFFFFFFFFFFFFF
        xi, x0 = pc.draw_noise(s, l, self.noise, self.k_offset, self.K_local, self.d_pad, self.dev)
        x0_t = x0 if x0 is not None else self.x0_vec
        ev = None
        if self.events is not None:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
        nat.check(lib.psp_dnet_rollout_fwd(C.byref(cfg), nat.ptr(self.flat), nat.ptr(x0_t), self.d_pad if x0 is not None else 0,
                                           nat.ptr(self.y0_param) if self.learn_y0 else None, nat.ptr(xi), seed, l, None,
                                           nat.ptr(self.PX), nat.ptr(self.PXI), nat.ptr(self.D), None,
                                           nat.ptr(self.XN_k) if self.attached else None,
                                           nat.ptr(self.Yn), nat.ptr(self.fwd_partial), nat.ptr(self.tables), st),
                  'psp_dnet_rollout_fwd')
        if ev is not None:
            ev[1].record()
        nat.check(lib.psp_dnet_terminal_reduce(C.byref(cfg), nat.ptr(self.fwd_partial), nat.ptr(self.sums), st),
                  'psp_dnet_terminal_reduce')
        sharding.allreduce_sum_(self.sums)                        # collective 1: 16 bytes
        if self.generic_loss:
            loss, w = sharding.generic_loss_weights(s.loss_method, s.adaptive_forward_process, self.D, self.Yn, s.K, self.w)
        else:
            loss = sharding.loss_from_sums(self.sums, s.K, s.loss_method)
            w = None if self.relent else sharding.loss_weights(self.D, self.sums, s.K, s.loss_method)
        loss_out[l] = loss.to(torch.float32)
        if self.ul2 is not None and ul2_out is not None:
            pc.log_mean_ul2(self.ul2, s.K, ul2_out, l)
        if ev is not None:
            ev[2].record()
        m_gv = int(s.compute_gradient_variance)
        if m_gv > 0 and l % m_gv == 0:                            # solver.py:496-497: before the gradient step
            if self.gv_log is None or self.gv_count >= self.gv_log.numel():
                self.begin_gradient_log(max(int(s.L), l + 1))
            self.gradient_moments(out=self.gv_log[self.gv_count:self.gv_count + 1])
            self.gv_count += 1
        if self.attached:
            # the sweep leaves dL/dZ_n / sqrt(dt) in the xi slot of the images
            wT = pc.attached_weights(s.loss_method, self.relent, s.K, w, self.Yn, self.mu, self.nu, self.wT)
            nat.check(lib.psp_dnet_adjoint_sweep(C.byref(cfg), nat.ptr(self.flat), nat.ptr(self.images), nat.ptr(self.XN_k),
                                                 nat.ptr(self.mu), nat.ptr(self.nu) if self.relent else None, nat.ptr(wT),
                                                 nat.ptr(self.tables), st), 'psp_dnet_adjoint_sweep')
            self.w_bwd.fill_(1.0)
            w = self.w_bwd
        elif self.relent:
            # detached relative entropy: dL/dZ_n = Z_n dt / K, and the xi slot holds Z_n  ->  weight sqrt(dt) / K
            self.w_bwd.fill_(float(cfg.base.sqrt_dt) / float(s.K))
            w = self.w_bwd
        self._gradient(w)
        if ev is not None:
            ev[3].record()
            self.events.append(ev)
        sharding.allreduce_sum_(self.grad)                        # collective 2
        self.step += 1
        pc.adam_step(lib, self.flat, self.grad, self.m, self.v, self.P, self.step,
                     pc.adam_hyper(self.nets, s.lr, PlanUnsupported), st)
        if self.learn_y0:
            self.y0.step(lib, self.sums, s.K, s.loss_method, self.w if self.generic_loss else None, self.step,
                         pc.adam_hyper(s.y_0, s.lr, PlanUnsupported), st)
        return loss

    def range_fallbacks(self):
        return pc.range_fallbacks(self.range_flag)
