"""Native (HIP) execution plan for Solver.train on MI355X.

Replaces the body of the reference's training iteration (solver.py:430-514) by five
asynchronous launches through the C ABI of libpsp_hip.so (include/psp.h):

    psp_hjb_rollout_fwd  ->  psp_hjb_terminal_reduce  -> [all-reduce (sum D, sum D^2)]
    psp_hjb_rollout_bwd  -> [all-reduce flat gradient] -> psp_adam_step

torch supplies device memory, the stream and (for world_size > 1) the RCCL all-reduces;
no arithmetic of the hot path runs in torch.  Trajectories are sharded across ranks by
contiguous blocks; noise is indexed by GLOBAL trajectory id so the result does not depend
on the number of ranks.

Path stores larger than a budget (configs[4]: d=500, K=1048576, N=200 needs 946 GB) are bounded by K-CHUNKING: the
rank's trajectories are processed in chunks that share one path-store buffer.  Because the log-variance weights
w_k = (2/K)(D_k - mean D) need the GLOBAL mean, a chunked iteration is either
  'two_gradient' (log-variance / moment, detached): per chunk forward + store, backward with weights D_k - c (c = mean of
      the first chunk, any constant is exact) AND backward with unit weights; afterwards
      grad = (2/K) [G1 - (mean D - c) G0].  No forward recompute; costs one extra backward launch per chunk.
  'recompute' (every other native mode): pass 1 = forward per chunk WITHOUT the store -> global sums / weights,
      pass 2 = forward with the store (same Philox counters: bit-identical), [adjoint sweep,] backward.
The reference keeps the whole autograd graph instead (SURVEY.md 7 "Activation memory").
"""
import ctypes as C
import os
from collections import namedtuple

import numpy as np
import torch

try:
    from . import native as nat
    from . import native_shapes as shapes
    from . import plan_common as pc
    from . import sharding
    from .plan_common import PlanUnsupported  # noqa: F401  (re-exported: the name callers import from here)
except ImportError:
    import native as nat
    import native_shapes as shapes
    import plan_common as pc
    import sharding
    from plan_common import PlanUnsupported  # noqa: F401


def _overridden(problem):
    try:
        from .problems import coefficients_overridden
    except ImportError:
        from problems import coefficients_overridden
    return coefficients_overridden(problem)


# ---- state basis -------------------------------------------------------------------------------------
# With a constant invertible sigma = B the rollout may carry X~ = B^-1 X:  X~_{n+1} = X~_n + dt (B^-1 A B) X~_n + v_n  -- ONE
# d x d product per step instead of two (A X and B v).  The kernels are handed the equivalent problem (drift M = B^-1 A B,
# sigma = I, terminal vector B^T alpha, x0 = B^-1 x0); Z, Y, D, h1, h2 and the noise are unchanged; the net sees
# W1x X = (W1x B) X~ (psp_hjb_basis_params before the forward) and the backward's dW~1x goes back through
# dW1x = dW~1x B^T (psp_hjb_basis_grad before the all-reduce and Adam).
# plan.cfg, plan.path and plan.grad_k are then in the sigma basis (the store holds X~, the backward leaves dW~1x): code that
# drives psp_hjb_rollout_bwd on a plan's buffers itself must read plan.state_basis; plan.grad and the parameters stay in x.
STATE_BASIS_MAX_COND = 4.0       # fp32 rollouts of the two forms are indistinguishable against fp64 up to cond_2(B) = 4.2 and
                                 # 4x apart at 41
STATE_BASIS_MAX_D = 112          # the narrow kernel family
STATE_BASIS_MAX_X0_SPREAD = 100.0


def sigma_basis_problem(A, B, alpha, x0):
    """M = B^-1 A B, alpha' = B^T alpha, x~0 = B^-1 x0 in fp64 (numpy arrays in, numpy float64 out)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    alpha, x0 = np.asarray(alpha, dtype=np.float64).reshape(-1), np.asarray(x0, dtype=np.float64).reshape(-1)
    return np.linalg.solve(B, A @ B), B.T @ alpha, np.linalg.solve(B, x0)


def state_basis_decision(solver, spec=None):
    """('sigma' | 'x', reason) for the solver's HJB plan -- host arithmetic only, no GPU.  Solver(state_basis='x' | 'sigma' |
    'auto'); PSP_STATE_BASIS=0 in the environment forces 'x' (same-build A/B runs; read once, when the plan is built).
    'sigma' on an ineligible configuration raises ValueError (whatever the backend)."""
    want = getattr(solver, 'state_basis', 'auto')
    if want not in ('auto', 'x', 'sigma'):
        raise ValueError("state_basis must be 'auto', 'x' or 'sigma'")
    if os.environ.get('PSP_STATE_BASIS', '') == '0':
        return 'x', 'PSP_STATE_BASIS=0'
    if want == 'x':
        return 'x', "state_basis='x' requested"
    why = _sigma_basis_obstacle(solver, spec)
    if why is None and want == 'auto':
        why = _sigma_basis_auto_obstacle(solver)
    if why is not None:
        if want == 'sigma':
            # (a ValueError, not PlanUnsupported: backend='auto' must not answer an explicit request with the composite plan)
            raise ValueError("state_basis='sigma' is not available: " + why)
        return 'x', why
    return 'sigma', 'dense drift and sigma, linear terminal cost, fixed X_0, cond_2(B) <= %g' % STATE_BASIS_MAX_COND


def _sigma_basis_auto_obstacle(solver):
    """'auto' only.  An fp32 X~ resolves X = B X~ to eps ||B|| max |X~| in EVERY component, so a start vector whose largest
    component is orders of magnitude above the others costs the small ones their digits (measured: one component at 7e4 next to
    O(1) ones, d = 100: gradient error 1.8e-4 of max |grad| against 9e-8 in the x basis); cond_2(B) does not see that."""
    x0 = np.abs(solver.X_0.detach().double().cpu().numpy().reshape(-1))
    if x0.size and float(x0.max()) > STATE_BASIS_MAX_X0_SPREAD * max(1.0, float(np.median(x0))):
        return 'max |X_0| = %.3g is more than %g x the typical component' % (float(x0.max()), STATE_BASIS_MAX_X0_SPREAD)
    return None


def _sigma_basis_obstacle(solver, spec=None):
    if spec is None:
        fn = getattr(solver.problem, 'native_spec', None)
        spec = fn() if fn is not None else None
    if spec is None:
        return 'problem has no native_spec()'
    if getattr(solver, 'approx_method', 'control') != 'control' or getattr(solver, 'time_approx', 'inner') != 'inner':
        return "only the time-input control net (time_approx='inner') rolls out in the sigma basis"
    if spec['drift'][0] != nat.DRIFT_DENSE or spec['sigma'][0] != nat.SIGMA_DENSE:
        return 'drift and sigma are not both dense matrices'
    if solver.adaptive_forward_process and not solver.detach_forward:
        return 'attached forward process: the adjoint sweep differentiates through the state path in the x basis'
    if spec['runcost'][0] != nat.RUNCOST_ZERO:
        return 'the running cost reads X in the x basis'
    if spec['term'][0] != nat.TERM_LINEAR:
        return 'the terminal cost is not linear in X'
    if solver.random_X_0:
        return 'random_X_0 draws a per-trajectory X_0 in the x basis'
    if solver.u_l2_error_flag and getattr(solver.problem, 'u_true_x_independent', False) is not True:
        return 'the u_L2 log of an x-dependent reference control reads X from the path store'
    if getattr(solver, 'mlp_dtype', 'auto') == 'bf16':
        return "mlp_dtype='bf16' keeps its own tolerance in the x basis"
    if solver.d > STATE_BASIS_MAX_D or os.environ.get('PSP_FORCE_WIDE', '') == '1':
        return 'the wide kernel family (d > %d) is built around the two products' % STATE_BASIS_MAX_D
    B = spec['sigma'][1].detach().double().cpu().numpy()
    sv = np.linalg.svd(B, compute_uv=False)
    if not (sv[-1] > 0.0) or not np.isfinite(sv).all():
        return 'sigma is singular'
    cond = float(sv[0] / sv[-1])
    if cond > STATE_BASIS_MAX_COND:
        return 'cond_2(sigma) = %.3g exceeds %g' % (cond, STATE_BASIS_MAX_COND)
    return None


def native_eligibility(solver):
    """Returns None if the solver can run natively, else a human-readable reason."""
    if solver.device.type != 'cuda':
        return 'device is %s (the HIP rollout needs a GPU)' % solver.device
    if solver.approx_method != 'control' or solver.time_approx != 'inner':
        return "only approx_method='control' with time_approx='inner' is native"
    if solver.loss_method not in ('log-variance', 'moment', 'variance', 'cross_entropy', 'relative_entropy'):
        return ("loss_method %r is not native (log-variance, moment, variance, cross_entropy, relative_entropy)"
                % solver.loss_method)
    if solver.burgers_drift:
        return 'burgers_drift is not native'
    if solver.u_l2_error_flag and getattr(solver.problem, 'u_true_x_independent', False) is not True \
            and getattr(solver.problem, 'u_true_linear_in_x', False) is not True and pc.u_tables(solver.problem) is None:
        return ('u_l2_error_flag=True evaluates problem.u_true(X_n, t_n) on the host every step '
                '(reference solver.py:491-494); a u_true that does not depend on x (LLGC) is logged inside the kernels, one '
                'that is linear in x (LQGC) or tabulated per coordinate (the double wells) from the path store -- pass '
                'u_l2_error_flag=False for the native plan otherwise')
    if solver.compute_gradient_variance > 0 or solver.log_gradient:
        return 'per-iteration diagnostics (gradient variance / gradient log) are not native'
    if solver.metastability_logs is not None:
        return 'metastability_logs needs X_N on the host every iteration'
    net = solver.z_n
    shape = getattr(net, 'native_shape', lambda: None)()
    if shape is None or shape[0] != solver.d + 1 or shape[2] != solver.d:
        return 'control net is not a two-hidden-layer tanh MLP (MySequential)'
    spec_fn = getattr(solver.problem, 'native_spec', None)
    spec = spec_fn() if spec_fn is not None else None
    if spec is None:
        return getattr(solver.problem, 'native_plan_reason', None) or \
            'problem has no native_spec() (coefficients outside the native catalogue)'
    if nat.dnet_only_kind(spec) is not None:
        return nat.dnet_only_kind(spec)
    over = _overridden(solver.problem)
    if over is not None:
        return 'problem.%s is not the catalogue implementation native_spec() describes' % over
    if not nat.is_built():
        raise nat.NativeLibraryError('libpsp_hip.so is not built; run __graft_entry__.build()')
    probe = nat.HjbConfig()
    probe.K_local, probe.N, probe.K_global = 16, 1, 16
    probe.drift_kind, probe.sigma_kind = spec['drift'][0], spec['sigma'][0]
    probe.runcost_kind, probe.term_kind = spec['runcost'][0], spec['term'][0]
    probe.adaptive = 1 if solver.adaptive_forward_process else 0
    probe.store_path = 1
    chosen, why = shapes.choose(probe, solver.d, shape[1])
    if chosen is None:
        return why
    return None


def chunk_scratch_sizes(cfg, chunk_Ks, query_rc=nat.query_rc):
    """psp_hjb_sizes that serve EVERY chunk size in `chunk_Ks`: the field-wise maximum of the per-size queries."""
    sizes = None
    for k in sorted(set(int(k) for k in chunk_Ks)):
        probe = nat.HjbConfig.from_buffer_copy(cfg)
        probe.K_local = k
        rc, q, _ = query_rc(probe)
        nat.check(rc, 'psp_hjb_query')
        if sizes is None:
            sizes = q
        else:
            for f in ('path_bytes', 'fwd_partial_bytes', 'grad_partial_bytes', 'fwd_workgroups', 'bwd_workgroups'):
                setattr(sizes, f, max(getattr(sizes, f), getattr(q, f)))
    return sizes


# ---- decide(): every selection rule of the plan is a line of it (or of state_basis_decision / _decide_chunks, which it calls) ----
# Host arithmetic and size queries only.  tests/golden/hjb_plan_decisions.json pins its answers; a deliberate change re-records it.
HjbDecision = namedtuple('HjbDecision', 'state_basis state_basis_reason mlp_dtype matrix_mode range_guard store_path regen_xi '
                                        'sigma_kind d_pad H_pad family sizes alloc_sizes ul2_mode n_chunks chunk_K chunk_mode')
QUERY_PTR = 0x1000                        # a non-null pointer for the size queries: no query dereferences one
DEFAULT_PATH_BUDGET = 180 * 2 ** 30       # five eighths of the 288 GB of HBM3E when the device cannot be asked


def launch_bound(K, cus):
    """At most two 16-trajectory tiles per CU: the iteration over K trajectories is launch-bound (the regime of the small-K
    forward kernels and of the hipGraph replay), not store- or matrix-pipe-bound.  cus = None (no device): no size rule applies."""
    return cus is not None and (K + 15) // 16 <= 2 * cus


def decide(solver, spec, base_cfg, K_local, world, cus, budget, query_rc=nat.query_rc):
    """The launch configuration of an HjbNativePlan as an HjbDecision.  base_cfg: the config after plan_common.fill_hjb_base
    (copied, not written); K_local: this rank's trajectories of the solver's K over `world` ranks; cus / budget: the device's CU
    count and default path-store budget in bytes, None without a device (no size rule; DEFAULT_PATH_BUDGET).  Allocates
    nothing on the device.  Raises PlanUnsupported / ValueError for what the plan refuses."""
    cfg = nat.HjbConfig.from_buffer_copy(base_cfg)
    H = solver.z_n.native_shape()[1]
    # the state basis of every launch of the plan (comment above state_basis_decision): under 'sigma' the kernels get identity sigma
    basis, basis_why = state_basis_decision(solver, spec)
    if basis == 'sigma' and getattr(solver, 'state_basis', 'auto') == 'auto' and launch_bound(-(-solver.K // world), cus):
        # (from the even share K / world, not this rank's K_local: every rank of a job picks the same basis)
        # 'auto' follows the size rule of the split-product mode and of store_path 4 below: a launch-bound iteration pays for the
        # two transform launches (and for the fused backward + Adam launch of the hipGraph replay, which the gradient transform
        # splits).  Conservative: at d = 100, K = 8192 an explicit 'sigma' still measures 4 % faster.
        basis, basis_why = 'x', 'launch-bound size (at most two 16-trajectory tiles per CU)'
    if basis == 'sigma':
        cfg.sigma_kind = nat.SIGMA_IDENTITY
    # matrix products: 'fp32' = v_mfma_f32_16x16x4_f32; 'f16x3' = fp32-grade split products on the f16 pipe (three
    # v_mfma_f32_16x16x32_f16 per fp32 product, csrc/hjb_kernels.h gemm_Tx, csrc/hjbx_kernels.h -- same parity bounds);
    # 'auto' (the default) = 'f16x3' where those kernels exist, fit the LDS and the tile-per-wave forward would run anyway
    # (not launch-bound: the small-K forward kernels are fp32 only), else 'fp32'
    want = getattr(solver, 'mlp_dtype', 'auto')
    cfg.mlp_dtype = {'auto': nat.MLP_FP32, 'fp32': nat.MLP_FP32, 'bf16': nat.MLP_BF16_FWD, 'f16x3': nat.MLP_F16X3}[want]
    # kernel instance: the exact (d, H) if compiled, else the cheapest larger one (zero padding, native_shapes.py)
    chosen, why = shapes.choose(cfg, solver.d, H, query_rc)
    if chosen is None:
        raise PlanUnsupported(why)
    if basis == 'sigma' and chosen[2] != 1:          # (only the narrow family has the one-product forward)
        basis, basis_why = 'x', 'the configuration runs on the wide kernel family'
        cfg.sigma_kind = spec['sigma'][0]
        chosen, why = shapes.choose(cfg, solver.d, H, query_rc)
        if chosen is None:
            raise PlanUnsupported(why)
    d_pad, H_pad, family, sizes = chosen
    # (the wide family has no small-K kernels: its split-product forward serves every K)
    if want == 'auto' and cus is not None and (family == 2 or not launch_bound(K_local, cus)):
        cfg.mlp_dtype = nat.MLP_F16X3
        rc, sizes_x3, _ = query_rc(cfg)
        if rc == 0:
            sizes = sizes_x3
        else:
            cfg.mlp_dtype = nat.MLP_FP32
    # range guard of the split-product mode (include/psp.h: psp_hjb_config.range_flag): the reference is fp32 end to end
    # (solver.py:39-40); an f16x3 operand beyond 65504 turns D_k into NaN, the forward call raises a device flag and the
    # fp32-MFMA kernels -- enqueued behind the split ones, predicated on that flag -- redo the iteration.  No host sync.
    guard = False
    if cfg.mlp_dtype == nat.MLP_F16X3 and getattr(solver, 'range_guard', True):
        cfg.range_flag = QUERY_PTR                   # (the plan puts its flag tensor here; every later query sees a guarded config)
        guard = query_rc(cfg)[0] == 0
        if not guard:                                # (the fp32-MFMA tables of this instance do not fit the LDS: unguarded)
            cfg.range_flag = None
    # store_path 4 (include/psp.h): the forward keeps X_n, h1, h2 only and the backward producers regenerate xi from the
    # Philox counters -- where the stored image would be xi itself (detached adaptive process, on-device noise), in the
    # narrow kernel family, on the eager iteration (psp_hjb_rollout_bwd_step of the hipGraph replay takes no seed; that
    # regime is launch-bound, not store-bound).  Solver(path_noise='store') keeps xi.
    regen = False
    if (getattr(solver, 'path_noise', 'auto') != 'store' and cfg.store_path == 1 and cfg.noise_mode == nat.NOISE_PHILOX
            and cfg.adaptive and family == 1 and getattr(solver, 'use_graph', 'auto') is not True
            and cus is not None and not launch_bound(K_local, cus)):
        cfg.store_path = 4
        regen = query_rc(cfg)[0] == 0
        if not regen:
            cfg.store_path = 1
    simple = base_cfg.store_path == 1 and base_cfg.loss_kind != nat.LOSS_WEIGHTS      # log-variance / moment, detached
    n_chunks, chunk_K, chunk_mode, alloc = _decide_chunks(solver, cfg, sizes, K_local, simple, cus, budget, query_rc)
    # the u_L2 log: tabulated per coordinate on a grid (the double wells) or linear in x (LQGC), both formed from the path store
    # (_ul2_rows_from_path), or x-independent (LLGC), accumulated inside the kernels from a table u*(t_n)
    ul2_mode, sizes = None, alloc
    if solver.u_l2_error_flag:
        x_free = getattr(solver.problem, 'u_true_x_independent', False) is True
        ul2_mode = 'ul2_tab' if pc.u_tables(solver.problem) is not None else ('ul2' if x_free else 'ul2_gain')
        if ul2_mode == 'ul2' and n_chunks <= 1:
            # the sizes above were queried without u_ref: with it the library launches no cooperative forward (wide family,
            # f16x3, Philox noise), so fwd_workgroups / fwd_coop_tiles described a launch that never happens.  The buffers
            # sized from that query (alloc_sizes) stay: the tile-per-wave forward needs no more workgroups than the cooperative one
            cfg.u_ref = cfg.u_l2_out = QUERY_PTR
            rc, sizes, _ = query_rc(cfg)
            nat.check(rc, 'psp_hjb_query')
            assert sizes.fwd_partial_bytes <= alloc.fwd_partial_bytes and sizes.path_bytes == alloc.path_bytes
    matrix_mode = {nat.MLP_FP32: 'fp32', nat.MLP_BF16_FWD: 'bf16', nat.MLP_F16X3: 'f16x3'}[cfg.mlp_dtype]
    return HjbDecision(basis, basis_why, int(cfg.mlp_dtype), matrix_mode, guard, int(cfg.store_path), regen, int(cfg.sigma_kind),
                       d_pad, H_pad, family, sizes, alloc, ul2_mode, n_chunks, chunk_K, chunk_mode)


def _decide_chunks(solver, cfg, sizes, K_local, simple, cus, budget, query_rc):
    """(n_chunks, chunk_K, chunk_mode, sizes): the number of trajectory chunks from the path-store budget, the trajectories per
    chunk (a multiple of 16), 'two_gradient' | 'recompute' (None: one chunk) and the scratch sizes that serve every chunk.
    The default budget is five eighths of the device's TOTAL memory -- a function of the device alone, so the same seed and
    configuration give the same chunk count (hence the same summation order of the partial sums and gradients) from run to run
    and on every rank of a job, whatever else occupies the card; a store that then does not fit fails in its allocation and says
    so.  (A third measured worse: d = 500, K = 131 072, N = 200, a 120 GB store, paid its backward twice: 179 ms against 139 ms.)"""
    budget = getattr(solver, 'path_budget_bytes', None) or budget or DEFAULT_PATH_BUDGET
    forced = getattr(solver, 'path_chunks', None)
    n = int(forced) if forced else max(1, -(-int(sizes.path_bytes) // int(budget)))
    n = min(n, max(1, (K_local + 15) // 16))
    if n <= 1:
        return 1, K_local, None, sizes
    if solver.u_l2_error_flag and getattr(solver.problem, 'u_true_x_independent', False) is not True:
        raise PlanUnsupported('the u_L2 log of an x-dependent reference control reads the whole path store: not with K-chunking')
    Kc = -(-K_local // n)
    Kc = -(-Kc // 16) * 16
    if not forced:
        # whole launch waves: a chunk of a multiple of (16 trajectories x 4 tiles per workgroup x CUs) fills every CU the
        # same number of times (K = 1048576 under a 32 GiB budget: 32 chunks of 32768 instead of 29 ragged ones, +24 %)
        per_b = max(1, int(sizes.path_bytes) // max(1, K_local))          # store bytes per trajectory
        fit = int(budget) // per_b
        quantum = 16 * 4 * (cus if cus is not None else 256)              # (256: size queries on a machine without a GPU)
        if fit >= quantum:
            Kc = min(Kc if Kc % quantum == 0 else (fit // quantum) * quantum, (fit // quantum) * quantum)
    n = -(-K_local // Kc)
    if n <= 1:
        return 1, K_local, None, sizes
    # every DISTINCT chunk size is queried and each scratch buffer takes the maximum: the forward grid (hence the
    # fp64 partials, and in the wide family the operand tables behind them) is not monotone in K_local -- a ragged
    # last chunk can pick another forward kernel with a LARGER grid than the full chunks (K_local = 2064 in two
    # chunks: 65 tiles -> feature-split kernel, grid 65; 64 tiles -> quad kernel, grid 256)
    sizes = chunk_scratch_sizes(cfg, {Kc, K_local - (n - 1) * Kc}, query_rc)
    mode = getattr(solver, 'chunk_mode', 'auto')
    if mode == 'auto':
        mode = 'two_gradient' if simple else 'recompute'
    if mode == 'two_gradient' and not simple:
        raise PlanUnsupported("chunk_mode='two_gradient' needs a detached log-variance or moment run")
    if mode not in ('two_gradient', 'recompute'):
        raise ValueError("chunk_mode must be 'auto', 'two_gradient' or 'recompute'")
    return n, Kc, mode, sizes


class HjbNativePlan:
    def __init__(self, solver, noise='reference'):
        reason = native_eligibility(solver)
        if reason is not None:
            raise PlanUnsupported(reason)
        self.s, self.lib, self.noise, self.dev = solver, nat.load(), noise, solver.device
        dev = self.dev
        self.dist, self.rank, self.world, lo, hi = pc.local_shard(solver.K)
        self.K_local, self.k_offset = hi - lo, lo
        self.net = net = solver.z_n
        self.H = net.native_shape()[1]
        self.flat = pc.rehome_params(net.flat_layout(), dev)       # (psp.h layout)
        self.P = self.flat.numel()
        spec = solver.problem.native_spec()
        self._keep = []   # device tensors referenced by raw pointer from the config
        cfg = nat.HjbConfig()
        self.generic_loss, self.relent, self.attached = pc.fill_hjb_base(cfg, solver, spec, noise, self.K_local, self.k_offset)
        # the one look at the device: its CU count (the size rules) and five eighths of its memory (the path-store budget)
        props = torch.cuda.get_device_properties(dev) if torch.device(dev).type == 'cuda' else None
        self.cus = props.multi_processor_count if props is not None else None
        budget = max(1 << 28, int(props.total_memory) * 5 // 8) if props is not None else None
        self.decision = dec = decide(solver, spec, cfg, self.K_local, self.world, self.cus, budget)
        self.state_basis, self.state_basis_reason, self.matrix_mode = dec.state_basis, dec.state_basis_reason, dec.matrix_mode
        self.d_pad, self.H_pad, self.family, self.regen_xi = dec.d_pad, dec.H_pad, dec.family, dec.regen_xi
        self.n_chunks, self.chunk_K, self.chunk_mode, self.sizes = dec.n_chunks, dec.chunk_K, dec.chunk_mode, dec.sizes
        cfg.d, cfg.H, cfg.sigma_kind, cfg.mlp_dtype, cfg.store_path = dec.d_pad, dec.H_pad, dec.sigma_kind, dec.mlp_dtype, dec.store_path
        self.range_flag = torch.zeros(4, dtype=torch.int32, device=dev) if dec.range_guard else None
        cfg.range_flag = nat.ptr(self.range_flag)
        solver.state_basis_plan = (self.state_basis, self.state_basis_reason)
        solver.path_plan = dict(n_chunks=self.n_chunks, chunk_mode=self.chunk_mode, chunk_K=self.chunk_K)   # what the budget chose
        self.cfg = cfg
        self.pad = pad = shapes.ParamPad(solver.d, self.H, self.d_pad, self.H_pad, dev)
        assert dec.alloc_sizes.n_params == pad.Pp, (dec.alloc_sizes.n_params, pad.Pp)
        x0_plan = self._upload_problem(spec)
        # kernel-side (padded) parameter and gradient vectors; identical to the real ones when nothing is padded
        # (sigma basis: always a buffer of its own -- it holds W1x B where self.flat, the nn.Parameter views, holds W1x)
        sizes = dec.alloc_sizes
        self.flat_k = self.flat if (pad.identity and self.state_basis != 'sigma') else pad.new_padded_params()
        self.path = torch.empty(sizes.path_bytes // 4, dtype=torch.float32, device=dev)
        self.fwd_partial = torch.empty(max(1, self.n_chunks) * (sizes.fwd_partial_bytes // 8), dtype=torch.float64, device=dev)
        self.grad_partial = torch.empty(sizes.grad_partial_bytes // 4, dtype=torch.float32, device=dev)
        self.D = torch.empty(self.K_local, dtype=torch.float32, device=dev)
        self.Yn = torch.empty(self.K_local, dtype=torch.float32, device=dev) if self.generic_loss else None
        self.w = torch.empty(self.K_local, dtype=torch.float32, device=dev) if self.generic_loss else None
        self.sums = torch.zeros(2, dtype=torch.float64, device=dev)
        self.grad = torch.empty(self.P, dtype=torch.float32, device=dev)
        self.grad_k = self.grad if pad.identity else torch.empty(pad.Pp, dtype=torch.float32, device=dev)
        self.m = torch.zeros(self.P, dtype=torch.float32, device=dev)
        self.v = torch.zeros(self.P, dtype=torch.float32, device=dev)
        self.x0_vec = self._dev_f32(pad.vec(x0_plan))
        self._alloc_ul2(dec.ul2_mode)
        if self.attached or self.relent:
            self.cfg_w = nat.HjbConfig.from_buffer_copy(cfg)          # backward with explicit trajectory weights
            self.cfg_w.loss_kind = nat.LOSS_WEIGHTS
            self.w_bwd = torch.empty(self.K_local, dtype=torch.float32, device=dev)
            if self.attached:
                self.XN_k = torch.empty(self.K_local, self.d_pad, dtype=torch.float32, device=dev)
                self.mu = torch.zeros(self.K_local, dtype=torch.float32, device=dev)
                self.nu = torch.zeros(self.K_local, dtype=torch.float32, device=dev)
                self.wT = torch.zeros(self.K_local, dtype=torch.float32, device=dev)
        self.step = sharding.adam_state_import(net.flat_layout(), self.m, self.v, getattr(net, 'optim', None))
        self.events = self.pass1_events = None   # bench.py: lists collecting HIP-event pairs around the rollout kernels
        if self.n_chunks > 1:
            self._alloc_chunks()
        # hipGraph replay of the launch-bound small-K iteration (module docstring of include/psp.h: psp_iter_state)
        self._graph, self._graph_key, self._graph_iter, self._eager_done, self.graph_active = None, None, -1, 0, False
        # learnable Y_0 (solver.py:372-374): a one-element Adam beside the net's; it continues the state y_0.optim carries
        self.learn_y0 = bool(solver.learn_Y_0)
        if self.learn_y0:
            self.y0 = pc.Y0Adam(solver.y_0, dev, import_state=True)
            self.y0_param = self.y0.param

    def _dev_f32(self, t):
        """`t` as a contiguous fp32 tensor on the plan's device, kept alive for the raw pointers that reference it (None: None)."""
        if t is None:
            return None
        t = t.detach().to(device=self.dev, dtype=torch.float32).contiguous()
        self._keep.append(t)
        return t

    def _upload_problem(self, spec):
        """The problem's coefficients on the device, padded, behind the pointers of self.cfg; returns the plan's X_0."""
        solver, cfg, pad, dev_f32 = self.s, self.cfg, self.pad, self._dev_f32
        x0_plan = solver.X_0.detach().to(self.dev)
        if self.state_basis == 'sigma':
            # the transformed problem, once per plan in fp64 on the host, rounded to fp32: M = B^-1 A B, alpha' = B^T alpha,
            # x~0 = B^-1 x0.  EVERY launch of the plan (forward, backward, the range guard's fp32 twins, chunks, ranks, the small-K
            # forwards) takes its problem from this one config.
            M, al, x0t = sigma_basis_problem(spec['drift'][1].detach().double().cpu().numpy(), spec['sigma'][1].detach().double().cpu().numpy(),
                                             spec['term'][1].detach().double().cpu().numpy(), solver.X_0.detach().double().cpu().numpy())
            self.basis_B = dev_f32(pad.mat(spec['sigma'][1]))                   # for the two per-iteration transforms
            cfg.drift = nat.ptr(dev_f32(pad.mat(torch.from_numpy(M).to(torch.float32))))
            cfg.sigma = None
            cfg.term = nat.ptr(dev_f32(pad.vec(torch.from_numpy(al).to(torch.float32))))
            x0_plan = torch.from_numpy(x0t).to(torch.float32).to(self.dev)
        else:
            self.basis_B = None
            cfg.drift = nat.ptr(dev_f32(pad.drift_or_sigma(spec['drift'][1]))) if spec['drift'][1] is not None else None
            cfg.sigma = nat.ptr(dev_f32(pad.drift_or_sigma(spec['sigma'][1]))) if spec['sigma'][1] is not None else None
            cfg.term = nat.ptr(dev_f32(pad.vec(spec['term'][1])))
        cfg.runcost = nat.ptr(dev_f32(pad.vec(spec['runcost'][1]))) if spec['runcost'][1] is not None else None
        return x0_plan

    def _alloc_ul2(self, mode):
        """The u_L2 log's reference control on the device in the form decide() chose: one of self.ul2 / ul2_gain / ul2_tab, or none."""
        solver, dev = self.s, self.dev
        self.ul2 = self.ul2_gain = self.ul2_tab = None
        if mode == 'ul2_tab':
            # u*(x, t) tabulated per coordinate on a grid (the double wells: problems.py u_true_tables, reference problems.py:
            # 277-281, 399-404, 471-476): the tables go to the device once, the log is formed from the path store (_ul2_from_path)
            tb = pc.u_tables(solver.problem)
            self.ul2_tab = dict(tables=[torch.tensor(np.asarray(t), dtype=torch.float32, device=dev) for t in tb['tables']],
                                group=torch.tensor(tb['group_of_dim'], dtype=torch.long, device=dev),
                                xb=float(tb['xb']), dx=float(tb['dx']),
                                n_ref=[int(np.ceil(n * solver.delta_t_np / tb['delta_t'])) for n in range(solver.N)])
            self.XN_k = torch.empty(self.K_local, self.d_pad, dtype=torch.float32, device=dev)
        elif mode == 'ul2_gain':
            # u*(x, t_n) = M_n x (LQGC, problems.py:169-171): M_n once per plan by probing u_true with the unit vectors; the log
            # is then formed from the X_n and h2 images of the path store after the forward kernel (_ul2_from_path)
            eye = torch.eye(solver.d)
            gains = [torch.tensor(np.asarray(solver.problem.u_true(eye, n * solver.delta_t_np))).reshape(solver.d, solver.d).float()
                     for n in range(solver.N)]                                       # u_true returns (d, K): column i = M e_i
            self.ul2_gain = torch.stack(gains).to(dev)                             # (N, d, d) = M_n
            self.XN_k = torch.empty(self.K_local, self.d_pad, dtype=torch.float32, device=dev)
        elif mode == 'ul2':
            # u_L2 log (solver.py:491-494) for an x-independent reference control: u*(t_n) once per plan instead of
            # problem.u_true(X.cpu(), t_n) every step of every iteration; the kernels accumulate |-Z_n - u*(t_n)|^2 dt
            probe = torch.zeros(1, solver.d)
            rows = [torch.tensor(np.asarray(solver.problem.u_true(probe, n * solver.delta_t_np))).reshape(solver.d, -1)[:, 0].float()
                    for n in range(solver.N)]
            table = self.pad.last_dim(torch.stack(rows).to(dev)).reshape(-1)
            self.uref = self._dev_f32(torch.cat([table, torch.zeros(16, device=dev)]))   # 16 floats of slack: the kernels read whole blocks
            self.ul2 = torch.zeros(self.K_local, dtype=torch.float32, device=dev)
            self.cfg.u_ref, self.cfg.u_l2_out = nat.ptr(self.uref), nat.ptr(self.ul2)

    def _stream(self):
        return nat.stream_ptr(self.dev)

    def _kernel_params(self, st):
        """The kernel-layout parameter vector of this iteration: self.flat itself, its zero-padded scatter, or -- sigma basis -- one
        launch that copies it into self.flat_k with W1x B in place of W1x (psp_hjb_basis_params; capturable, no host sync)."""
        if self.state_basis != 'sigma':
            return self.pad.scatter_params(self.flat, self.flat_k)
        src = self.pad.scatter_params(self.flat, self.flat_k)          # identity padding: self.flat; else scattered into flat_k
        nat.check(self.lib.psp_hjb_basis_params(nat.ptr(src), nat.ptr(self.flat_k), nat.ptr(self.basis_B), self.d_pad, self.H_pad,
                                                self.pad.Pp, st), 'psp_hjb_basis_params')
        return self.flat_k

    def _grad_to_x_basis(self, st):
        """sigma basis: dW1x = dW~1x B^T on the kernel-layout gradient (linear: before the all-reduce is as good as after)."""
        if self.state_basis == 'sigma':
            nat.check(self.lib.psp_hjb_basis_grad(nat.ptr(self.grad_k), nat.ptr(self.basis_B), self.d_pad, self.H_pad, st),
                      'psp_hjb_basis_grad')

    # ---- the three rollout launches: the eager, chunked and captured iterations and forward_only all launch through these ----
    def _seed(self):
        return int(self.s.seed) & 0xFFFFFFFFFFFFFFFF

    def _launch_fwd(self, cfg, flat_k, x0, xi, l, *, off=0, store=True, XN=None, Yn=None, partial_off=0, st):
        """psp_hjb_rollout_fwd on the trajectories of `cfg`, which start `off` into this rank's.  x0: (K_local, d_pad) start points
        or None (the plan's fixed X_0); xi: the launch's own noise or None (Philox); XN, Yn: this rank's whole output tensors, or
        None for an output the caller does not take; partial_off: this launch's slice of the fp64 partials."""
        x0_p, x0_stride = (nat.ptr(x0, off * self.d_pad), self.d_pad) if x0 is not None else (nat.ptr(self.x0_vec), 0)
        nat.check(self.lib.psp_hjb_rollout_fwd(C.byref(cfg), nat.ptr(flat_k), x0_p, x0_stride,
                                               nat.ptr(self.y0_param) if self.learn_y0 else None, nat.ptr(xi), self._seed(), l,
                                               nat.ptr(self.path) if store else None, nat.ptr(self.D, off), nat.ptr(XN, off * self.d_pad),
                                               nat.ptr(Yn, off), nat.ptr(self.fwd_partial, partial_off), st), 'psp_hjb_rollout_fwd')

    def _launch_sweep(self, cfg, flat_k, wT, st, off=0, partial_off=0):
        """psp_hjb_adjoint_sweep (attached forward process) over the store the forward of `cfg` left; wT: terminal weights or None."""
        nat.check(self.lib.psp_hjb_adjoint_sweep(C.byref(cfg), nat.ptr(flat_k), nat.ptr(self.path), nat.ptr(self.XN_k, off * self.d_pad),
                                                 nat.ptr(self.mu, off), nat.ptr(self.nu, off) if self.relent else None, nat.ptr(wT, off),
                                                 nat.ptr(self.fwd_partial, partial_off), st), 'psp_hjb_adjoint_sweep')

    def _launch_bwd(self, cfg, flat_k, xi, l, w, w_off, out, out_off, st):
        """psp_hjb_rollout_bwd over the store: D or weights from w[w_off:], the kernel-layout gradient into out[out_off:]."""
        nat.check(self.lib.psp_hjb_rollout_bwd(C.byref(cfg), nat.ptr(flat_k), nat.ptr(xi), self._seed(), l, nat.ptr(self.path),
                                               nat.ptr(w, w_off), nat.ptr(self.sums), nat.ptr(self.grad_partial), nat.ptr(out, out_off),
                                               st), 'psp_hjb_rollout_bwd')

    # ---- K-chunking (module docstring) -------------------------------------------------------------------------------
    def _alloc_chunks(self):
        """Per-chunk configs (K_local, k_offset and the per-trajectory output pointers moved to the chunk) and the small
        per-chunk result rows; the big scratch buffers (path store, partial gradients) are shared by all chunks."""
        dev, cfg, n, Kc = self.dev, self.cfg, self.n_chunks, self.chunk_K
        self.chunks = []
        for i in range(n):
            off = i * Kc
            k = min(Kc, self.K_local - off)
            c = nat.HjbConfig.from_buffer_copy(cfg)
            c.K_local, c.k_offset = k, self.k_offset + off
            if self.ul2 is not None:
                c.u_l2_out = nat.ptr(self.ul2, off)
            c0 = nat.HjbConfig.from_buffer_copy(c)       # pass 1 of 'recompute': no path store
            c0.store_path = 0
            cw = nat.HjbConfig.from_buffer_copy(c)       # backward with explicit trajectory weights
            cw.loss_kind = nat.LOSS_WEIGHTS
            self.chunks.append((off, k, c, c0, cw))
        self.sums_c = torch.zeros(n, 2, dtype=torch.float64, device=dev)
        Pp = self.pad.Pp
        self.grad_rows = torch.zeros(n, Pp, dtype=torch.float32, device=dev)
        if self.chunk_mode == 'two_gradient' and self.s.loss_method == 'log-variance':
            self.grad_rows0 = torch.zeros(n, Pp, dtype=torch.float32, device=dev)
            self.w_chunk = torch.empty(Kc, dtype=torch.float32, device=dev)
            self.ones_chunk = torch.ones(Kc, dtype=torch.float32, device=dev)
        self.fp_stride = self.sizes.fwd_partial_bytes // 8

    def _iteration_chunked(self, l, loss_out, ul2_out=None):
        s, lib, cfg, st = self.s, self.lib, self.cfg, self._stream()
        xi_full, x0 = pc.draw_noise(s, l, self.noise, self.k_offset, self.K_local, self.d_pad, self.dev)
        flat_k = self._kernel_params(st)
        K = float(s.K)

        def fwd(i, c, store):
            off, k = self.chunks[i][0], self.chunks[i][1]
            xi = xi_full[:, off:off + k].contiguous() if xi_full is not None else None
            self._launch_fwd(c, flat_k, x0, xi, l, off=off, store=store, XN=self.XN_k if (self.attached and store) else None,
                             Yn=self.Yn, partial_off=i * self.fp_stride, st=st)
            nat.check(lib.psp_hjb_terminal_reduce(C.byref(c), nat.ptr(self.fwd_partial, i * self.fp_stride),
                                                  nat.ptr(self.sums_c, 2 * i), st), 'psp_hjb_terminal_reduce')
            return xi

        def bwd(i, c, w_t, w_off, out_rows, xi):
            self._launch_bwd(c, flat_k, xi, l, w_t, w_off, out_rows, i * self.pad.Pp, st)

        def events():
            return [torch.cuda.Event(enable_timing=True) for _ in range(4)] if self.events is not None else None

        if self.chunk_mode == 'two_gradient':
            logvar = s.loss_method == 'log-variance'
            for i, (off, k, c, c0, cw) in enumerate(self.chunks):
                ev = events()
                if ev:
                    ev[0].record()
                xi = fwd(i, c, True)
                if ev:
                    ev[1].record()
                if logvar:
                    if i == 0:
                        shift = (self.sums_c[0, 0] / float(k)).to(torch.float32)       # device scalar, no sync
                    torch.sub(self.D[off:off + k], shift, out=self.w_chunk[:k])
                    if ev:
                        ev[2].record()
                    bwd(i, cw, self.w_chunk, 0, self.grad_rows, xi)
                    if ev:
                        ev[3].record()
                        self.events.append(ev)
                    bwd(i, cw, self.ones_chunk, 0, self.grad_rows0, xi)
                else:                                    # moment: w_k = (2/K) D_k needs nothing global
                    if ev:
                        ev[2].record()
                    bwd(i, c, self.D, off, self.grad_rows, xi)
                    if ev:
                        ev[3].record()
                        self.events.append(ev)
            torch.sum(self.sums_c, 0, out=self.sums)
            sharding.allreduce_sum_(self.sums)           # collective 1: 16 bytes
            loss = sharding.loss_from_sums(self.sums, s.K, s.loss_method)
            if logvar:
                g1, g0 = self.grad_rows.sum(0), self.grad_rows0.sum(0)
                corr = (self.sums[0] / K - shift.double()).to(torch.float32)
                torch.mul(g1 - corr * g0, 2.0 / K, out=self.grad_k)
            else:
                torch.sum(self.grad_rows, 0, out=self.grad_k)
        else:
            # pass 1: forward without the path store -> D, global sums, loss weights
            p1 = None
            if self.pass1_events is not None:
                p1 = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                p1[0].record()
            for i, (off, k, c, c0, cw) in enumerate(self.chunks):
                fwd(i, c0, False)
            if p1:
                p1[1].record()
                self.pass1_events.append(p1)
            torch.sum(self.sums_c, 0, out=self.sums)
            sharding.allreduce_sum_(self.sums)           # collective 1
            w_t, use_w = self.D, False
            if self.generic_loss:
                loss, w_t = sharding.generic_loss_weights(s.loss_method, s.adaptive_forward_process, self.D, self.Yn, s.K, self.w)
                use_w = True
            else:
                loss = sharding.loss_from_sums(self.sums, s.K, s.loss_method)
            if self.attached:
                wT = pc.attached_weights(s.loss_method, self.relent, s.K, self._dL_dY(w_t), self.Yn, self.mu, self.nu, self.wT)
                self.w_bwd.fill_(1.0)
                w_t, use_w = self.w_bwd, True
            elif self.relent:
                self.w_bwd.fill_(float(cfg.sqrt_dt) / K)
                w_t, use_w = self.w_bwd, True
            # pass 2: forward with the store (bit-identical rollout), [adjoint sweep,] backward
            for i, (off, k, c, c0, cw) in enumerate(self.chunks):
                ev = events()
                if ev:
                    ev[0].record()
                xi = fwd(i, c, True)
                if ev:
                    ev[1].record()
                    ev[2].record()
                if self.attached:
                    self._launch_sweep(c, flat_k, wT, st, off=off, partial_off=i * self.fp_stride)
                bwd(i, cw if use_w else c, w_t, off, self.grad_rows, xi)
                if ev:
                    ev[3].record()
                    self.events.append(ev)
            torch.sum(self.grad_rows, 0, out=self.grad_k)
        loss_out[l] = loss.to(torch.float32)
        if self.ul2 is not None and ul2_out is not None:
            pc.log_mean_ul2(self.ul2, s.K, ul2_out, l)
        self._finish_step(st, self.w if self.generic_loss else None)
        return loss

    # ---- hipGraph replay ---------------------------------------------------------------------------------------------
    def _graph_wanted(self):
        """The iteration is captured into a hipGraph when it is launch-bound (at most two 16-trajectory tiles per CU, the
        regime of the feature-split forward kernel) and nothing in it needs a per-iteration host argument: on-device noise,
        fixed X_0, a loss the kernels form themselves (with or without the adjoint sweep of an attached forward process: its
        trajectory weights are device arithmetic on D and the sums), one rank, no u_L2 log.  Solver(use_graph=True / False) overrides
        the size rule (never the eligibility)."""
        want = getattr(self.s, 'use_graph', 'auto')
        ok = (self.world == 1 and self.noise == 'philox' and not self.s.random_X_0 and not self.generic_loss
              and self.ul2 is None and self.ul2_gain is None and self.ul2_tab is None and self.n_chunks == 1)
        if want is False or not ok:
            return False
        return want is True or launch_bound(self.K_local, self.cus)

    def _graph_state_upload(self, l):
        b = self._graph_hyper
        st = nat.IterState()
        nat.check(self.lib.psp_iter_state_init(C.byref(st), int(l), int(self.step) + 1, b[1], b[2]), 'psp_iter_state_init')
        host = torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8)
        self._gstate.copy_(host)
        self._graph_iter = l

    def _graph_body(self, loss_out):
        """The launches of one iteration with every per-iteration quantity read from the device psp_iter_state."""
        s, lib, cfg, st = self.s, self.lib, self._gcfg, self._stream()
        state = nat.ptr(self._gstate)
        flat_k = self._kernel_params(st)
        self._launch_fwd(cfg, flat_k, None, None, 0, XN=self.XN_k if self.attached else None, st=st)
        nat.check(lib.psp_hjb_terminal_reduce_loss(C.byref(cfg), nat.ptr(self.fwd_partial), nat.ptr(self.sums),
                                                   nat.ptr(loss_out), state, st), 'psp_hjb_terminal_reduce_loss')
        d_or_w, bcfg = self.D, cfg
        if self.attached:
            # trajectory weights of the adjoint sweep (plain iteration: same call), sweep, backward with unit weights (w_bwd = 1)
            pc.attached_weights(s.loss_method, self.relent, s.K, self._dL_dY(None), None, self.mu, self.nu, None)
            self._launch_sweep(cfg, flat_k, None, st)
            d_or_w, bcfg = self.w_bwd, self._gcfg_w
        elif self.relent:                                # detached relative entropy: weight sqrt(dt) / K on the Z image
            d_or_w, bcfg = self.w_bwd, self._gcfg_w
        lr, b1, b2, eps = self._graph_hyper
        if self.pad.identity and not self.learn_y0 and self.state_basis != 'sigma':
            # backward + (gradient reduction, Adam, state advance) as two launches (sigma basis: the gradient transform stands
            # between the reduction and Adam -- the separate launches below)
            nat.check(lib.psp_hjb_rollout_bwd_step(C.byref(bcfg), nat.ptr(self.flat), nat.ptr(self.path), nat.ptr(d_or_w),
                                                   nat.ptr(self.sums), nat.ptr(self.grad_partial), nat.ptr(self.grad),
                                                   nat.ptr(self.m), nat.ptr(self.v), state, nat.ptr(self._gticket),
                                                   lr, b1, b2, eps, st), 'psp_hjb_rollout_bwd_step')
            return
        self._launch_bwd(bcfg, flat_k, None, 0, d_or_w, 0, self.grad_k, 0, st)
        self._grad_to_x_basis(st)
        self.pad.gather_grad(self.grad_k, self.grad)
        nat.check(lib.psp_adam_step_dev(nat.ptr(self.flat), nat.ptr(self.grad), nat.ptr(self.m), nat.ptr(self.v), self.P,
                                        state, lr, b1, b2, eps, st), 'psp_adam_step_dev')
        if self.learn_y0:
            y0 = self.y0
            y0.grad[0] = sharding.y0_gradient(self.sums, s.K, s.loss_method)
            ylr = pc.adam_hyper(s.y_0, s.lr, PlanUnsupported)[0]
            nat.check(lib.psp_adam_step_dev(nat.ptr(y0.param), nat.ptr(y0.grad), nat.ptr(y0.m),
                                            nat.ptr(y0.v), 1, state, ylr, b1, b2, eps, st), 'psp_adam_step_dev(Y_0)')
        nat.check(lib.psp_iter_state_advance(state, b1, b2, st), 'psp_iter_state_advance')

    def _iteration_graph(self, l, loss_out):
        hyper = pc.adam_hyper(self.net, self.s.lr, PlanUnsupported)
        if self.learn_y0 and pc.adam_hyper(self.s.y_0, self.s.lr, PlanUnsupported)[1:] != hyper[1:]:
            self.s.use_graph = False                     # different betas for Y_0: one psp_iter_state cannot serve both
            return self.iteration(l, loss_out)
        if self._eager_done < 1:
            # the first iteration runs eagerly: kernels are loaded and every buffer exists before anything is captured
            self._eager_done += 1
            ev, self.events = self.events, []
            try:
                return self.iteration(l, loss_out)
            finally:
                self.events = ev
        key = (loss_out.data_ptr(), hyper)
        if self._graph is None or self._graph_key != key:
            self._graph_hyper = hyper
            self._gstate = torch.zeros(24, dtype=torch.uint8, device=self.dev)
            self._gticket = torch.zeros(1, dtype=torch.int32, device=self.dev)
            self._gcfg = nat.HjbConfig.from_buffer_copy(self.cfg)
            self._gcfg.iter_dev = nat.ptr(self._gstate)
            if self.relent or self.attached:
                self._gcfg_w = nat.HjbConfig.from_buffer_copy(self._gcfg)
                self._gcfg_w.loss_kind = nat.LOSS_WEIGHTS
                self.w_bwd.fill_(1.0 if self.attached else float(self.cfg.sqrt_dt) / float(self.s.K))
            self._graph_state_upload(l)
            torch.cuda.synchronize(self.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._graph_body(loss_out)
            self._graph, self._graph_key = g, key
        if self._graph_iter != l:                        # the caller jumped to another iteration index
            self._graph_state_upload(l)
        self._graph.replay()
        self._graph_iter += 1
        self.step += 1
        self.graph_active = True
        return loss_out[l]

    def _ul2_from_path(self):
        """This rank's share of the u_L2 log: the sum of _ul2_rows_from_path() over the GLOBAL K."""
        return self._ul2_rows_from_path().sum() / float(self.s.K)

    def _ul2_rows_from_path(self):
        """u_L2 log (solver.py:491-494) for a reference control that is linear in x (LQGC) or tabulated per coordinate (the double
        wells): (K_local,) values sum_n |-Z_n - u*(X_{n+1}, t_n)|^2 dt, one per trajectory of this rank, from the register images
        the forward kernel left in the path store (the same layout in both kernel families, every matrix mode and every store_path;
        tests/test_gpu_solver_ul2.py holds each of them to float64) -- block (n, tile): X_n image at float 0, h2 image behind the h1 image; image float ks * 64 + 16 q + j holds feature 4 ks + q of sample j (csrc/hjb_kernels.h
        Geo::pX / pH2).  Z_n = W3 h2 + b3 with the net's own parameters.  A diagnostic: K N small products in torch, skipped
        with u_l2_error_flag=False (as the timed runs do)."""
        s = self.s
        N, nt = s.N, (self.K_local + 15) // 16
        PB = self.sizes.path_bytes // 4 // (N * nt)
        DBp, HBp = (self.d_pad + 15) // 16, (self.H_pad + 15) // 16
        blocks = self.path.view(N, nt, PB)

        def image(off, nb):
            img = blocks[:, :, off:off + 4 * nb * 64].reshape(N, nt, 4 * nb, 4, 16)
            return img.permute(0, 1, 4, 2, 3).reshape(N, nt * 16, 16 * nb)[:, :self.K_local]
        # the reference compares -Z_n(X_n) with u*(X_{n+1}, t_n): the log line sits AFTER the Euler step (solver.py:471-472, 491-494)
        X = torch.cat([image(0, DBp)[1:, :, :s.d], self.XN_k[:, :s.d].unsqueeze(0)], 0)
        h2 = image(4 * DBp * 64 + 4 * HBp * 64, HBp)[:, :, :self.H]
        lin = self.net.linears[-1]
        with torch.no_grad():
            Z = h2 @ lin.weight.t() + lin.bias                                  # (N, K, d)
            if self.ul2_tab is not None:
                # the double wells: u*_i = table_{g(i)}[ceil(t_n / dt_ref), cell(x_i)], cell = floor((clamp(x) + xb) / dx) in fp32 as the
                # reference computes it -- which also lowers the index of the LAST trajectory of the batch by two (problems.py:270)
                tb = self.ul2_tab
                cell = torch.floor((torch.clamp(X, -tb['xb'], tb['xb'] - 2 * tb['dx']) + tb['xb']) / tb['dx']).long()
                if self.k_offset + self.K_local == s.K:
                    cell[:, -1, :] -= 2
                tot = torch.zeros(self.K_local, dtype=torch.float32, device=self.dev)
                for n in range(N):                                              # (per step: bounds the index tensors)
                    u_ref = torch.empty(self.K_local, s.d, device=self.dev)
                    for gi, tab in enumerate(tb['tables']):
                        dims = torch.nonzero(tb['group'] == gi).flatten()
                        if dims.numel():
                            u_ref[:, dims] = tab[tb['n_ref'][n]][cell[n][:, dims]]
                    tot = tot + ((-Z[n] - u_ref) ** 2).sum(1)
                return tot * s.delta_t
            u_ref = torch.bmm(X, self.ul2_gain.transpose(1, 2))                 # M_n X_{n+1}
            return ((-Z - u_ref) ** 2).sum((0, 2)) * s.delta_t

    def _finish_step(self, st, w_generic):
        """Gather the real gradient entries, all-reduce, Adam on the net and on the learnable Y_0."""
        s, lib = self.s, self.lib
        self._grad_to_x_basis(st)
        self.pad.gather_grad(self.grad_k, self.grad)    # real entries of the (possibly padded) gradient
        sharding.allreduce_sum_(self.grad)              # collective 2: p floats
        self.step += 1
        pc.adam_step(lib, self.flat, self.grad, self.m, self.v, self.P, self.step, pc.adam_hyper(self.net, s.lr, PlanUnsupported), st)
        if self.learn_y0:
            self.y0.step(lib, self.sums, s.K, s.loss_method, w_generic, self.step,
                         pc.adam_hyper(s.y_0, s.lr, PlanUnsupported), st)

    def range_fallbacks(self):
        return pc.range_fallbacks(self.range_flag)

    def export_optimizer_state(self):
        """Called by Solver._train_native when training returns: the nets' own optimisers see the moments this plan kept."""
        sharding.adam_state_export(self.net.flat_layout(), self.m, self.v, self.step, getattr(self.net, 'optim', None))
        if self.learn_y0:
            self.y0.export(self.step)

    def _dL_dY(self, w_generic):
        """dL/dY_k of this rank's trajectories, for the adjoint sweep: the weights the plan formed itself (generic losses),
        those of the global sums (log-variance, moment), or None (relative entropy: the sweep's weights are constants)."""
        if self.generic_loss:
            return w_generic
        return None if self.relent else sharding.loss_weights(self.D, self.sums, self.s.K, self.s.loss_method)

    def iteration(self, l, loss_out, ul2_out=None):
        """One training iteration; writes the fp32 loss into loss_out[l] (and mean u_L2 into ul2_out[l]) on the
        device, no sync."""
        if self.n_chunks > 1:
            return self._iteration_chunked(l, loss_out, ul2_out)
        if self._graph_wanted() and self.events is None:
            return self._iteration_graph(l, loss_out)
        s, lib, cfg, st = self.s, self.lib, self.cfg, self._stream()
        xi, x0 = pc.draw_noise(s, l, self.noise, self.k_offset, self.K_local, self.d_pad, self.dev)
        flat_k = self._kernel_params(st)
        ev = None
        if self.events is not None:      # events go on torch's current stream = the launch stream
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
        want_XN = self.attached or self.ul2_gain is not None or self.ul2_tab is not None
        self._launch_fwd(cfg, flat_k, x0, xi, l, XN=self.XN_k if want_XN else None, Yn=self.Yn, st=st)
        if ev is not None:
            ev[1].record()
        d_or_w, bcfg = self.D, cfg
        if self.world == 1 and not self.generic_loss:
            # one rank: the local sums are the global ones -- sums and the loss value in ONE launch (no element-wise torch kernels)
            nat.check(lib.psp_hjb_terminal_reduce_loss(C.byref(cfg), nat.ptr(self.fwd_partial), nat.ptr(self.sums),
                                                       nat.ptr(loss_out, l), None, st), 'psp_hjb_terminal_reduce_loss')
            loss = loss_out[l]
        else:
            nat.check(lib.psp_hjb_terminal_reduce(C.byref(cfg), nat.ptr(self.fwd_partial), nat.ptr(self.sums), st),
                      'psp_hjb_terminal_reduce')
            sharding.allreduce_sum_(self.sums)              # collective 1: 16 bytes
            if self.generic_loss:
                loss, d_or_w = sharding.generic_loss_weights(s.loss_method, s.adaptive_forward_process, self.D, self.Yn, s.K,
                                                             self.w)
            else:
                loss = sharding.loss_from_sums(self.sums, s.K, s.loss_method)
            loss_out[l] = loss.to(torch.float32)
        if self.ul2 is not None and ul2_out is not None:
            pc.log_mean_ul2(self.ul2, s.K, ul2_out, l)
        elif (self.ul2_gain is not None or self.ul2_tab is not None) and ul2_out is not None:
            m = self._ul2_from_path().reshape(1)
            sharding.allreduce_sum_(m)
            ul2_out[l:l + 1] = m
        if ev is not None:
            ev[2].record()
        if self.attached:
            wT = pc.attached_weights(s.loss_method, self.relent, s.K, self._dL_dY(d_or_w), self.Yn, self.mu, self.nu, self.wT)
            self._launch_sweep(cfg, flat_k, wT, st)
            self.w_bwd.fill_(1.0)                       # the sweep left dL/dZ_n / sqrt(dt) in the xi slot
            d_or_w, bcfg = self.w_bwd, self.cfg_w
        elif self.relent:
            # detached relative entropy: dL/dZ_n = Z_n dt / K, and the xi slot holds Z_n  ->  weight sqrt(dt) / K
            self.w_bwd.fill_(float(cfg.sqrt_dt) / float(s.K))
            d_or_w, bcfg = self.w_bwd, self.cfg_w
        self._launch_bwd(bcfg, flat_k, xi, l, d_or_w, 0, self.grad_k, 0, st)
        if ev is not None:
            ev[3].record()
            self.events.append(ev)
        self._finish_step(st, self.w if self.generic_loss else None)
        # keep xi alive until the kernels that read it are enqueued on this stream (they are);
        # torch's caching allocator is stream-ordered, so freeing here is safe.
        return loss

    def forward_only(self, l, want_XN=False):
        """Forward rollout without the path store; returns (D, X_N or None)."""
        s = self.s
        cfg = nat.HjbConfig.from_buffer_copy(self.cfg)
        cfg.store_path = 0
        xi = x0 = None
        if self.noise == 'reference':                    # (under 'philox' this helper starts every trajectory at the fixed X_0)
            xi, x0 = pc.draw_noise(s, l, self.noise, self.k_offset, self.K_local, self.d_pad, self.dev)
        XN = torch.empty(self.K_local, self.d_pad, dtype=torch.float32, device=self.dev) if want_XN else None
        flat_k = self._kernel_params(self._stream())
        self._launch_fwd(cfg, flat_k, x0, xi, l, store=False, XN=XN, st=self._stream())
        if XN is not None and self.state_basis == 'sigma':
            XN = XN @ self.basis_B.t()                   # the kernel left X~_N; X_N = B X~_N (an evaluation helper, not the hot path)
        return self.D, (XN[:, :s.d] if XN is not None else None)
