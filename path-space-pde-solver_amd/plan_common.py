"""Host steps that the native plans take the same way, written once as plain functions.

Every function takes what it needs as arguments and returns what it makes; none takes a plan and reads its attributes, and none
asks which plan called it.  Where the plans differ on purpose (the exception class of a refusal, whether the optimiser state
of Y_0 is imported) the difference is an argument at the call site.  The launches, their order and the two collectives stay in
the plans' own ``iteration`` methods; the loss arithmetic on global sums stays in sharding.py.
"""
import numpy as np
import torch

try:
    from . import native as nat
    from . import sharding
except ImportError:
    import native as nat
    import sharding


class PlanUnsupported(Exception):
    """The (problem, net, loss, flags) combination is outside the native catalogue."""


# ---- parameters and their Adam ---------------------------------------------------------------------------------------------
def rehome_params(params, device):
    """Re-home the tensors of `params` as views of ONE flat fp32 buffer, in list order (include/psp.h layout per parameter set),
    and return it: state_dict / save_networks / Z_n keep working on live values, the fused Adam sees one vector."""
    flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=device)
    off = 0
    for p in params:
        n = p.numel()
        flat[off:off + n].copy_(p.detach().reshape(-1))
        p.data = flat[off:off + n].view(p.shape)
        off += n
    return flat


def adam_hyper(modules, default_lr, error):
    """(lr, beta1, beta2, eps) of the modules' OWN optimisers (function_space.py:131, 185: each ansatz space builds its Adam in
    its constructor and solver.py:198-200 steps every one of them) -- a swapped-in net keeps its learning rate; a module without
    ``optim`` gets (default_lr, 0.9, 0.999, 1e-8).  `modules` is one module or a list; one fused Adam runs over the concatenation
    of all parameter sets, so a list must agree.  What the native Adam does not implement raises `error`."""
    if not isinstance(modules, (list, tuple)):           # (one module: the per-iteration call of the launch-bound plans)
        return _module_adam_hyper(modules, default_lr, error)
    hyp = None
    for mod in modules:
        h = _module_adam_hyper(mod, default_lr, error)
        if hyp is not None and h != hyp:
            raise error('the per-step nets carry different Adam settings; the fused native Adam needs one')
        hyp = h
    return hyp


def _module_adam_hyper(mod, default_lr, error):
    opt = getattr(mod, 'optim', None)
    if opt is None or not opt.param_groups:
        return float(default_lr), 0.9, 0.999, 1e-8
    g = opt.param_groups[0]
    if g.get('weight_decay', 0) or g.get('amsgrad', False):
        raise error('the native Adam implements weight_decay = 0, amsgrad = False (the reference default)')
    b = g.get('betas', (0.9, 0.999))
    return float(g['lr']), float(b[0]), float(b[1]), float(g.get('eps', 1e-8))


def adam_step(lib, flat, grad, m, v, P, step, hyper, stream, what='psp_adam_step'):
    """psp_adam_step on the first P entries of (flat, grad, m, v) with hyper = (lr, beta1, beta2, eps)."""
    lr, b1, b2, eps = hyper
    nat.check(lib.psp_adam_step(nat.ptr(flat), nat.ptr(grad), nat.ptr(m), nat.ptr(v), P, step, lr, b1, b2, eps, stream), what)


class Y0Adam:
    """The learnable Y_0 (solver.py:372-374) of a Solver plan: its one-element parameter, gradient and Adam moments on the device.
    import_state: continue the moments that ``y_0.optim`` already carries (a previous torch run, a loaded checkpoint);
    `imported_step` is the step count found there (0: none, or not asked for)."""

    def __init__(self, y_0, device, import_state):
        self.y_0, self.param = y_0, y_0.Y_0
        self.m = torch.zeros(1, dtype=torch.float32, device=device)
        self.v = torch.zeros(1, dtype=torch.float32, device=device)
        self.grad = torch.zeros(1, dtype=torch.float32, device=device)
        self.imported_step = 0
        if import_state:
            self.imported_step = sharding.adam_state_import([self.param], self.m, self.v, getattr(y_0, 'optim', None))

    def step(self, lib, sums, K_global, loss_method, w_generic, step, hyper, stream):
        """dL/dY_0 = sum_k dL/dY_k from the GLOBAL sums (sharding.y0_gradient: exactly 0 for log-variance, (2/K) sum D for moment,
        the all-reduced sum of `w_generic` for the losses whose weights are formed on the host side), then psp_adam_step."""
        self.grad[0] = sharding.y0_gradient(sums, K_global, loss_method, w_generic)
        adam_step(lib, self.param, self.grad, self.m, self.v, 1, step, hyper, stream, 'psp_adam_step(Y_0)')

    def export(self, step):
        """``y_0.optim`` sees the moments kept here (sharding.adam_state_export)."""
        sharding.adam_state_export([self.param], self.m, self.v, step, getattr(self.y_0, 'optim', None))


# ---- trajectories of this rank, the HJB config, the per-iteration draws -----------------------------------------------------------
def local_shard(K):
    """(dist, rank, world, lo, hi): this rank's contiguous block [lo, hi) of K trajectories, split evenly."""
    dist, rank, world = sharding.dist_info()
    try:
        lo, hi = sharding.shard_bounds(K, rank, world)
    except ValueError as e:
        raise PlanUnsupported(str(e))
    return dist, rank, world, lo, hi


def fill_hjb_base(cfg, solver, spec, noise, K_local, k_offset):
    """The fields of a psp_hjb_config that follow from the solver and the problem's ``native_spec()`` alone.  d / H, mlp_dtype
    and the pointers stay with the caller (as does sigma_kind where the rollout runs in the sigma basis).  Returns
    (generic_loss, relent, attached):
      generic_loss  the loss weights are not affine in D: the plan forms them (PSP_LOSS_WEIGHTS);
      relent        relative entropy: the xi slot of the store holds Z_n (store_path 3);
      attached      gradients through the state path (the reference's default flags): forward with the attached-mode image in
                    the xi slot (store_path 2), reverse-time adjoint sweep, then the ordinary backward with unit weights."""
    s = solver
    cfg.K_local, cfg.N, cfg.K_global, cfg.k_offset = K_local, s.N, s.K, k_offset
    cfg.dt, cfg.sqrt_dt = float(s.delta_t.item()), float(s.sq_delta_t.item())
    cfg.drift_kind, cfg.sigma_kind, cfg.sigma_scale = spec['drift'][0], spec['sigma'][0], float(spec['sigma'][2])
    cfg.runcost_kind, cfg.term_kind = spec['runcost'][0], spec['term'][0]
    cfg.coord_split = int(spec.get('split', 0))           # per-coordinate kinds (DoubleWell_OU): DenseNet-control family only
    cfg.adaptive = 1 if s.adaptive_forward_process else 0
    cfg.loss_kind = {'log-variance': nat.LOSS_LOG_VARIANCE, 'moment': nat.LOSS_MOMENT,
                     'relative_entropy': nat.LOSS_REL_ENTROPY}.get(s.loss_method, nat.LOSS_WEIGHTS)
    generic_loss = cfg.loss_kind == nat.LOSS_WEIGHTS
    relent = s.loss_method == 'relative_entropy'
    attached = bool(s.adaptive_forward_process and not s.detach_forward)
    cfg.noise_mode = nat.NOISE_PHILOX if noise == 'philox' else nat.NOISE_SUPPLIED
    cfg.store_path = 3 if relent else (2 if attached else 1)
    return generic_loss, relent, attached


def pad_coeff(pad, t):
    """A coefficient of a ``native_spec()`` for a kernel instance of width pad.dp: matrices and per-coordinate vectors zero padded;
    a parameter vector shorter than d (the radial kinds' {kappa, r0, w} / {alpha, rho}) likewise -- the kernels stage dp floats."""
    if t is None or t.dim() == 2 or t.numel() == pad.d:
        return pad.drift_or_sigma(t)
    out = torch.zeros(max(pad.dp, t.numel()), dtype=t.dtype, device=t.device)
    out[:t.numel()] = t
    return out


def draw_noise(solver, l, noise, k_offset, K_local, d_pad, device):
    """The per-iteration draws that reach the kernels as arguments: (xi (N+1, K_local, d_pad), X_0 (K_local, d_pad)), zero
    padded and contiguous on `device`; None for what the kernels make themselves.
      'reference'  the reference's draws from the CPU generator, for ALL K trajectories and in ITS order -- randn(K, d) first if
                   random_X_0, then randn(K, d, N+1) (solver.py:367, 381) --, sliced to this rank, xi re-laid-out per step;
      'philox'     xi comes from the counters inside the kernels; a random X_0 from a device generator seeded per iteration."""
    s = solver
    lo, hi = k_offset, k_offset + K_local
    xi = x0 = None
    if noise == 'reference':
        if s.random_X_0:
            x0 = torch.randn(s.K, s.d)[lo:hi].contiguous().to(device)
        xi = torch.randn(s.K, s.d, s.N + 1)[lo:hi].permute(2, 0, 1).contiguous().to(device)
    elif s.random_X_0:
        g = torch.Generator(device=device)
        g.manual_seed(int(s.seed) * 1000003 + l)
        x0 = torch.randn(s.K, s.d, generator=g, device=device)[lo:hi].contiguous()
    if d_pad != s.d:
        pad = (0, d_pad - s.d)
        xi = torch.nn.functional.pad(xi, pad).contiguous() if xi is not None else None
        x0 = torch.nn.functional.pad(x0, pad).contiguous() if x0 is not None else None
    return xi, x0


# ---- after the forward ----------------------------------------------------------------------------------------------------
def attached_weights(loss_method, relent, K_global, w, Yn, mu, nu, wT):
    """Trajectory weights of the adjoint sweep of an attached forward process, written into the plan's buffers: mu = dL/dY_N,
    nu = dL/dZsum_N (global K and global mean: rank-independent).  `w` is dL/dY_k as the caller has formed it (unused for
    relative entropy: mu = 0, nu = 1/K).  Returns the buffer of the explicit terminal weight for the sweep, or None:
    mean(Y exp(-g(X_N) + Y.detach())) (cross entropy, solver.py:183-185) also depends on X_N through exp(-g), so
    lambda_N = -(Y_N exp(D) / K) grad g while dL/dY_N = exp(D) / K."""
    if relent:
        mu.zero_()
        nu.fill_(1.0 / float(K_global))
        return None
    mu.copy_(w)
    if loss_method == 'cross_entropy':
        wT.copy_(-Yn * w)
        return wT
    return None


def log_mean_ul2(ul2, K_global, ul2_out, l):
    """ul2_out[l] = the u_L2 log of this iteration: the per-trajectory values of every rank over the GLOBAL K; no host sync."""
    m = (ul2.sum() / float(K_global)).reshape(1)
    sharding.allreduce_sum_(m)
    ul2_out[l:l + 1] = m


def range_fallbacks(range_flag):
    """Iterations (chunk launches) the range guard sent to the fp32-MFMA kernels so far; one device read."""
    return int(range_flag[1].item()) if range_flag is not None else 0


# ---- u_L2 log: the description of the reference control u* that the forward kernels read --------------------------------------
def u_tables(problem):
    """problem.u_true_tables() (the double wells' finite-difference reference control, problems.py) or None."""
    fn = getattr(problem, 'u_true_tables', None)
    return fn() if fn is not None else None


def ul2_kind(problem):
    """Which description of the reference control u* the forward kernel can log u_L2 against (include/psp.h PSP_UL2_*): 2 the
    grid tables of the double wells (problem.u_true_tables()), 0 a u* that does not depend on x, 1 a u* linear in x; None: none."""
    if u_tables(problem) is not None:
        return nat.UL2_GRID
    if getattr(problem, 'u_true_x_independent', False) is True:
        return nat.UL2_TABLE
    if getattr(problem, 'u_true_linear_in_x', False) is True:
        return nat.UL2_LINEAR
    return None


def ul2_unsupported(problem, N, dt_np):
    """None if the forward kernel can log u_L2 for this problem on the time grid (N steps of dt_np), else the precise reason."""
    kind = ul2_kind(problem)
    if kind is None:
        return ('u_l2_error_flag=True evaluates problem.u_true(X_n, t_n) on the host every step (reference solver.py:491-494); '
                'the forward kernel logs u_L2 for a u_true that does not depend on x (u_true_x_independent), is linear in x '
                '(u_true_linear_in_x) or is tabulated per coordinate (u_true_tables(), e.g. a double well after '
                'compute_reference_solution) -- this problem has none of these; pass u_l2_error_flag=False for the native plan')
    if kind != nat.UL2_GRID:
        return None
    tb = u_tables(problem)
    shapes = [np.shape(t) for t in tb['tables']]
    if any(len(sh) != 2 or sh != shapes[0] for sh in shapes):
        return ('the u_true_tables() of this problem have unequal shapes %s; the forward kernel reads tables of one '
                '(rows, cells) shape' % shapes)
    last = int(np.ceil((N - 1) * dt_np / tb['delta_t'])) if N > 0 else 0
    if last >= shapes[0][0]:
        return ('the u_true_tables() of this problem end at t = %g (%d rows of dt_ref = %g); the solver reads row %d at t = %g'
                % ((shapes[0][0] - 1) * tb['delta_t'], shapes[0][0], tb['delta_t'], last, (N - 1) * dt_np))
    return None


def ul2_reference(problem, N, dt_np, d_pad, K_global, k_offset):
    """Host-side description of u*(x, t_n), n < N, for the u_L2 log of the DenseNet-control forward kernel, padded to d_pad
    (CPU tensors; None when the problem has no description the kernel reads -- see ul2_kind).  t_n = n * dt_np as the reference
    forms it (solver.py:493).  Keys: 'kind', 'd', 'K_global', 'k_offset' and
      kind 0: 'table' (N, d_pad) u*(t_n)                                     -- probed at x = 0 (plan_native.py recipe)
      kind 1: 'gains' (N, d_pad, d_pad) M_n with u*(x, t_n) = M_n x          -- probed with the unit vectors
      kind 2: 'tables' (G, nrows, ncols) fp32, 'group' (d_pad) int32, 'row' (N) int32 = ceil(t_n / dt_ref), 'xb', 'dx', 'xhi' =
              fp32(xb - 2 dx) (formed in double, as the reference's clamp bound), 'nrows', 'ncols'.
    The cell arithmetic of kind 2 (clamp, true fp32 division, the last global trajectory lowered by two, numpy wrap-around) is the
    kernel's (csrc/hjbd_kernels.h); K_global / k_offset locate that trajectory.  Raises ValueError with ul2_unsupported's reason
    for grid tables the kernel cannot read."""
    kind = ul2_kind(problem)
    if kind is None:
        return None
    reason = ul2_unsupported(problem, N, dt_np)
    if reason is not None:
        raise ValueError(reason)
    d = problem.d
    out = dict(kind=kind, d=d, K_global=int(K_global), k_offset=int(k_offset))
    if kind == nat.UL2_TABLE:
        probe = torch.zeros(1, d)
        rows = [torch.tensor(np.asarray(problem.u_true(probe, n * dt_np))).reshape(d, -1)[:, 0].float() for n in range(N)]
        table = torch.zeros(N, d_pad)
        table[:, :d] = torch.stack(rows)
        out['table'] = table
    elif kind == nat.UL2_LINEAR:
        eye = torch.eye(d)
        gains = torch.zeros(N, d_pad, d_pad)
        for n in range(N):                                   # u_true returns (d, K): column j = M e_j
            gains[n, :d, :d] = torch.tensor(np.asarray(problem.u_true(eye, n * dt_np))).reshape(d, d).float()
        out['gains'] = gains
    else:
        tb = u_tables(problem)
        tabs = [np.asarray(t, dtype=np.float32) for t in tb['tables']]
        nrows, ncols = tabs[0].shape
        group = torch.zeros(d_pad, dtype=torch.int32)
        group[:d] = torch.tensor(tb['group_of_dim'], dtype=torch.int32)
        xb, dx = float(tb['xb']), float(tb['dx'])
        rows = [int(np.ceil(n * dt_np / tb['delta_t'])) for n in range(N)]
        const = tb.get('constant')
        if const:
            # coordinates whose u* does not depend on x (DoubleWell_OU): per-STEP tables with row[n] = n -- the grid tables
            # gathered at their rows, and one table per distinct u*_i(t_n) that is constant along the cell axis
            tabs = [t[rows] for t in tabs]
            vals, index = [], {}
            for i in sorted(const):
                v = tuple(float(np.float32(const[i](n * dt_np))) for n in range(N))
                if v not in index:
                    index[v] = len(tabs) + len(vals)
                    vals.append(v)
                group[i] = index[v]
            tabs += [np.repeat(np.asarray(v, dtype=np.float32).reshape(N, 1), ncols, 1) for v in vals]
            rows, nrows = list(range(N)), N
        out.update(tables=torch.from_numpy(np.ascontiguousarray(np.stack(tabs))), group=group,
                   row=torch.tensor(rows, dtype=torch.int32),
                   xb=float(np.float32(xb)), dx=float(np.float32(dx)), xhi=float(np.float32(xb - 2 * dx)),
                   nrows=int(nrows), ncols=int(ncols))
    return out


# ---- the K_test_log diagnostic of the GeneralSolver / EllipticSolver plans --------------------------------------------------------
def device_test_log(solver, net_spec, elliptic, device):
    """test_log='device': the K_test_log diagnostic on the plan's stream (device_test_log.py); every rank evaluates all
    K_test_log points with its replicated parameters -- no collective, identical logs.  None: the host log.  `net_spec` is the
    plan's plan_general_deep.value_net_spec of solver.V, or None for a plan that keeps none (it is formed here then)."""
    s = solver
    if getattr(s, 'test_log', 'reference') != 'device' or s.K_test_log is None:
        return None
    try:
        from . import device_test_log as dtl
        from .plan_general_deep import value_net_spec
    except ImportError:
        import device_test_log as dtl
        from plan_general_deep import value_net_spec
    why = dtl.eval_reason(s.problem)
    net = net_spec or value_net_spec(s.V, s.d + (0 if elliptic else 1))
    if why is None and isinstance(net, str):
        why = net
    if why is not None:
        raise ValueError("test_log='device' unavailable: " + why)
    return dtl.DeviceTestLog(net, s.problem, s.K_test_log, 'elliptic' if elliptic else 'parabolic', device, max(1, s.L))


def read_test_log(solver, test_log):
    """The one read-back of the device test log."""
    l2, mae, mre = test_log.read()
    solver.V_test_L2 += l2
    solver.V_test_abs += mae
    solver.V_test_rel_abs += mre


def train_with_test_log(solver, test_log, loop):
    """loop() -- a plan's training loop -- with the device test log (None: just the loop) begun before it and read back once
    after it."""
    if test_log is None:
        return loop()
    test_log.begin(max(1, solver.L))
    try:
        loop()
    except BaseException:                                        # the log of the iterations that ran; the loop's error survives
        try:
            read_test_log(solver, test_log)
        except Exception:
            pass
        raise
    read_test_log(solver, test_log)
