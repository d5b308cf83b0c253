"""Evaluation utilities -- API mirror of the hot-path-adjacent part of the reference's utilities.py.

``do_importance_sampling_me`` (reference utilities.py:287-359) estimates E[exp(-int f - g(X_T))] under the
learned control with the Girsanov weight and reports mean, variance and relative error.  It is the
same controlled Euler-Maruyama rollout as the training step, forward only, at ``K`` up to 1e7
(SURVEY.md 8f rank 1), and is called from Solver.train every ``IS_variance_iter`` iterations when
``IS_variance_K > 0`` (solver.py:521-528).

Native plan: psp_hjb_rollout_eval (include/psp.h) on the solver's control net whenever the solver is
native-eligible; composite torch plan otherwise.  Plotting helpers of the reference are out of scope.

``loss_relative_errors`` is not in the reference's utilities.py: it is the cell of its notebook `Compare relative errors of
losses.ipynb` (a forward-only rollout of a bare net at K = 5e7 and the statistics of five loss estimators) as a function, in
chunks on the forward kernels with the statistics reduced on the device in double (psp_loss_stats_*, csrc/lstat_kernels.h).
"""
import ctypes as C

import numpy as np
import torch

try:
    from . import native as nat
    from . import native_shapes as shapes
except ImportError:
    import native as nat
    import native_shapes as shapes


def _time_feature_table(model, N, delta_t):
    """Network time input the reference uses at IS step n: Z_n(X, n*delta_t) -> index ceil(t/model.delta_t)
    in fp32 (solver.py:360-362), then ones * index * model.delta_t (solver.py:355)."""
    dt32 = model.delta_t.detach().cpu()
    vals = []
    for n in range(N):
        t = torch.as_tensor(n * delta_t, dtype=torch.float32)
        idx = int(torch.ceil(t / dt32))
        vals.append(float((torch.ones(1) * idx * dt32).item()))
    return torch.tensor(vals, dtype=torch.float32)


def _native_reason(problem, model, control, simulate_naive):
    try:
        from .plan_native import native_eligibility
    except ImportError:
        from plan_native import native_eligibility
    if control != 'approx' and model.u_l2_error_flag:
        return "control='true' evaluates problem.u_true on the host"
    if simulate_naive:
        return 'simulate_naive needs the uncontrolled process too'
    if getattr(model, 'backend', 'auto') == 'torch':
        return "backend='torch' requested"
    saved = (model.IS_variance_K, model.u_l2_error_flag)
    model.IS_variance_K, model.u_l2_error_flag = 0, False          # these two do not matter for the evaluation itself
    try:
        return native_eligibility(model)
    finally:
        model.IS_variance_K, model.u_l2_error_flag = saved


def _stats(logw):
    w = torch.exp(logw)
    mean_IS = torch.mean(w).item()
    variance_IS = torch.var(w).item()
    return mean_IS, variance_IS, float(np.sqrt(variance_IS) / mean_IS)


def _is_native(problem, model, K, delta_t, logw_only=False):
    dev = model.device
    lib = nat.load()
    N = int(np.ceil(problem.T / delta_t))
    spec = problem.native_spec()
    keep = []

    def dev_f32(t):
        t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
        keep.append(t)
        return t

    H = model.z_n.native_shape()[1]
    cfg = nat.HjbConfig()
    cfg.K_local, cfg.N = K, N
    cfg.K_global, cfg.k_offset = K, 0
    cfg.dt = float(torch.tensor(delta_t, dtype=torch.float32).item())
    cfg.sqrt_dt = float(torch.tensor(np.sqrt(delta_t), dtype=torch.float32).item())
    cfg.drift_kind = spec['drift'][0]
    cfg.sigma_kind = spec['sigma'][0]
    cfg.sigma_scale = float(spec['sigma'][2])
    cfg.runcost_kind = spec['runcost'][0]
    cfg.term_kind = spec['term'][0]
    cfg.adaptive, cfg.loss_kind, cfg.store_path = 1, nat.LOSS_LOG_VARIANCE, 0
    philox = getattr(model, 'noise', 'reference') == 'philox'
    cfg.noise_mode = nat.NOISE_PHILOX if philox else nat.NOISE_SUPPLIED
    chosen, why = shapes.choose(cfg, model.d, H)       # exact instance or the cheapest larger one (zero padding)
    if chosen is None:
        raise NotImplementedError('native IS evaluation unavailable: ' + why)
    d_pad, H_pad, _, sizes = chosen
    pad = shapes.ParamPad(model.d, H, d_pad, H_pad, dev)
    cfg.drift = nat.ptr(dev_f32(pad.drift_or_sigma(spec['drift'][1]))) if spec['drift'][1] is not None else None
    cfg.sigma = nat.ptr(dev_f32(pad.drift_or_sigma(spec['sigma'][1]))) if spec['sigma'][1] is not None else None
    cfg.runcost = nat.ptr(dev_f32(pad.vec(spec['runcost'][1]))) if spec['runcost'][1] is not None else None
    cfg.term = nat.ptr(dev_f32(pad.vec(spec['term'][1])))
    flat = torch.cat([p.detach().reshape(-1) for p in model.z_n.flat_layout()]).to(dev).contiguous()
    flat = pad.scatter_params(flat, pad.new_padded_params() if not pad.identity else None)
    xi = xi_dev = None
    if not philox:                                   # the reference's draws: N x randn(K, d) (utilities.py:310)
        xi_cpu = torch.zeros(N + 1, K, model.d)
        for n in range(N):
            xi_cpu[n + 1] = torch.randn(K, model.d)
        xi_dev = xi_cpu.to(dev)
        xi = pad.last_dim(xi_dev)
    tfeat = _time_feature_table(model, N, delta_t).to(dev)
    x0 = dev_f32(pad.vec(torch.as_tensor(problem.X_0, dtype=torch.float32).to(dev)))
    D = torch.empty(K, dtype=torch.float32, device=dev)
    Fint = torch.empty(K, dtype=torch.float32, device=dev)
    part = torch.empty(sizes.fwd_partial_bytes // 8, dtype=torch.float64, device=dev)
    model._is_calls = getattr(model, '_is_calls', 0) + 1
    nat.check(lib.psp_hjb_rollout_eval(C.byref(cfg), nat.ptr(flat), nat.ptr(x0), 0, nat.ptr(xi),
                                       (int(model.seed) + 7919) & 0xFFFFFFFFFFFFFFFF, model._is_calls,
                                       nat.ptr(tfeat), nat.ptr(D), nat.ptr(Fint), None, nat.ptr(part),
                                       nat.stream_ptr(dev)), 'psp_hjb_rollout_eval')
    if logw_only:                                    # (log-weights, the unpadded device noise for the uncontrolled rollout)
        return D - 2.0 * Fint, xi_dev
    return _stats(D - 2.0 * Fint)


def _dense_reason(problem, model):
    """None if the learned control is a DenseNet configuration the hjbd forward kernel covers (plan_dense_native.py)."""
    try:
        from .plan_dense_native import dense_eligibility
    except ImportError:
        from plan_dense_native import dense_eligibility
    if getattr(model, 'backend', 'auto') == 'torch':
        return "backend='torch' requested"
    saved = (model.IS_variance_K, model.u_l2_error_flag, model.loss_method, model.detach_forward)
    model.IS_variance_K, model.u_l2_error_flag, model.loss_method, model.detach_forward = 0, False, 'log-variance', True
    try:                                              # (training-only restrictions do not matter for a forward sweep)
        return dense_eligibility(model)
    finally:
        model.IS_variance_K, model.u_l2_error_flag, model.loss_method, model.detach_forward = saved


def _is_dense_native(problem, model, K, delta_t, logw_only=False):
    """The controlled forward sweep of utilities.py:296-330 on the DenseNet-control rollout kernel.  The reference
    evaluates Z_n(X, n delta_t) through solver.py:360-362: step index ceil(t / model.delta_t) -> the time feature
    (inner) or the per-step net (outer); here that index selects the time-feature entry or the parameter set."""
    try:
        from .plan_dense_native import _instance_for, _nets
        from .plan_common import pad_coeff
    except ImportError:
        from plan_dense_native import _instance_for, _nets
        from plan_common import pad_coeff
    dev = model.device
    lib = nat.load()
    N = int(np.ceil(problem.T / delta_t))
    spec = problem.native_spec()
    keep = []

    def dev_f32(t):
        t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
        keep.append(t)
        return t

    nets = _nets(model)
    outer = model.time_approx == 'outer'
    H = nets[0].nn_dims[1]
    d_pad, H_pad = _instance_for(model.d, H)
    pad = shapes.ParamPad(model.d, H, d_pad, H_pad, dev)
    cfg = nat.DnetConfig()
    b = cfg.base
    b.d, b.H, b.K_local, b.N, b.K_global, b.k_offset = d_pad, H_pad, K, N, K, 0
    b.dt = float(torch.tensor(delta_t, dtype=torch.float32).item())
    b.sqrt_dt = float(torch.tensor(np.sqrt(delta_t), dtype=torch.float32).item())
    b.drift_kind, b.sigma_kind, b.sigma_scale = spec['drift'][0], spec['sigma'][0], float(spec['sigma'][2])
    b.runcost_kind, b.term_kind = spec['runcost'][0], spec['term'][0]
    b.coord_split = int(spec.get('split', 0))
    b.adaptive, b.loss_kind, b.store_path = 1, nat.LOSS_LOG_VARIANCE, 0
    philox = getattr(model, 'noise', 'reference') == 'philox'
    b.noise_mode = nat.NOISE_PHILOX if philox else nat.NOISE_SUPPLIED
    b.drift = nat.ptr(dev_f32(pad_coeff(pad, spec['drift'][1]))) if spec['drift'][1] is not None else None
    b.sigma = nat.ptr(dev_f32(pad.drift_or_sigma(spec['sigma'][1]))) if spec['sigma'][1] is not None else None
    b.runcost = nat.ptr(dev_f32(pad.vec(spec['runcost'][1]))) if spec['runcost'][1] is not None else None
    b.term = nat.ptr(dev_f32(pad_coeff(pad, spec['term'][1])))
    cfg.d_real, cfg.H_real = model.d, H
    cfg.time_input, cfg.per_step = (0 if outer else 1), (1 if outer else 0)
    sets = [torch.cat([p.detach().reshape(-1) for p in net.W]).to(dev) for net in nets]
    tfeat = _time_feature_table(model, N, delta_t)
    if outer:                                        # one parameter set per EVALUATION step: the net solver.py:192-193 picks
        dt32 = float(model.delta_t.detach().cpu())
        idx = [max(0, min(int(round(float(t) / dt32)), model.N - 1)) for t in tfeat.tolist()]
        flat = torch.cat([sets[i] for i in idx]).contiguous()
    else:
        flat = sets[0].contiguous()
    sizes = nat.DnetSizes()
    nat.check(lib.psp_dnet_query(C.byref(cfg), C.byref(sizes)), 'psp_dnet_query')
    xi = xi_dev = None
    if not philox:                                   # the reference's draws: N x randn(K, d) (utilities.py:310)
        xi_cpu = torch.zeros(N + 1, K, model.d)
        for n in range(N):
            xi_cpu[n + 1] = torch.randn(K, model.d)
        xi_dev = xi_cpu.to(dev)
        xi = pad.last_dim(xi_dev)
    tfeat = tfeat.to(dev)
    x0 = dev_f32(pad.vec(torch.as_tensor(problem.X_0, dtype=torch.float32).to(dev)))
    D = torch.empty(K, dtype=torch.float32, device=dev)
    Fint = torch.empty(K, dtype=torch.float32, device=dev)
    part = torch.empty(sizes.fwd_partial_bytes // 8, dtype=torch.float64, device=dev)
    tables = torch.empty(sizes.table_bytes // 4, dtype=torch.float32, device=dev)
    model._is_calls = getattr(model, '_is_calls', 0) + 1
    nat.check(lib.psp_dnet_rollout_fwd(C.byref(cfg), nat.ptr(flat), nat.ptr(x0), 0, None, nat.ptr(xi),
                                       (int(model.seed) + 7919) & 0xFFFFFFFFFFFFFFFF, model._is_calls, nat.ptr(tfeat),
                                       None, None, nat.ptr(D), nat.ptr(Fint), None, None, nat.ptr(part),
                                       nat.ptr(tables), nat.stream_ptr(dev)), 'psp_dnet_rollout_fwd')
    if logw_only:
        return D - 2.0 * Fint, xi_dev
    return _stats(D - 2.0 * Fint)


def _affine_is_reason(problem, model, wide=False):
    """None if the learned control is a Linear or Constant list that psp_is_rollout evaluates as u = -Z_n (PSP_ISC_LINEAR /
    PSP_ISC_TABLE; plan_affine_native.is_control_tables), else the reason."""
    try:
        from .plan_affine_native import control_class
        from .function_space import Linear, Constant
    except ImportError:
        from plan_affine_native import control_class
        from function_space import Linear, Constant
    if getattr(model, 'approx_method', 'control') != 'control' or getattr(model, 'time_approx', None) != 'outer':
        return "not a per-step control (approx_method='control', time_approx='outer')"
    cls = control_class(getattr(model, 'z_n', None))
    if cls not in (Linear, Constant):
        return 'the learned control is not a list of Linear or of Constant modules (Affine keeps the composite evaluation)'
    if len(model.z_n) != model.N:
        return 'z_n does not hold one module per time step'
    return _coeff_reason(problem, model, wide)


def _is_affine_native(problem, model, K, delta_t, logw_only=False):
    """The controlled sweep of utilities.py:296-330 for a Linear / Constant list on the reference-control rollout kernel: the
    learned control IS a table of gains / of vectors, u = -Z_idx(n) with idx the step map of solver.py:360-362, 352-353."""
    try:
        from .plan_affine_native import is_control_tables
    except ImportError:
        from plan_affine_native import is_control_tables
    dev = model.device
    N = int(np.ceil(problem.T / delta_t))
    philox = getattr(model, 'noise', 'reference') == 'philox'
    kind, table = is_control_tables(model, N, delta_t)
    cfg, keep = _is_config(problem, model, K, delta_t, nat.ISC_NONE, philox)
    cfg.control_kind = kind
    cfg.u_ref = nat.ptr(table)
    reason = _is_query(cfg)
    if reason is not None:
        raise NotImplementedError('native IS evaluation unavailable: ' + reason)
    xi = None if philox else _ref_noise(N, K, problem.d, dev)
    model._is_calls = getattr(model, '_is_calls', 0) + 1
    logw, _ = _is_rollout(problem, model, K, cfg, xi, model._is_calls, False)
    if logw_only:
        return logw, xi
    return _stats(logw)


def _is_composite(problem, model, K, delta_t):
    dev = model.device
    sq_dt = np.sqrt(delta_t)
    N = int(np.ceil(problem.T / delta_t))
    X_u = torch.as_tensor(problem.X_0, dtype=torch.float32).repeat(K, 1).to(dev)
    ito = torch.zeros(K).to(dev)
    riemann = torch.zeros(K).to(dev)
    f_int_u = torch.zeros(K).to(dev)
    for n in range(N):
        xi = torch.randn(K, problem.d).to(dev)
        with torch.no_grad():
            ut = -model.Z_n(X_u, n * delta_t)
        sig = problem.sigma(X_u)
        X_u = (X_u + (problem.b(X_u) + torch.mm(sig, ut.t()).t()) * delta_t + torch.mm(sig, xi.t()).t() * sq_dt)
        ito = ito + torch.sum(ut * xi, 1) * sq_dt
        riemann = riemann + torch.sum(ut ** 2, 1) * delta_t
        f_int_u = f_int_u + model.f(X_u, n * delta_t) * delta_t
    return _stats(-f_int_u - problem.g(X_u) - ito - 0.5 * riemann)


def do_importance_sampling_me(problem, model, K, control='approx', simulate_naive=False, verbose=False,
                              delta_t=0.01, on_cpu=False, cross_statistics=None, wide_states='torch'):
    """Reference utilities.py:287-359.  Returns (mean_IS, variance_IS, rel_error_IS), preceded by the naive estimator's three
    numbers when ``simulate_naive``.  ``control='true'`` (with model.u_l2_error_flag) evaluates IS under problem.u_true;
    ``cross_statistics`` adds the counts of final states above it to the verbose lines.  ``on_cpu`` is not built.
    ``wide_states``: where the naive rollout, the ``control='true'`` rollout and a Linear / Constant list run above d = 64 --
    'torch' (default) on the composite plan, 'native' on psp_isw_rollout (csrc/hjbew_kernels.h, d <= native.ISW_MAX_D);
    d <= 64 runs on psp_is_rollout under either value."""
    if on_cpu:
        raise NotImplementedError('on_cpu is not built')
    if wide_states not in ('torch', 'native'):
        raise ValueError("wide_states must be 'torch' or 'native'")
    wide = wide_states == 'native'
    if simulate_naive or cross_statistics is not None or (control != 'approx' and model.u_l2_error_flag):
        return _is_estimators(problem, model, K, control, simulate_naive, verbose, delta_t, cross_statistics, wide)
    reason = _native_reason(problem, model, control, simulate_naive)
    if reason is None:
        out = _is_native(problem, model, K, delta_t)
    elif _dense_reason(problem, model) is None:
        out = _is_dense_native(problem, model, K, delta_t)
    elif _affine_is_reason(problem, model, wide) is None and (
            problem.d <= nat.IS_MAX_D or getattr(model, 'backend', 'auto') == 'native' or _affine_wide_ok(problem, model, K, delta_t)):
        out = _is_affine_native(problem, model, K, delta_t)
    else:
        if getattr(model, 'backend', 'auto') == 'native':
            raise NotImplementedError('native IS evaluation unavailable: ' + reason)
        out = _is_composite(problem, model, K, delta_t)
    if verbose:
        print('IS mean: %.4e, IS variance: %.4e, IS RE %.4e' % out)
    return out




# ---- simulate_naive / control='true' / cross_statistics (reference utilities.py:296-337) ----------------------------------------
def _true_control_reason(problem, model, N, delta_t):
    """None if psp_is_rollout can evaluate the problem's u* (include/psp.h PSP_ISC_*), else the reason."""
    try:
        from .plan_dense_native import ul2_kind, ul2_unsupported
    except ImportError:
        from plan_dense_native import ul2_kind, ul2_unsupported
    if ul2_kind(problem) is None:
        return 'the problem has no description of u_true the kernel reads (ul2_kind is None)'
    why = ul2_unsupported(problem, N, delta_t)
    if why is not None:
        return why
    return None                                      # (the LDS budget is psp_is_query's to judge: _is_estimators)


def _coeff_reason(problem, model, wide=False):
    try:
        from .problems import coefficients_overridden
    except ImportError:
        from problems import coefficients_overridden
    if getattr(model, 'backend', 'auto') == 'torch':
        return "backend='torch' requested"
    if not hasattr(problem, 'native_spec') or problem.native_spec() is None:
        return 'the problem has no catalogue description of its coefficients (native_spec)'
    if nat.dnet_only_kind(problem.native_spec()) is not None:
        return nat.dnet_only_kind(problem.native_spec())
    over = coefficients_overridden(problem)
    if over is not None:
        return 'problem.%s is not the catalogue implementation' % over
    if problem.d > nat.IS_MAX_D and not wide:          # (wide: psp_isw_query judges d, with its own message)
        return 'd = %d is outside the native range d <= %d of psp_is_rollout' % (problem.d, nat.IS_MAX_D)
    if model.device.type != 'cuda':
        return 'the model is not on a GPU'
    return None


def _ref_noise(N, K, d, dev):
    """The reference's draws: N x randn(K, d) from the CPU generator (utilities.py:310), slice n + 1 drives step n."""
    xi = torch.zeros(N + 1, K, d)
    for n in range(N):
        xi[n + 1] = torch.randn(K, d)
    return xi.to(dev)


def _is_config(problem, model, K, delta_t, kind, philox):
    """(psp_is_config, the device tensors it points to) for one psp_is_rollout call on the model's device."""
    try:
        from .plan_dense_native import ul2_reference
        from .problems import DoubleWell
    except ImportError:
        from plan_dense_native import ul2_reference
        from problems import DoubleWell
    dev = model.device
    d = problem.d
    N = int(np.ceil(problem.T / delta_t))
    spec = problem.native_spec()
    keep = []

    def dev_t(t, dtype=torch.float32):
        t = torch.as_tensor(t).detach().to(device=dev, dtype=dtype).contiguous()
        keep.append(t)
        return t

    cfg = nat.IsConfig()
    cfg.d, cfg.K_local, cfg.N, cfg.control_kind = d, K, N, kind
    cfg.K_global, cfg.k_offset = K, 0
    cfg.dt = float(torch.tensor(delta_t, dtype=torch.float32).item())
    cfg.sqrt_dt = float(torch.tensor(np.sqrt(delta_t), dtype=torch.float32).item())
    cfg.drift_kind, cfg.sigma_kind, cfg.sigma_scale = spec['drift'][0], spec['sigma'][0], float(spec['sigma'][2])
    cfg.runcost_kind, cfg.term_kind = spec['runcost'][0], spec['term'][0]
    cfg.dwell_form = 1 if isinstance(problem, DoubleWell) else 0        # the two roundings of -grad V (problems.py)
    cfg.noise_mode = nat.NOISE_PHILOX if philox else nat.NOISE_SUPPLIED
    cfg.x0 = nat.ptr(dev_t(torch.as_tensor(problem.X_0, dtype=torch.float32).reshape(-1)))
    cfg.drift = nat.ptr(dev_t(spec['drift'][1])) if spec['drift'][1] is not None else None
    cfg.sigma = nat.ptr(dev_t(spec['sigma'][1])) if spec['sigma'][1] is not None else None
    cfg.runcost = nat.ptr(dev_t(spec['runcost'][1])) if spec['runcost'][1] is not None else None
    cfg.term = nat.ptr(dev_t(spec['term'][1]))
    if kind != nat.ISC_NONE:
        ref = ul2_reference(problem, N, delta_t, d, K, 0)
        if kind == nat.ISC_TABLE:
            cfg.u_ref = nat.ptr(dev_t(ref['table']))
        elif kind == nat.ISC_LINEAR:
            cfg.u_ref = nat.ptr(dev_t(ref['gains']))
        else:
            cfg.u_ref = nat.ptr(dev_t(ref['tables']))
            cfg.u_group = nat.ptr(dev_t(ref['group'], torch.int32))
            cfg.u_row = nat.ptr(dev_t(ref['row'], torch.int32))
            cfg.u_ntables, (cfg.u_nrows, cfg.u_ncols) = ref['tables'].shape[0], ref['tables'].shape[1:]
            cfg.u_xb, cfg.u_dx, cfg.u_xhi = ref['xb'], ref['dx'], ref['xhi']
    return cfg, keep


def _is_query(cfg):
    """None if the rollout accepts the config (the LDS budget included), else its reason: psp_is_rollout up to d = 64,
    psp_isw_rollout above (a config of that size gets here under wide_states='native' only: _coeff_reason)."""
    lib = nat.load()
    if cfg.d > nat.IS_MAX_D:
        if lib.psp_isw_query(C.byref(cfg), C.byref(nat.IswSizes())) != 0:
            return nat.last_error()
        return None
    if lib.psp_is_query(C.byref(cfg), None) != 0:
        return nat.last_error()
    return None


def _affine_wide_ok(problem, model, K, delta_t):
    """backend='auto' above d = 64: whether psp_isw_query takes the Linear / Constant list's config (else the composite plan)."""
    try:
        from .plan_affine_native import is_control_tables
    except ImportError:
        from plan_affine_native import is_control_tables
    kind, table = is_control_tables(model, int(np.ceil(problem.T / delta_t)), delta_t)
    cfg, keep = _is_config(problem, model, K, delta_t, nat.ISC_NONE, False)
    cfg.control_kind, cfg.u_ref = kind, nat.ptr(table)
    return _is_query(cfg) is None


def _is_rollout(problem, model, K, cfg, xi, iter_, want_XN):
    """One psp_is_rollout call (d <= 64) or psp_isw_rollout call (above): (log-weights (K), X_N (K, d) or None) on the model's
    device."""
    dev = model.device
    lib = nat.load()
    d = problem.d
    logw = torch.empty(K, dtype=torch.float32, device=dev)
    XN = torch.empty(K, d, dtype=torch.float32, device=dev) if want_XN else None
    if cfg.d > nat.IS_MAX_D:
        sizes = nat.IswSizes()
        nat.check(lib.psp_isw_query(C.byref(cfg), C.byref(sizes)), 'psp_isw_query')
        tables = torch.empty(max(1, sizes.table_bytes // 4), dtype=torch.float32, device=dev)
        nat.check(lib.psp_isw_rollout(C.byref(cfg), nat.ptr(xi), (int(model.seed) + 7919) & 0xFFFFFFFFFFFFFFFF, iter_, nat.ptr(tables),
                                      nat.ptr(logw), nat.ptr(XN), nat.stream_ptr(dev)), 'psp_isw_rollout')
        return logw, XN
    nat.check(lib.psp_is_rollout(C.byref(cfg), nat.ptr(xi), (int(model.seed) + 7919) & 0xFFFFFFFFFFFFFFFF, iter_, nat.ptr(logw),
                                 nat.ptr(XN), nat.stream_ptr(dev)), 'psp_is_rollout')
    return logw, XN


_KIND_OF_UL2 = {nat.UL2_TABLE: nat.ISC_TABLE, nat.UL2_LINEAR: nat.ISC_LINEAR, nat.UL2_GRID: nat.ISC_GRID}


def _is_composite_full(problem, model, K, control, simulate_naive, delta_t):
    """utilities.py:296-337 restated: the naive and the controlled path on one noise stream, u* on the host for control='true'.
    Returns (naive weights or None, IS weights, X naive or None, X_u)."""
    device = model.device
    sq_delta_t = np.sqrt(delta_t)
    N = int(np.ceil(problem.T / delta_t))
    X = problem.X_0.repeat(K, 1).to(device) if simulate_naive else None
    X_u = problem.X_0.repeat(K, 1).to(device)
    ito_int = torch.zeros(K).to(device)
    riemann_int = torch.zeros(K).to(device)
    f_int = torch.zeros(K).to(model.device)
    f_int_u = torch.zeros(K).to(model.device)
    for n in range(N):
        xi = torch.randn(K, problem.d).to(device)
        if simulate_naive:
            X = (X + problem.b(X) * delta_t + torch.mm(problem.sigma(X), xi.t()).t() * sq_delta_t)
            f_int += model.f(X, n * delta_t) * delta_t
        if control == 'approx' or model.u_l2_error_flag is False:
            with torch.no_grad():
                ut = -model.Z_n(X_u, n * delta_t)
        elif control == 'true':
            ut = torch.tensor(problem.u_true(X_u.cpu(), n * delta_t)).t().float().to(device)
        X_u = (X_u + (problem.b(X_u) + torch.mm(problem.sigma(X_u), ut.t()).t()) * delta_t
               + torch.mm(problem.sigma(X_u), xi.t()).t() * sq_delta_t)
        ito_int += torch.sum(ut * xi, 1) * sq_delta_t
        riemann_int += torch.sum(ut ** 2, 1) * delta_t
        f_int_u += model.f(X_u, n * delta_t) * delta_t
    girsanov = torch.exp(- ito_int - 0.5 * riemann_int)
    w_naive = torch.exp(- f_int - problem.g(X)) if simulate_naive else None
    return w_naive, torch.exp(- f_int_u - problem.g(X_u)) * girsanov, X, X_u


def _weight_stats(w):
    mean = torch.mean(w).item()
    var = torch.var(w).item()
    return mean, var, np.sqrt(var) / mean


def _learned_kernel(problem, model, control):
    """The evaluation kernel of today's path for a learned control (_is_native / _is_dense_native), or a reason."""
    reason = _native_reason(problem, model, control, False)
    if reason is None:
        return _is_native
    if _dense_reason(problem, model) is None:
        return _is_dense_native
    return reason


def _full_reason(problem, model, K, control, simulate_naive, delta_t, cross, wide=False):
    """None if _is_estimators runs natively (psp_is_rollout, next to today's evaluation kernel for a learned control), else the
    reason."""
    why = _coeff_reason(problem, model, wide)
    if why is not None:
        return why
    if control != 'approx' and model.u_l2_error_flag:
        return _true_control_reason(problem, model, int(np.ceil(problem.T / delta_t)), delta_t)
    if cross is not None:
        return 'cross_statistics with the learned control needs the final states of the controlled evaluation rollout'
    kernel = _learned_kernel(problem, model, control)
    return kernel if isinstance(kernel, str) else None


def _is_estimators(problem, model, K, control, simulate_naive, verbose, delta_t, cross, wide=False):
    """simulate_naive / control='true' / cross_statistics: fully native or fully composite (utilities.py:296-359)."""
    try:
        from .plan_dense_native import ul2_kind
    except ImportError:
        from plan_dense_native import ul2_kind
    reason = _full_reason(problem, model, K, control, simulate_naive, delta_t, cross, wide)
    true_control = control != 'approx' and model.u_l2_error_flag
    philox = getattr(model, 'noise', 'reference') == 'philox'
    cfgs = {}
    if reason is None:                                   # the library's own checks (LDS budget of the u* data) before any draw
        kinds = ([nat.ISC_NONE] if simulate_naive else []) + ([_KIND_OF_UL2[ul2_kind(problem)]] if true_control else [])
        for kind in kinds:
            cfgs[kind] = _is_config(problem, model, K, delta_t, kind, philox)
            reason = reason or _is_query(cfgs[kind][0])
    X = X_u = None
    if reason is None:
        N = int(np.ceil(problem.T / delta_t))
        want = cross is not None
        if true_control:                                               # u* on the device, naive and IS on one noise stream
            xi = None if philox else _ref_noise(N, K, problem.d, model.device)
            model._is_calls = getattr(model, '_is_calls', 0) + 1
            if simulate_naive:
                lw_naive, X = _is_rollout(problem, model, K, cfgs[nat.ISC_NONE][0], xi, model._is_calls, want)
            kind = _KIND_OF_UL2[ul2_kind(problem)]
            lw, X_u = _is_rollout(problem, model, K, cfgs[kind][0], xi, model._is_calls, want)
        else:                                                          # learned control: IS on today's kernel, unchanged
            lw, xi = _learned_kernel(problem, model, control)(problem, model, K, delta_t, logw_only=True)   # counts the call
            lw_naive, _ = _is_rollout(problem, model, K, cfgs[nat.ISC_NONE][0], xi, model._is_calls, False)   # same noise
        w_naive = torch.exp(lw_naive) if simulate_naive else None
        w_is = torch.exp(lw)
    else:
        if getattr(model, 'backend', 'auto') == 'native':
            raise NotImplementedError('native IS evaluation unavailable: ' + reason)
        w_naive, w_is, X, X_u = _is_composite_full(problem, model, K, control, simulate_naive, delta_t)
    naive = _weight_stats(w_naive) if simulate_naive else None
    out = _weight_stats(w_is)
    if verbose is True:
        string = ''
        if simulate_naive:
            string += 'naive mean: %.4e, naive variance: %.4e, naive RE %.4e' % naive
            if cross is not None:
                string += ', crossed: %d/%d' % (torch.sum(X > torch.as_tensor(cross).to(X.device)), X.shape[0])
            string += '\n'
        string += 'IS mean: %.4e, IS variance: %.4e, IS RE %.4e' % out
        if cross is not None:
            string += ', crossed: %d/%d' % (torch.sum(X_u > torch.as_tensor(cross).to(X_u.device)), X_u.shape[0])
        print(string)
    return (naive + out) if simulate_naive else out


def compute_test_error(model, problem, K, device=None, modus='elliptic'):
    """Monte-Carlo error of the value net against ``problem.v_true`` on K fresh points of the domain -- the ``K_test_log``
    diagnostic of EllipticSolver / GeneralSolver (reference utilities.py:440-472; draws from the CPU generator in that order:
    randn(K, d) and rand(K) for the ball-shaped domains, rand(K, d) for the boxes, then rand(K, 1) for the times).
    Returns (L2 error, mean absolute error, mean relative error)."""
    device = torch.device(device) if device is not None else model.device
    d = problem.d
    if problem.boundary in ('sphere', 'unbounded', 'two_spheres'):
        R = problem.boundary_distance_2 if problem.boundary == 'two_spheres' else problem.boundary_distance
        X = torch.randn(K, d).to(device)
        X = R * X / torch.sqrt(torch.sum(X ** 2, 1)).unsqueeze(1) * (torch.rand(K).unsqueeze(1) ** (1 / d)).to(device)
        if problem.boundary == 'two_spheres':
            X = X[torch.sqrt(torch.sum(X ** 2, 1)) > problem.boundary_distance_1, :]
    else:
        X = (problem.X_r - problem.X_l) * torch.rand(K, d).to(device) + problem.X_l
    with torch.no_grad():
        if modus == 'parabolic':
            t_n = torch.rand(K, 1).to(device) * problem.T
            v_true = np.asarray(torch.as_tensor(problem.v_true(X.detach().cpu(), t_n.cpu().squeeze())).squeeze())
            v_est = model.V(torch.cat([X, t_n], 1)).squeeze().cpu().numpy()
        else:
            v_true = np.asarray(torch.as_tensor(problem.v_true(X.detach().cpu())).squeeze())
            v_est = model.V(X).squeeze().cpu().numpy()
    diff = v_true - v_est
    return float(np.mean(diff ** 2)), float(np.mean(np.abs(diff))), float(np.mean(np.abs(diff) / v_true))


def compute_test_error_native(model, problem, K, modus='elliptic', seed=None, iteration=0, return_points=False):
    """``compute_test_error`` on the device (psp_genl_test_error, csrc/genl_eval_kernels.h): the K points are drawn from the
    sampler's own Philox stream (seed, iteration), V and the problem's closed-form v_true are evaluated and the statistics
    reduced by two kernels.  Serves every value net ``plan_general_deep.value_net_spec`` accepts -- the two-layer and the deep
    plan's nets alike.  Returns (L2 error, mean absolute error, mean relative error) like compute_test_error; with
    ``return_points`` a fourth entry, a dict of the per-point device tensors x (K, d), t, v, v_true (K) and keep (K, bool: False
    for the points 'two_spheres' rejects).  ``seed`` defaults to ``model.seed``.
    NotImplementedError with the reason when the net, the domain or the problem is not covered."""
    try:
        from . import device_test_log as dtl
        from . import kernel_config as kc
        from .plan_general_deep import value_net_spec
    except ImportError:
        import device_test_log as dtl
        import kernel_config as kc
        from plan_general_deep import value_net_spec
    if modus not in ('elliptic', 'parabolic'):
        raise ValueError("modus must be 'elliptic' or 'parabolic'")
    why = dtl.eval_reason(problem)
    if why is not None:
        raise NotImplementedError('native test error unavailable: ' + why)
    d = problem.d
    net = value_net_spec(model.V, d + (1 if modus == 'parabolic' else 0))
    if isinstance(net, str):
        raise NotImplementedError('native test error unavailable: ' + net)
    layers = kc.value_net_limits_reason(net['dims'])[0]
    if layers is not None:
        raise NotImplementedError('native test error unavailable: ' + layers)
    sizes, why = dtl.eval_query(dtl.eval_config(net, problem, K, modus))
    if sizes is None:
        raise NotImplementedError('native test error unavailable: ' + why)
    dev = net['params'][0].device
    if dev.type != 'cuda':
        raise NotImplementedError('native test error unavailable: the value net lives on %s (the HIP kernels need a GPU)' % dev)
    log = dtl.DeviceTestLog(net, problem, K, modus, dev)
    flat = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in net['params']]).contiguous()
    dumps = None
    if return_points:
        f32 = dict(dtype=torch.float32, device=dev)
        dumps = {'x': torch.zeros(K, d, **f32), 't': torch.zeros(K, **f32), 'v': torch.zeros(K, **f32),
                 'v_true': torch.zeros(K, **f32), 'keep': torch.zeros(K, dtype=torch.int32, device=dev)}
    log.enqueue(flat, model.seed if seed is None else seed, iteration, 0, nat.stream_ptr(dev), dumps)
    l2, mae, mre = (v[0] for v in log.read())
    if return_points:
        dumps['keep'] = dumps['keep'].bool()
        return l2, mae, mre, dumps
    return l2, mae, mre


# ---- relative errors of the loss estimators (reference `Compare relative errors of losses.ipynb`, third cell) --------------------
LRE_TILE = 16                                  # the forward kernels' trajectory tile: chunks are whole tiles
LRE_NATIVE_CHUNK = 1 << 20                     # default chunk of the native plan: two 4 MiB buffers
LRE_TORCH_CHUNK = 1 << 16                      # ... of the composite plan, which holds (chunk, d) tensors per step
LRE_MAX_SAMPLES = 1 << 24                      # return_samples keeps two K-sized fp32 buffers
LRE_REFERENCE_NOISE_LIMIT = 1 << 28            # noise='reference' holds K * N * d floats on the host (1 GiB)
LRE_PHILOX_FILL_FLOATS = 1 << 27               # the composite plan's materialised Philox stream per chunk on a GPU
LRE_KEYS = ('terminal', 'cross_entropy', 'cross_entropy_detach', 'cross_entropy_detach_selection', 'log_variance', 'moment')
LRE_SELECT = 100.0


def lre_chunk(K, chunk, default):
    """The chunk the rollout runs in: `chunk` (None: `default`) rounded up to whole tiles, at most K rounded up."""
    c = int(default if chunk is None else chunk)
    if c < 1:
        raise ValueError('chunk must be positive')
    up = lambda v: -(-int(v) // LRE_TILE) * LRE_TILE
    return min(up(c), up(K))


def _lre_merge(a, b):
    """(n, mean, M2, M3, M4) of two sample sets -> of their union (Chan et al. / Pebay), numpy float64 scalars."""
    na, ma, M2a, M3a, M4a = a
    nb, mb, M2b, M3b, M4b = b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = na + nb
    dl = mb - ma
    mean = ma + dl * (nb / n) if np.isfinite(dl) else (na * ma + nb * mb) / n      # an infinite mean stays infinite
    return (n, mean, M2a + M2b + dl * dl * (na * nb / n),
            M3a + M3b + dl ** 3 * (na * nb * (na - nb) / (n * n)) + 3.0 * dl * (na * M2b - nb * M2a) / n,
            M4a + M4b + dl ** 4 * (na * nb * (na * na - na * nb + nb * nb) / (n ** 3))
            + 6.0 * dl * dl * (na * na * M2b + nb * nb * M2a) / (n * n) + 4.0 * dl * (na * M3b - nb * M3a) / n)


class _HostLossStats:
    """The statistics of psp_loss_stats_* in float64 torch on the host: the composite plan where there is no GPU."""

    def __init__(self):
        zero = tuple(np.float64(0.0) for _ in range(5))
        self.acc = [zero] * 6                    # terminal, CE, CE detached, its selection, moment, D

    @staticmethod
    def _moments(v):
        n = v.numel()
        if n == 0:
            return tuple(np.float64(0.0) for _ in range(5))
        m = v.mean()
        c = v - m
        e = c.sum() / n
        c = c - (e if torch.isfinite(e) else 0.0)
        e = e if torch.isfinite(e) else torch.zeros(())
        c2 = c * c
        return tuple(np.float64(x) for x in (n, (m + e).item(), c2.sum().item(), (c2 * c).sum().item(), (c2 * c2).sum().item()))

    def accumulate(self, Y, D):
        y, d = Y.detach().cpu().double(), D.detach().cpu().double()
        g = y - d
        ced = y * torch.exp(-g + y)
        samples = (torch.exp(-g), y * torch.exp(-g), ced, ced[ced.abs() < LRE_SELECT], d * d, d)
        with np.errstate(all='ignore'):
            self.acc = [_lre_merge(a, self._moments(v)) for a, v in zip(self.acc, samples)]

    def finish(self):
        out = np.full(20, np.nan)
        with np.errstate(all='ignore'):
            for slot, a in zip((0, 1, 2, 3, 5), self.acc[:5]):
                mean = a[1] if a[0] > 0 else np.float64(np.nan)
                var = a[2] / (a[0] - 1.0)
                out[3 * slot:3 * slot + 3] = mean, var, np.sqrt(var) / abs(mean)
            n, _, M2, _, M4 = self.acc[5]
            var = M2 / (n - 1.0)
            vv = M4 / n - var * var
            out[12:15] = var, vv, np.sqrt(vv) / abs(var)
            out[18], out[19] = self.acc[3][0], n
        return out


class _DeviceLossStats:
    """psp_loss_stats_accumulate / psp_loss_stats_finish (csrc/lstat_kernels.h) on a device-resident state."""

    def __init__(self, dev):
        self.lib, self.dev = nat.load(), dev
        self.state = torch.zeros(self.lib.psp_loss_stats_state_bytes() // 8, dtype=torch.float64, device=dev)

    def accumulate(self, Y, D):
        nat.check(self.lib.psp_loss_stats_accumulate(nat.ptr(Y), nat.ptr(D), Y.numel(), nat.ptr(self.state),
                                                     nat.stream_ptr(self.dev)), 'psp_loss_stats_accumulate')

    def finish(self):
        out = torch.empty(20, dtype=torch.float64, device=self.dev)
        nat.check(self.lib.psp_loss_stats_finish(nat.ptr(self.state), nat.ptr(out), nat.stream_ptr(self.dev)),
                  'psp_loss_stats_finish')
        return out.cpu().numpy()                 # the one read-back of the call


def _lre_control(control, N):
    """(z_n, time_approx) of a bare net, a list of per-step nets or a Solver."""
    if hasattr(control, 'z_n') and hasattr(control, 'time_approx'):
        if getattr(control, 'approx_method', 'control') != 'control':
            raise ValueError("a Solver's control is read from z_n: approx_method must be 'control'")
        z, ta = control.z_n, control.time_approx
    elif isinstance(control, (list, tuple, torch.nn.ModuleList)):
        z, ta = list(control), 'outer'
    elif callable(control):
        z, ta = control, 'inner'
    else:
        raise TypeError('control must be a net of (t, x), a list of per-step nets of x or a Solver')
    if ta == 'outer':
        z = list(z)
        if len(z) != N:
            raise ValueError('a per-step control needs one net per time step: N = floor(T / delta_t) = %d, got %d' % (N, len(z)))
    return z, ta


def _lre_plan(problem, view):
    """(kernel family 'dnet' / 'hjb', None) or (None, the reason for the composite plan)."""
    try:
        from .function_space import DenseNet, MySequential
    except ImportError:
        from function_space import DenseNet, MySequential
    if view.backend == 'torch':
        return None, "backend='torch' requested"
    first = view.z_n[0] if view.time_approx == 'outer' else view.z_n
    if not isinstance(first, (DenseNet, MySequential)) or (isinstance(first, MySequential) and view.time_approx != 'inner'):
        return None, ('the control is a user net (the forward kernels take a DenseNet(d + 1 -> d), a list of N DenseNet(d -> d) or '
                      'a MySequential(d + 1 -> d))')
    if getattr(problem, 'native_spec', None) is None or problem.native_spec() is None:
        return None, (getattr(problem, 'native_plan_reason', None)
                      or 'the problem has no native_spec() (coefficients outside the native catalogue)')
    if isinstance(first, DenseNet):
        nets = view.z_n if view.time_approx == 'outer' else [view.z_n]
        if any(n.activation != 'relu2' or n.output_relu for n in nets):
            return None, 'the DenseNet-control kernels take the relu(.)**2 net without an output ReLU'
        why = _dense_reason(problem, view)
        return ('dnet', None) if why is None else (None, why)
    why = _native_reason(problem, view, 'approx', False)
    return ('hjb', None) if why is None else (None, why)


def _lre_base(b, problem, pad, keep, K, N, delta_t, adaptive, philox, dev):
    """The psp_hjb_config fields both kernel families share for a forward-only chunked rollout."""
    try:
        from .plan_common import pad_coeff
    except ImportError:
        from plan_common import pad_coeff
    spec = problem.native_spec()

    def dev_f32(t):
        t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
        keep.append(t)
        return t

    b.N, b.K_global = N, K
    b.dt = float(torch.tensor(delta_t, dtype=torch.float32).item())
    b.sqrt_dt = float(torch.sqrt(torch.tensor(delta_t, dtype=torch.float32)).item())
    b.drift_kind, b.sigma_kind, b.sigma_scale = spec['drift'][0], spec['sigma'][0], float(spec['sigma'][2])
    b.runcost_kind, b.term_kind = spec['runcost'][0], spec['term'][0]
    b.coord_split = int(spec.get('split', 0))
    b.adaptive, b.loss_kind, b.store_path = (1 if adaptive else 0), nat.LOSS_LOG_VARIANCE, 0
    b.noise_mode = nat.NOISE_PHILOX if philox else nat.NOISE_SUPPLIED
    b.drift = nat.ptr(dev_f32(pad_coeff(pad, spec['drift'][1]))) if spec['drift'][1] is not None else None
    b.sigma = nat.ptr(dev_f32(pad.drift_or_sigma(spec['sigma'][1]))) if spec['sigma'][1] is not None else None
    b.runcost = nat.ptr(dev_f32(pad.vec(spec['runcost'][1]))) if spec['runcost'][1] is not None else None
    b.term = nat.ptr(dev_f32(pad_coeff(pad, spec['term'][1])))
    return dev_f32(pad.vec(torch.as_tensor(problem.X_0, dtype=torch.float32).reshape(-1).to(dev)))


def _lre_chunks(K, chunk):
    return [(k0, min(chunk, K - k0)) for k0 in range(0, K, chunk)]


def _lre_xi_chunk(xi_all, k0, kc, pad, dev):
    """The kernels' (N + 1, kc, d_pad) layout of the host draws (N, K, d): slice n + 1 drives step n."""
    N, _, d = xi_all.shape
    xi = torch.zeros(N + 1, kc, pad.dp, dtype=torch.float32, device=dev)
    xi[1:, :, :d] = xi_all[:, k0:k0 + kc].to(dev)
    return xi


def _lre_native(family, problem, view, K, N, delta_t, chunk, philox, seed, xi_all, sink):
    """K trajectories in chunks on psp_dnet_rollout_fwd / psp_hjb_rollout_fwd, forward only (store_path = 0): k_offset is the
    chunk's first global trajectory and (seed, iter = 0) is the same for every chunk, so a trajectory's Philox noise does not
    depend on the chunking.  `sink(Y, D)` takes the two chunk buffers on the stream; nothing is read back here."""
    try:
        from .plan_dense_native import _instance_for
        from .plan_native import chunk_scratch_sizes
    except ImportError:
        from plan_dense_native import _instance_for
        from plan_native import chunk_scratch_sizes
    dev, lib, d = view.device, nat.load(), problem.d
    keep = []
    chunks = _lre_chunks(K, chunk)
    sizes_k = sorted({kc for _, kc in chunks})
    seed64 = int(seed or 0) & 0xFFFFFFFFFFFFFFFF          # (unused under supplied noise, where seed may be None)
    Yb = torch.empty(chunk, dtype=torch.float32, device=dev)
    Db = torch.empty(chunk, dtype=torch.float32, device=dev)
    stream = nat.stream_ptr(dev)
    if family == 'dnet':
        outer = view.time_approx == 'outer'
        nets = view.z_n if outer else [view.z_n]
        H = nets[0].nn_dims[1]
        d_pad, H_pad = _instance_for(d, H)
        pad = shapes.ParamPad(d, H, d_pad, H_pad, dev)
        cfg = nat.DnetConfig()
        b = cfg.base
        b.d, b.H = d_pad, H_pad
        x0 = _lre_base(b, problem, pad, keep, K, N, delta_t, view.adaptive_forward_process, philox, dev)
        cfg.d_real, cfg.H_real = d, H
        cfg.time_input, cfg.per_step = (0 if outer else 1), (1 if outer else 0)
        flat = torch.cat([p.detach().reshape(-1) for net in nets for p in net.W]).to(device=dev, dtype=torch.float32).contiguous()
        sizes = nat.DnetSizes()
        b.K_local = sizes_k[-1]
        nat.check(lib.psp_dnet_query(C.byref(cfg), C.byref(sizes)), 'psp_dnet_query')
        part = torch.empty(sizes.fwd_partial_bytes // 8, dtype=torch.float64, device=dev)
        tables = torch.empty(sizes.table_bytes // 4, dtype=torch.float32, device=dev)
        for k0, kc in chunks:
            b.K_local, b.k_offset = kc, k0
            xi = None if philox else _lre_xi_chunk(xi_all, k0, kc, pad, dev)
            nat.check(lib.psp_dnet_rollout_fwd(C.byref(cfg), nat.ptr(flat), nat.ptr(x0), 0, None, nat.ptr(xi), seed64, 0, None,
                                               None, None, nat.ptr(Db), None, None, nat.ptr(Yb), nat.ptr(part), nat.ptr(tables),
                                               stream), 'psp_dnet_rollout_fwd')
            sink(Yb[:kc], Db[:kc])
        return
    net = view.z_n
    H = net.native_shape()[1]
    cfg = nat.HjbConfig()
    cfg.K_local = sizes_k[-1]
    pad0 = shapes.ParamPad(d, H, d, H, dev)                           # (the coefficient kinds first: choose() reads them)
    _lre_base(cfg, problem, pad0, [], K, N, delta_t, view.adaptive_forward_process, philox, dev)
    chosen, why = shapes.choose(cfg, d, H)
    if chosen is None:
        raise NotImplementedError('native loss_relative_errors unavailable: ' + why)
    d_pad, H_pad = chosen[0], chosen[1]
    pad = shapes.ParamPad(d, H, d_pad, H_pad, dev)
    x0 = _lre_base(cfg, problem, pad, keep, K, N, delta_t, view.adaptive_forward_process, philox, dev)
    sizes = chunk_scratch_sizes(cfg, sizes_k)
    flat = torch.cat([p.detach().reshape(-1) for p in net.flat_layout()]).to(device=dev, dtype=torch.float32).contiguous()
    flat = pad.scatter_params(flat, pad.new_padded_params() if not pad.identity else None)
    part = torch.empty(max(sizes.fwd_partial_bytes // 8, 2), dtype=torch.float64, device=dev)
    for k0, kc in chunks:
        cfg.K_local, cfg.k_offset = kc, k0
        xi = None if philox else _lre_xi_chunk(xi_all, k0, kc, pad, dev)
        nat.check(lib.psp_hjb_rollout_fwd(C.byref(cfg), nat.ptr(flat), nat.ptr(x0), 0, None, nat.ptr(xi), seed64, 0, None,
                                          nat.ptr(Db), None, nat.ptr(Yb), nat.ptr(part), stream), 'psp_hjb_rollout_fwd')
        sink(Yb[:kc], Db[:kc])


def _lre_torch(problem, view, K, N, delta_t, chunk, philox, seed, xi_all, sink):
    """The notebook's loop in fp32 torch on view.device, chunk by chunk.  Noise: the host draws (`xi_all`), or under 'philox' the
    kernels' own stream materialised by psp_philox_normal_fill on a GPU -- the same noise as the native plan -- and a
    torch.Generator seeded with `seed` where there is none (that stream depends on the chunking)."""
    dev, d = view.device, problem.d
    dt = torch.tensor(delta_t).to(dev)
    sq = torch.sqrt(dt).to(dev)
    X_0 = torch.as_tensor(problem.X_0, dtype=torch.float32).to(dev)
    outer = view.time_approx == 'outer'
    on_gpu = dev.type == 'cuda'
    gen = None
    if philox and on_gpu:
        chunk = min(chunk, max(LRE_TILE, LRE_PHILOX_FILL_FLOATS // ((N + 1) * d) // LRE_TILE * LRE_TILE))
    elif philox:
        gen = torch.Generator().manual_seed(int(seed))
    for k0, kc in _lre_chunks(K, chunk):
        if philox and on_gpu:
            fill = torch.empty(N + 1, kc, d, dtype=torch.float32, device=dev)
            nat.check(nat.load().psp_philox_normal_fill(nat.ptr(fill), N, kc, d, k0, int(seed) & 0xFFFFFFFFFFFFFFFF, 0,
                                                        nat.stream_ptr(dev)), 'psp_philox_normal_fill')
        X = X_0.repeat(kc, 1)
        Y = torch.zeros(kc).to(dev)
        with torch.no_grad():
            for n in range(N):
                if not philox:
                    xi = xi_all[n, k0:k0 + kc].to(dev)
                else:
                    xi = fill[n + 1] if on_gpu else torch.randn(kc, d, generator=gen)
                if outer:
                    Z = view.z_n[n](X)
                else:
                    Z = view.z_n(torch.cat([torch.ones([kc, 1]).to(dev) * n * dt, X], 1))
                c = -Z.t() if view.adaptive_forward_process else torch.zeros(d, 1).to(dev)
                sig = problem.sigma(X)
                X = (X + (problem.b(X) + torch.mm(sig, c).t()) * dt + torch.mm(sig, xi.t()).t() * sq)
                Y = (Y + (-problem.h(dt * n, X, Y, Z) + torch.sum(Z * c.t(), 1)) * dt + torch.sum(Z * xi, 1) * sq)
            D = Y - problem.g(X)
        sink(Y.contiguous(), D.contiguous())


def loss_relative_errors(problem, control, K, delta_t=0.005, adaptive_forward_process=False, noise='philox', seed=0, device=None,
                         backend='auto', chunk=None, return_samples=False):
    """Relative errors of the loss estimators over K forward-only trajectories of one control: the third cell of the reference's
    `experiments/HJB-log-variance-loss/Compare relative errors of losses.ipynb` (K = 5e7, N = 200, d <= 15 there).

    ``control``: a bare DenseNet(d + 1 -> d) (the notebook's net; the time input is column 0), a bare MySequential(d + 1 -> d),
    a list of N DenseNet(d -> d), or a Solver (its ``z_n`` and ``time_approx`` are used); any other callable of [t, x] (or list of
    callables of x) runs on the composite plan.  Per step n < N = floor(T / delta_t), from X_0 = problem.X_0 and Y_0 = 0:
        Z = control(t_n, X_n) with the time feature ones * n * delta_t in fp32;   c = -Z if adaptive_forward_process else 0
        X_{n+1} = X_n + (b(X_n) + sigma c) dt + sigma xi sqrt(dt)
        Y      += (-h(t_n, X_{n+1}, Y, Z) + Z . c) dt + Z . xi sqrt(dt)         (-h = |Z|^2 / 2 + f in this project's sign)
    With D = Y_N - g(X_N) the result holds, per estimator, the tuple (mean, variance, relative_error) of the samples
        'terminal' exp(-g)     'cross_entropy' Y exp(-g)     'cross_entropy_detach' Y exp(-g + Y)
        'cross_entropy_detach_selection' the same over the samples with |v| < 100, with their count as a fourth entry
        'moment' D^2           'log_variance': mean = var(D), variance = mean((D - mean D)^4) - var(D)^2
    relative_error = sqrt(variance) / |mean|; variances are unbiased as torch.var's.  (For the selection the notebook records
    sqrt(variance) and |mean| themselves.)  Also 'K', 'N', 'plan' ('native' or 'torch') and 'plan_reason'; with
    ``return_samples`` (K <= 2**24) the per-trajectory fp32 'Y' and 'D'.

    DELIBERATE DIFFERENCE FROM THE NOTEBOOK: every sum is formed in float64 (psp_loss_stats_* on a GPU; g = Y - D, the
    exponentials and the moments in double), where the notebook reduces fp32 tensors with torch.  Non-finite samples are not
    filtered: they make what they enter NaN.

    Plans.  backend='auto' on a GPU runs the K trajectories in chunks on the forward kernels (psp_dnet_rollout_fwd for DenseNets,
    psp_hjb_rollout_fwd for a MySequential; store_path = 0) when the problem has a ``native_spec()``; each chunk is reduced on
    the device and only the final statistics are read back.  Everything else -- no GPU, a user net, a problem outside the
    catalogue, backend='torch' -- runs the same update in fp32 torch with the same chunking and says why in 'plan_reason';
    backend='native' raises instead.  ``chunk`` (default 2**20 native, 2**16 composite) is rounded up to the kernels' tile of 16
    trajectories.
    noise='philox': the kernels' counter-based stream keyed by (seed, global trajectory index): a trajectory's noise does not
    depend on the chunking (the DenseNet kernel's samples are then bit-identical; psp_hjb_rollout_fwd picks among three forward
    variants by chunk size, which agree to summation order).  noise='reference': the notebook's draws, randn(K, d) per step from the CPU generator after
    torch.manual_seed(seed) (seed=None: the generator continues from where it stands, as in the notebook after the net was
    built); they are held on the host, so K * N * d is limited to 2**28."""
    from types import SimpleNamespace
    if backend not in ('auto', 'native', 'torch'):
        raise ValueError("backend must be 'auto', 'native' or 'torch'")
    if noise not in ('philox', 'reference'):
        raise ValueError("noise must be 'philox' or 'reference'")
    K = int(K)
    if K < 1:
        raise ValueError('K must be positive')
    if not delta_t > 0:
        raise ValueError('delta_t must be positive')
    N = int(np.floor(problem.T / delta_t))
    if N < 1:
        raise ValueError('delta_t = %g leaves no time step in T = %g' % (delta_t, problem.T))
    if return_samples and K > LRE_MAX_SAMPLES:
        raise ValueError('return_samples keeps two K-sized buffers and is limited to K <= 2**24 = %d (K = %d)' % (LRE_MAX_SAMPLES, K))
    d = problem.d
    philox = noise == 'philox'
    if philox and seed is None:
        raise ValueError("noise='philox' needs an integer seed")
    if not philox and K * N * d > LRE_REFERENCE_NOISE_LIMIT:
        raise ValueError("noise='reference' holds the K * N * d = %d draws on the host; the limit is 2**28 = %d -- use "
                         "noise='philox'" % (K * N * d, LRE_REFERENCE_NOISE_LIMIT))
    z, ta = _lre_control(control, N)
    if device is None:
        device = getattr(control, 'device', None) or getattr(problem, 'device', None) or 'cpu'
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    view = SimpleNamespace(device=dev, approx_method='control', loss_method='log-variance', time_approx=ta, z_n=z, d=d,
                           adaptive_forward_process=bool(adaptive_forward_process), detach_forward=True, burgers_drift=False,
                           log_gradient=False, metastability_logs=None, u_l2_error_flag=False, compute_gradient_variance=0,
                           IS_variance_K=0, problem=problem, N=N, delta_t_np=delta_t, backend=backend, K=K, seed=seed)
    family, reason = _lre_plan(problem, view)
    if family is None and backend == 'native':
        raise NotImplementedError('native loss_relative_errors unavailable: ' + reason)
    chunk = lre_chunk(K, chunk, LRE_NATIVE_CHUNK if family is not None else LRE_TORCH_CHUNK)
    xi_all = None
    if not philox:
        if seed is not None:
            torch.manual_seed(int(seed))
        xi_all = torch.empty(N, K, d)
        for n in range(N):
            xi_all[n] = torch.randn(K, d)
    stats = _DeviceLossStats(dev) if dev.type == 'cuda' else _HostLossStats()
    samples = [torch.empty(K, dtype=torch.float32, device=dev) for _ in range(2)] if return_samples else None
    filled = [0]

    def sink(Y, D):
        stats.accumulate(Y, D)
        if samples is not None:
            samples[0][filled[0]:filled[0] + Y.numel()].copy_(Y)
            samples[1][filled[0]:filled[0] + D.numel()].copy_(D)
        filled[0] += Y.numel()

    run = _lre_torch if family is None else (lambda *a: _lre_native(family, *a))
    run(problem, view, K, N, delta_t, chunk, philox, seed, xi_all, sink)
    res = stats.finish()
    assert filled[0] == K and int(res[19]) == K, (filled[0], res[19], K)
    out = {}
    for i, key in enumerate(LRE_KEYS):
        out[key] = tuple(float(v) for v in res[3 * i:3 * i + 3])
    out['cross_entropy_detach_selection'] += (int(res[18]),)
    out.update(K=K, N=N, chunk=chunk, plan='torch' if family is None else 'native', plan_reason=reason)
    if samples is not None:
        out['Y'], out['D'] = samples
    return out
