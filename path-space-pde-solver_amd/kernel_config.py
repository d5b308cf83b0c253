"""A catalogue problem and its value net, described to the kernels once: how ``general_native_spec()`` and
``plan_general_deep.value_net_spec`` become fields of psp_gen_config / psp_genl_config / psp_pinn_config / psp_genl_eval_config
(include/psp.h).  Plain functions that the value-net plans call from their constructors AND from their ``*_eligibility`` probes, so
that a probe asks the library about the configuration the plan will build.  A new kind or config field is added here, once."""
import torch

try:
    from . import native as nat
except ImportError:
    import native as nat

ACT = {'relu2': nat.ACT_RELU2, 'tanh2': nat.ACT_TANH2, 'tanh': nat.ACT_TANH}


def catalogue_spec(problem, names=None):
    """(general_native_spec(), None), or (None, why the problem's coefficients are not the catalogue's).  names: the coefficient
    methods that must be the catalogue implementations (default: problems.coefficients_overridden's)."""
    spec_fn = getattr(problem, 'general_native_spec', None)
    if spec_fn is None:
        return None, 'problem has no general_native_spec() (coefficients outside the native catalogue)'
    try:
        from .problems import coefficients_overridden
    except ImportError:
        from problems import coefficients_overridden
    over = coefficients_overridden(problem) if names is None else coefficients_overridden(problem, names=names)
    if over is not None:
        return None, 'problem.%s is not the catalogue implementation general_native_spec() describes' % over
    return spec_fn(), None


def set_domain(cfg, pb, elliptic):
    """psp_gen_config.domain_kind / dom_a / dom_b from the problem's ``boundary`` (include/psp.h PSP_DOM_*)."""
    if pb.boundary == 'sphere':
        cfg.domain_kind, cfg.dom_a = nat.DOM_SPHERE, float(pb.boundary_distance)
    elif pb.boundary == 'two_spheres':                            # solver.py:1122-1123 / :752-753
        cfg.domain_kind, cfg.dom_a, cfg.dom_b = nat.DOM_ANNULUS, float(pb.boundary_distance_1), float(pb.boundary_distance_2)
    elif pb.boundary == 'square':
        cfg.dom_a, cfg.dom_b = float(pb.X_l), float(pb.X_r)
        cfg.domain_kind = nat.DOM_BOX if not pb.one_boundary else \
            (nat.DOM_BOX_UPPER_ALL if elliptic else nat.DOM_BOX_UPPER_ANY)
    elif pb.boundary == 'square-corner':                          # solver.py:759-760: any(X_proposal <= X_r)
        cfg.domain_kind, cfg.dom_a, cfg.dom_b = nat.DOM_BOX_UPPER_ANY, float(pb.X_l), float(pb.X_r)


def fill_run(base, solver, K_local, k_offset, noise):
    """The discretisation of one launch in a nat.GenConfig: this rank's batch, the step, the noise source."""
    base.K_local, base.N, base.k_offset = K_local, solver.N, k_offset
    base.dt, base.sqrt_dt = float(solver.delta_t.item()), float(solver.sq_delta_t.item())
    base.adaptive = 1 if solver.adaptive_forward_process else 0
    base.noise_mode = nat.NOISE_PHILOX if noise == 'philox' else nat.NOISE_SUPPLIED
    base.store_path = 1


def fill_kinds(cfg, spec):
    """What nat.GenConfig and nat.PinnConfig share: drift_kind, h_kind, h_par and the sigma_scale of a scaled identity (a dense
    sigma: plan_general_native.set_sigma / plan_pinn_native.pinn_config)."""
    cfg.drift_kind, cfg.h_kind = spec['drift'][0], spec['h']
    for i, v in enumerate(spec.get('h_par', ())):
        cfg.h_par[i] = float(v)
    if spec.get('sigma') is None:
        cfg.sigma_scale = float(spec['sigma_scale'])


def fill_problem(base, solver, spec, elliptic, K_local, k_offset, noise):
    """Everything a nat.GenConfig (a psp_gen_config itself, or psp_genl_config.base) says about a GeneralSolver / EllipticSolver
    and its catalogue problem, except ``d`` (a padded width on the templated kernels) and the pointers: nothing is uploaded."""
    fill_run(base, solver, K_local, k_offset, noise)
    base.d_real = solver.d
    base.T = float('inf') if elliptic else float(torch.tensor(solver.problem.T, dtype=torch.float32).item())
    set_domain(base, solver.problem, elliptic)
    fill_kinds(base, spec)
    base.dwell_form = int(spec.get('dwell_form', 0))              # the rounding order of the double-well drift (include/psp.h)


def upload(x, shape, device, keep, what):
    """``x`` in fp32 on ``device``, row-major by VALUE (a transposed view is copied), kept alive in ``keep``.  shape: what
    ``x`` must have (None: anything); ``what`` opens the ValueError of one that has not."""
    x = torch.as_tensor(x)
    if shape is not None and tuple(x.shape) != shape:
        raise ValueError('%s, got %s' % (what, tuple(x.shape)))
    t = x.detach().to(device=device, dtype=torch.float32).contiguous()
    keep.append(t)
    return t


def fill_value_net(cfg, net_spec, has_time):
    """The value net of a nat.GenlConfig, nat.PinnConfig or nat.GenlEvalConfig from a ``value_net_spec`` (the three name these
    fields alike; time_first / time_scale belong to the value-function ansatz alone)."""
    dims = net_spec['dims']
    cfg.has_time, cfg.n_hidden = (1 if has_time else 0), len(dims) - 2
    for i, h in enumerate(dims[1:-1][:nat.GENL_MAX_HIDDEN_LAYERS]):
        cfg.widths[i] = int(h)
    cfg.activation, cfg.linear_layout = ACT[net_spec['act']], (1 if net_spec['linear'] else 0)


def value_net_limits_reason(dims):
    """(layers, widths, short): why the depth, why the widths of a value net with these ``dims`` are outside what the native
    value-net kernels take -- None where they are inside -- and the one phrase for either."""
    L, lim = len(dims) - 2, (nat.GENL_MAX_HIDDEN_LAYERS, nat.GENL_MAX_WIDTH, nat.GENL_MAX_INPUT)
    layers = widths = None
    if L < 1 or L > lim[0]:
        layers = 'V has %d hidden layers (the native value-net kernels take 1 to %d)' % (L, lim[0])
    if max(dims[1:-1], default=0) > lim[1] or dims[0] > lim[2]:
        widths = 'V is wider than the native value-net kernels take (hidden <= %d, input <= %d)' % lim[1:]
    return layers, widths, ('outside 1-%d hidden layers of <= %d units, input <= %d' % lim if layers or widths else None)


def probe(cfg):
    """The smallest batch of a config the fillers made: what an eligibility function hands to the library's size query."""
    base = getattr(cfg, 'base', cfg)
    base.K_local, base.N = 16, 1
    return cfg
