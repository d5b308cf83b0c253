"""Native plan of GeneralSolver / EllipticSolver for value nets of ANY depth: V = dense-concat net (d [+ 1] -> 1,
arch = [H_1 .. H_L]), 1 <= L <= 4, H_i <= 128 -- the nets the reference's diffusion-loss notebooks train (Allen-Cahn.ipynb:72
arch = [110, 110, 50], the only Allen-Cahn configuration with a published timing; [30, 30, 30, 30]; `Committor function.ipynb`:
[d + 10, d, d, d] with tanh(.)**2; reference function_space.py:116-140 DenseNet, :143-158 DenseNet_tanh).

Same iteration as plan_general_native.GeneralNativePlan (host RNG in the reference's order, K-vector loss weights, the
K_boundary-sized terms by autograd, Adam through psp_adam_step); what differs are the two device steps:
    psp_genl_rollout_fwd   the rollout (csrc/genl_kernels.h: activations in per-tile LDS images, weight tables in L2,
                           rolled fp32-MFMA products; shapes and activation are run-time arguments, nothing is padded on the
                           host; a tile whose trajectories have all stopped leaves the time loop)
    psp_genl_rollout_bwd   ONE hand-written kernel over the executed sample blocks: activations and tangents recomputed, adjoint
                           sweep, every weight gradient as MFMA outer products over the samples of the block (no library GEMM)
The (d, H)-templated kernels of gen_kernels.h stay the fast path for DenseNet arch = [H, H], H <= 64.

Which nets: ``value_net_spec`` recognises the package's DenseNet (any ``activation``), DenseNet_tanh (nn.Linear weights) and --
by structure plus a numerical probe of its forward -- any module that carries ``nn_dims`` and a list ``W`` of (in, out) weights
and biases in the dense-concat layout with one of the three activations: the class a notebook defines for itself
(`Committor function.ipynb` cell 1) runs on the kernels without the package knowing its name.
"""
import ctypes as C

import torch

try:
    from . import kernel_config as kc
    from . import native as nat
    from . import sharding
    from .function_space import DenseNet, DenseNet_tanh
    from .plan_general_native import GeneralNativePlan, set_domain, set_sigma
except ImportError:
    import kernel_config as kc
    import native as nat
    import sharding
    from function_space import DenseNet, DenseNet_tanh
    from plan_general_native import GeneralNativePlan, set_domain, set_sigma

_ACT = kc.ACT


class _IdentityPad:
    """The genl kernels take the real shapes: nothing is padded on the host."""
    identity = True

    def __init__(self, P):
        self.Pp = P

    def last_dim(self, t):
        return t.contiguous()

    def vec(self, t):
        return t

    def scatter_params(self, flat, flat_pad):
        return flat

    def gather_grad(self, grad_pad, out):
        return out


def _dense_concat_forward(x, params, act):
    """The dense-concat forward on (in, out) weights: the formula the kernels implement."""
    n = len(params) // 2
    for i in range(n - 1):
        z = torch.matmul(x, params[2 * i]) + params[2 * i + 1]
        h = torch.relu(z) ** 2 if act == 'relu2' else (torch.tanh(z) ** 2 if act == 'tanh2' else torch.tanh(z))
        x = torch.cat([x, h], 1)
    return torch.matmul(x, params[2 * n - 2]) + params[2 * n - 1]


def _linear_layers_spec(V, dims, d_in, relu_ok):
    """A user-defined module whose ``layers`` are nn.Linear over the growing concatenation (the eigenvalue notebooks' own copy of
    DenseNet_tanh): dict as value_net_spec, or None if it is not that structure or its forward is not the tanh formula."""
    layers = getattr(V, 'layers', None)
    if not isinstance(layers, torch.nn.ModuleList) or len(layers) != len(dims) - 1:
        return None
    fan, params = 0, []
    for i, layer in enumerate(layers):
        fan += dims[i]
        if not isinstance(layer, torch.nn.Linear) or layer.bias is None or tuple(layer.weight.shape) != (dims[i + 1], fan):
            return None
        params += [layer.weight, layer.bias]
    regs = list(V.parameters())
    if len(regs) != len(params) or any(a is not b for a, b in zip(regs, params)):
        return None
    g = torch.Generator().manual_seed(1234)
    probe = torch.randn(16, d_in, generator=g).to(params[0].device)
    with torch.no_grad():
        try:
            want = V(probe)
        except Exception:                                        # pragma: no cover
            return None
        def fwd():
            return _dense_concat_forward(probe, [p.t() if p.dim() == 2 else p for p in params], 'tanh')
        relu = _probe_output_relu(V, probe, want, fwd, params[-1], relu_ok)
    if relu is None:
        return None
    return dict(dims=dims, act='tanh', linear=True, params=params, output_relu=relu)


def _probe_output_relu(V, probe, want, fwd, out_bias, relu_ok):
    """False: V(probe) is fwd(); True: it is relu(fwd()) (accepted only where relu_ok); None: neither.  Where no output of the
    probe batch is negative the two cannot be told apart, so the output bias is lowered until all are (and restored), and V
    decides -- also for a caller that takes no ReLU: a clipped net whose probe outputs happen to be positive is not the plain one."""
    got = fwd()
    if want.shape != got.shape:
        return None
    close = lambda a, b: torch.allclose(a, b, rtol=1e-5, atol=1e-6)     # noqa: E731
    if close(want, got):
        if bool((got < 0).any()):
            return False
        keep = out_bias.detach().clone()
        try:
            out_bias -= (got.max() + 1.0)
            want2, got2 = V(probe), fwd()
        finally:
            out_bias.copy_(keep)
        if close(want2, got2):
            return False
        return True if (relu_ok and close(want2, torch.relu(got2))) else None
    if relu_ok and close(want, torch.relu(got)):
        return True
    return None


def value_net_spec(V, d_in, output_relu_ok=False):
    """dict(dims, act, linear, params, output_relu) if V is a dense-concat net (d_in -> 1) the genl kernels implement, else a
    reason string.  output_relu_ok: the caller's kernels gate a ReLU on the output (plan_eigen_native.py); every other caller
    refuses such a net."""
    dims = getattr(V, 'nn_dims', None)
    if dims is None or len(dims) < 3 or dims[0] != d_in or dims[-1] != 1:
        return 'V is not a dense-concat net (%d -> 1) (no matching nn_dims)' % d_in
    dims = [int(v) for v in dims]
    relu = bool(getattr(V, 'output_relu', False))
    if isinstance(V, (DenseNet, DenseNet_tanh)) and relu and not output_relu_ok:
        return 'V carries a ReLU on its output (output_relu=True): only EigenvalueSolver runs that on the native kernels'
    if isinstance(V, DenseNet):
        return dict(dims=dims, act=getattr(V, 'activation', 'relu2'), linear=False, params=list(V.W), output_relu=relu)
    if isinstance(V, DenseNet_tanh):
        params = []
        for layer in V.layers:
            params += [layer.weight, layer.bias]
        return dict(dims=dims, act='tanh', linear=True, params=params, output_relu=relu)
    lin = _linear_layers_spec(V, dims, d_in, output_relu_ok)
    if lin is not None:
        return lin
    # a user-defined module of the same structure (the notebooks define their own variants): W = [W_1, b_1, .., W_out, b_out] with
    # (in, out) weights over the growing concatenation, registered in that order and nothing else -- and a forward that IS one
    # of the three formulas, checked on a probe batch (a private generator: the global RNG stream is the reference's)
    W = getattr(V, 'W', None)
    if not isinstance(W, (list, tuple)) or len(W) != 2 * (len(dims) - 1):
        return 'V carries no dense-concat parameter list W'
    fan = 0
    for i in range(len(dims) - 1):
        fan += dims[i]
        if tuple(W[2 * i].shape) != (fan, dims[i + 1]) or tuple(W[2 * i + 1].shape) != (dims[i + 1],):
            return 'V.W does not have the dense-concat shapes'
    regs = list(V.parameters())
    if len(regs) != len(W) or any(a is not b for a, b in zip(regs, W)):
        return 'V has parameters besides V.W'
    g = torch.Generator().manual_seed(1234)
    probe = torch.randn(16, d_in, generator=g).to(W[0].device)
    with torch.no_grad():
        try:
            want = V(probe)
        except Exception as e:                                   # pragma: no cover
            return 'V could not be evaluated on a probe batch (%s)' % e
        for act in ('relu2', 'tanh2', 'tanh'):
            relu = _probe_output_relu(V, probe, want, lambda: _dense_concat_forward(probe, W, act), W[-1], output_relu_ok)
            if relu is not None:
                return dict(dims=dims, act=act, linear=False, params=list(W), output_relu=relu)
    return "V's forward is none of the dense-concat formulas the kernels implement (relu^2, tanh^2, tanh)"


def neumann_points(img_last, nexec, n_last, XN, tN):
    """Where the BSDE loss's Neumann residual takes grad_x V (solver.py:1182-1183): [x, t] of every trajectory at the start of
    the last loop step n_last the reference executed.  A tile that left the time loop before that step (nexec[tile] <= n_last)
    never wrote slot n_last of the path store; its trajectories have all stopped, and a stopped trajectory keeps its state, so
    its point is the frozen (X_N, t_N).  img_last: (K, d + 1) decoded slot n_last; nexec: (ceil(K / 16),) loop steps per tile;
    XN: (K, d); tN: (K,).  Returns (K, d + 1); the unread slots never enter the result, not even as a NaN."""
    K = img_last.shape[0]
    left = (nexec.to(torch.int64) <= n_last).repeat_interleave(16)[:K].unsqueeze(1)
    return torch.where(left, torch.cat([XN, tN.reshape(-1, 1)], 1), img_last)


def deep_config(solver, net, spec, elliptic, K_local, k_offset, device, keep):
    """The psp_genl_config of a solver, its value net (``value_net_spec``) and its problem's ``general_native_spec()``; the
    tensors its pointers name go to ``device`` and into ``keep``.  spec None (deep_eligibility on a problem outside the catalogue,
    which plan_general_native.native_eligibility refuses): the net's part alone."""
    gcfg = nat.GenlConfig()
    gcfg.base.d = solver.d
    if spec is not None:
        kc.fill_problem(gcfg.base, solver, spec, elliptic, K_local, k_offset, solver.noise)
        set_sigma(gcfg, spec, device, keep)
        if spec['drift'][1] is not None:
            gcfg.base.drift = nat.ptr(kc.upload(spec['drift'][1], None, device, keep, 'the drift vector'))
    kc.fill_value_net(gcfg, net, not elliptic)
    return gcfg


def deep_eligibility(solver):
    """None if the value net is one the genl kernels take, else a reason."""
    elliptic = bool(solver.elliptic)
    net = value_net_spec(solver.V, solver.d + (0 if elliptic else 1))
    if isinstance(net, str):
        return net
    layers, widths, _ = kc.value_net_limits_reason(net['dims'])
    if layers or widths:
        return layers or widths
    keep = []                                                     # (the query validates the pointers, it reads nothing)
    cfg = kc.probe(deep_config(solver, net, kc.catalogue_spec(solver.problem)[0], elliptic, 16, 0, torch.device('cpu'), keep))
    lib = nat.load()
    if lib.psp_genl_query(C.byref(cfg), C.byref(nat.GenlSizes())) != 0:
        return lib.psp_last_error().decode()
    return None


class GeneralDeepPlan(GeneralNativePlan):
    output_relu_ok = False          # plan_eigen_native.EigenDeepPlan: its forward gates the output ReLU

    def _query(self, gcfg, sz):
        """The size query of this plan's forward entry point."""
        return self.lib.psp_genl_query(C.byref(gcfg), C.byref(sz))

    def __init__(self, solver):
        s = solver
        self.s = s
        self.lib = nat.load()
        self.dev = s.device
        self._shard(s.K_original)
        self.K_cap = self.K_local
        self.net = s.V
        self.key = None
        self.elliptic = bool(s.elliptic)
        net = value_net_spec(s.V, s.d + (0 if self.elliptic else 1), self.output_relu_ok)
        assert not isinstance(net, str), net
        self.net_spec = net
        self.dims = list(net['dims'])
        self.L = len(self.dims) - 2
        self.H = self.dims[1]
        self._flatten(net['params'])
        spec = s.problem.general_native_spec()
        self._keep = []
        gcfg = deep_config(s, net, spec, self.elliptic, self.K_local, self.lo, self.dev, self._keep)
        cfg = gcfg.base
        self.gcfg, self.cfg = gcfg, cfg
        sz = nat.GenlSizes()
        nat.check(self._query(gcfg, sz), 'psp_genl_query')
        assert sz.n_params == self.P, (sz.n_params, self.P)
        self.sizes = sz
        self.matrix_mode, self.range_flag = 'fp32', None            # fp32 MFMA only (v_mfma_f32_16x16x4_f32)
        self.d_pad, self.H_pad = s.d, self.H
        self.pad = _IdentityPad(self.P)
        self.flat_k = self.flat
        dev, f32 = self.dev, torch.float32
        self.tables = torch.empty(sz.table_bytes // 4, dtype=f32, device=dev)
        self.path = torch.empty(sz.path_bytes // 4, dtype=f32, device=dev)
        self.ahat = torch.zeros((sz.ahat_bytes + 3) // 4, dtype=f32, device=dev)
        self.grad_partial = torch.empty(sz.grad_partial_bytes // 4, dtype=f32, device=dev)
        self.grad_k = self.grad
        self._common_buffers(s.d)

    def _check_sizes(self):
        sz = nat.GenlSizes()
        nat.check(self._query(self.gcfg, sz), 'psp_genl_query')
        assert sz.path_bytes <= self.path.numel() * 4 and sz.ahat_bytes <= self.ahat.numel() * 4
        if sz.grad_partial_bytes > self.grad_partial.numel() * 4:
            self.grad_partial = torch.empty(sz.grad_partial_bytes // 4, dtype=torch.float32, device=self.dev)
        self.sizes = sz

    def _x_image_floats(self):
        return 4 * ((self.dims[0] + 15) // 16) * 64

    def _tile_steps(self):
        """Loop steps every tile of this rank executed (int32 view of the tail of `ahat`, include/psp.h)."""
        nt = (self.K_local + 15) // 16
        return self.ahat[(self.s.N + 1) * nt * 16:(self.s.N + 1) * nt * 16 + nt].view(torch.int32)

    def _last_step_points(self, n_last):
        """As GeneralNativePlan's, but the genl forward leaves the time loop per tile: tiles that stopped early give X_N, t_N."""
        d_in = self.dims[0]
        img = super()._last_step_points(n_last)[:, :d_in]
        return neumann_points(img, self._tile_steps(), n_last, self.XN, self.tN)

    def _loop_steps(self, t0):
        """The kernels count the executed steps of every tile themselves: the loop of the reference runs as long as the
        longest-running tile."""
        m = self._tile_steps().max().reshape(1)
        dist, _, world = sharding.dist_info()
        if world > 1:
            dist.all_reduce(m, op=dist.ReduceOp.MAX)
        return int(m.item())

    def _launch_fwd(self, flat_k, x0, t0, xi, l, st):
        nat.check(self.lib.psp_genl_rollout_fwd(C.byref(self.gcfg), nat.ptr(self.flat), nat.ptr(x0), nat.ptr(t0), nat.ptr(xi),
                                                int(self.s.seed) & 0xFFFFFFFFFFFFFFFF, l, nat.ptr(self.tables), nat.ptr(self.path),
                                                nat.ptr(self.ahat), nat.ptr(self.VN), nat.ptr(self.YN), nat.ptr(self.XN_k),
                                                nat.ptr(self.tN), nat.ptr(self.kcount), st), 'psp_genl_rollout_fwd')

    def _launch_bwd(self, flat_k, st):
        nat.check(self.lib.psp_genl_rollout_bwd(C.byref(self.gcfg), nat.ptr(self.flat), nat.ptr(self.tables), nat.ptr(self.path),
                                                nat.ptr(self.ahat), nat.ptr(self.wY), nat.ptr(self.wV), nat.ptr(self.grad_partial),
                                                nat.ptr(self.grad), st), 'psp_genl_rollout_bwd')
