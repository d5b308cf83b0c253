"""Native plan of EigenvalueSolver: the iteration of eigenvalue_solver.py on the run-time-shaped value-net kernels.

Per iteration:
    normalisation and periodic boundary terms   torch autograd on views of the flat parameter vector (at most K + 2 K_boundary
                                                points), in the notebooks' RNG order, in front of the rollout
    psp_genl_rollout_fwd_eig                    the rollout (csrc/genl_kernels.h, EIG instances): lambda read from device memory,
                                                V = relu(o) and its gate, the h / drift kinds of the two problems, and
                                                S_k = sum_n act_n V(X_n) dt per trajectory
    psp_genl_rollout_bwd                        the parameter gradient of alpha[0] mean((V(X_N) - Y_N)^2), Y_0 = V(X_0) attached
    psp_adam_step                               V, then lambda with dLoss/dlambda = alpha[0] (2 / K) sum_k D_k S_k
lambda never visits the host: its value, gradient and Adam moments are device tensors, and ``lambda_log`` and the loss logs are
device buffers read back when train() prints or returns.
"""
import ctypes as C
import time

import torch

try:
    from . import kernel_config as kc
    from . import native as nat
    from . import plan_common as pc
    from . import sharding
    from .plan_general_deep import GeneralDeepPlan, deep_config, value_net_spec
    from .eigenvalue_solver import periodic_terms
except ImportError:
    import kernel_config as kc
    import native as nat
    import plan_common as pc
    import sharding
    from plan_general_deep import GeneralDeepPlan, deep_config, value_net_spec
    from eigenvalue_solver import periodic_terms


def eigen_eligibility(solver):
    """None if the EIG instances of the value-net kernels take this EigenvalueSolver, else a reason."""
    s = solver
    if s.device.type != 'cuda':
        return 'device is %s (the HIP rollout needs a GPU)' % s.device
    if sharding.dist_info()[2] > 1:
        return 'EigenvalueSolver runs on one rank (the native plan is not sharded)'
    if getattr(s, 'mlp_dtype', 'fp32') != 'fp32':
        return "mlp_dtype=%r: the eigenvalue kernels are fp32 only" % (s.mlp_dtype,)
    net = value_net_spec(s.V, s.d, output_relu_ok=True)
    if isinstance(net, str):
        return net
    layers, widths, _ = kc.value_net_limits_reason(net['dims'])
    if layers or widths:
        return layers or widths
    spec, why = kc.catalogue_spec(s.problem, names=('b', 'sigma', 'h', 'g'))
    if spec is None:
        return why
    if spec.get('sigma') is not None:
        return 'a dense sigma is not built for EigenvalueSolver'
    if not nat.is_built():
        raise nat.NativeLibraryError('libpsp_hip.so is not built; run __graft_entry__.build()')
    keep = []                                                     # (the query validates the pointers, it reads nothing)
    cfg = kc.probe(deep_config(s, net, spec, bool(s.elliptic), 16, 0, torch.device('cpu'), keep))
    eig = nat.GenlEig(struct_bytes=C.sizeof(nat.GenlEig), output_relu=1 if net['output_relu'] else 0)
    lib = nat.load()
    if lib.psp_genl_query_eig(C.byref(cfg), C.byref(eig), C.byref(nat.GenlSizes())) != 0:
        return lib.psp_last_error().decode()
    return None


class EigenDeepPlan(GeneralDeepPlan):
    output_relu_ok = True

    def __init__(self, solver):
        self.eig = nat.GenlEig(struct_bytes=C.sizeof(nat.GenlEig))
        self.eig.output_relu = 1 if value_net_spec(solver.V, solver.d, output_relu_ok=True)['output_relu'] else 0
        super().__init__(solver)
        dev, f32 = self.dev, torch.float32
        s = solver
        # lambda on the device: the SingleParam's own tensor (its optimiser and state_dict keep seeing live values)
        self.lam_param = s.lambda_.Y_0
        if self.lam_param.device != dev or self.lam_param.dtype != f32:
            self.lam_param.data = self.lam_param.data.to(device=dev, dtype=f32)
        self.lam = self.lam_param.data
        self.lam_grad = torch.zeros(1, dtype=f32, device=dev)
        self.lam_m = torch.zeros(1, dtype=f32, device=dev)
        self.lam_v = torch.zeros(1, dtype=f32, device=dev)
        self._S = torch.zeros(self.K_cap, dtype=f32, device=dev)
        self.eig.lambda_ = nat.ptr(self.lam)
        self.eig.s_out = nat.ptr(self._S)
        self.out_relu = bool(self.eig.output_relu)
        self.last_parts = None
        self.timing = None                                        # tools/time_eigenvalue.py: [seconds in the torch-side terms]

    def _query(self, gcfg, sz):
        return self.lib.psp_genl_query_eig(C.byref(gcfg), C.byref(self.eig), C.byref(sz))

    def _launch_fwd(self, flat_k, x0, t0, xi, l, st):
        nat.check(self.lib.psp_genl_rollout_fwd_eig(C.byref(self.gcfg), C.byref(self.eig), nat.ptr(self.flat), nat.ptr(x0), nat.ptr(t0),
                                                    nat.ptr(xi), int(self.s.seed) & 0xFFFFFFFFFFFFFFFF, l, nat.ptr(self.tables),
                                                    nat.ptr(self.path), nat.ptr(self.ahat), nat.ptr(self.VN), nat.ptr(self.YN),
                                                    nat.ptr(self.XN_k), nat.ptr(self.tN), nat.ptr(self.kcount), st),
                  'psp_genl_rollout_fwd_eig')

    def _torch_terms(self, gen):
        """Normalisation and periodic boundary terms, differentiated into p.grad; the draws in the notebooks' order."""
        s = self.s
        norm, center = s._normalisation_term(gen)
        Xb, Xr = s._sample_periodic_pair()
        t_val, t_grad = periodic_terms(s.V, Xb, Xr)
        loss_b = norm + s.alpha[1] * t_val + s.alpha[1] * t_grad
        loss_b.backward()
        return loss_b.detach(), center.detach(), t_val.detach(), t_grad.detach()

    def iteration(self, l):
        s, lib, dev = self.s, self.lib, self.dev
        st = nat.stream_ptr(dev)
        d, pb, K, N = s.d, s.problem, s.K, s.N
        reference_noise = s.noise == 'reference'
        for p in self.params:
            p.grad = None
        gen = None
        if not reference_noise:
            if not hasattr(self, '_gen'):
                self._gen = torch.Generator(device=dev)
            self._gen.manual_seed(int(s.seed) * 1000003 + l)
            gen = self._gen
        t_a = time.perf_counter() if self.timing is not None else 0.0
        loss_b, center, t_val, t_grad = self._torch_terms(gen)
        if self.timing is not None:
            torch.cuda.synchronize(dev)
            self.timing.append(time.perf_counter() - t_a)
        self._set_batch(K)
        xi, rng_state = None, None
        if reference_noise:
            X = (pb.X_r - pb.X_l) * torch.rand(K, d).to(dev) + pb.X_l
            rng_state = torch.get_rng_state()                    # the number of draws is known after the rollout
            xi = torch.stack([torch.randn(K, d) for _ in range(N)]).to(dev).contiguous()
        else:
            X = (pb.X_r - pb.X_l) * torch.rand(K, d, generator=gen, device=dev) + pb.X_l
        x0 = X.contiguous()
        t0 = torch.zeros(K, device=dev)
        self.kcount.zero_()
        self._launch_fwd(self.flat, x0, t0, xi, l, st)
        if rng_state is not None:                                # rewind, then consume what the notebooks' loop consumes
            draws = self._draws_executed(t0)
            torch.set_rng_state(rng_state)
            for _ in range(draws):
                torch.randn(K, d)
        D = self.VN - self.YN                                    # Y_N carries Y_0 = V(X_0): D = V(X_N) - V(X_0) - Y
        domain = (torch.sum(D.double() ** 2) / K).float()
        loss = loss_b + s.alpha[0] * domain
        w = (2.0 * s.alpha[0] / K) * D
        self.wY[:K].copy_(-w)
        self.wV[:K].copy_(w * (self.VN > 0).float() if self.out_relu else w)     # d relu(o_N) / d theta = 1[o_N > 0] d o_N / d theta
        self._launch_bwd(self.flat, st)
        self.grad += torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in self.params])
        self.lam_grad[0] = torch.sum(w.double() * self._S[:K].double()).float()     # dY_N / dlambda = -S_k, dD / dlambda = S_k
        self.last_v_l2 = self._v_l2_from_path() if self.log_v_l2 else None      # before the update, as the notebooks log it
        self.step += 1
        pc.adam_step(lib, self.flat, self.grad, self.m, self.v, self.P, self.step,
                     pc.adam_hyper(self.net, s.lr, NotImplementedError), st)
        pc.adam_step(lib, self.lam, self.lam_grad, self.lam_m, self.lam_v, 1, self.step,
                     pc.adam_hyper(s.lambda_, s.lr, NotImplementedError), st, 'psp_adam_step(lambda)')     # after V
        self.last_parts = torch.stack([loss, center, t_val, t_grad, domain, self.lam[0].clone()])
        return loss, self.kcount.clone()

    def train(self):
        return self._train_loop()

    def _train_loop(self):
        s = self.s
        parts, counts, vl2 = [], [], []
        t_block = time.time()
        for l in range(s.L):
            _, kc = self.iteration(l)
            parts.append(self.last_parts)
            counts.append(kc)
            if self.last_v_l2 is not None:
                vl2.append(self.last_v_l2)
            if (s.verbose and l % s.print_every == 0) or l == s.L - 1:
                vals = torch.stack(parts).cpu()                   # one sync per block
                now = time.time()
                n = vals.shape[0]
                s.loss_log += vals[:, 0].tolist()
                s.loss_log_center += [s.center_scale * v for v in vals[:, 1].tolist()]
                s.loss_log_boundary += vals[:, 2].tolist()
                s.loss_log_derivative_boundary += vals[:, 3].tolist()
                s.loss_log_domain += vals[:, 4].tolist()
                s.lambda_log += vals[:, 5].tolist()
                s.K_log += [int(c.item()) for c in counts]
                s.V_L2_log += torch.stack(vl2).cpu().tolist() if vl2 else [0.0] * n
                s.times += [(now - t_block) / n] * n
                t_block = now
                if s.verbose and l % s.print_every == 0:
                    print('%d - loss = %.4e, v L2 error = %.4e, lambda = %.4e, %.4f s/iter'
                          % (l, s.loss_log[-1], s.V_L2_log[-1], s.lambda_log[-1], s.times[-1]))
                parts, counts, vl2 = [], [], []
