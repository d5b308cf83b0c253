"""Native (HIP) execution plan of GeneralSolver.train_PINN / EllipticSolver.train_PINN (reference solver.py:1208-1323, :828-931).

Per iteration:
    host RNG in the reference's order (boundary batch, domain sample with the 'two_spheres' rejection, t ~ U(0, T), boundary times)
    the K_boundary-sized data terms (terminal, Dirichlet / Neumann) by torch autograd into p.grad, as the diffusion-loss plans do
    psp_pinn_residual   -> R_k = [V_t] + s^2/2 Lap V + b . grad V + h(x, V, s grad V) by forward-Laplacian propagation
    loss = alpha0 mean(R^2) or alpha0 var(R) (PINN_log_variance); rbar = dLoss/dR, two K-vector operations in torch
    psp_pinn_backward   -> flat gradient of the domain part (hand-written adjoint, fp32-MFMA weight gradients, fixed-order sum)
    psp_adam_step
The reference differentiates the net d + 1 times per iteration (one autograd.grad per input column, each through the graph of
the gradient); here the value, every tangent and the Laplacian row pass through the net once, in one kernel.

EllipticSolver(full_hessian=True, hessian='directions') with a dense constant sigma B: the reference takes trace(B B^T Hess V)
from one autograd.functional.hessian call per sample (the default, hessian='reference', keeps doing that on the composite plan:
the plan a configuration runs on does not change under its user).  Here B B^T is factored once on the host (``direction_table``) into r = rank(B)
vectors u_j with sum_j u_j u_j^T = B B^T, and the same kernels carry the u_j as tangent rows: 1/2 sum_j u_j^T Hess V u_j.

Scope: a dense-concat value net the run-time-shaped kernels take (plan_general_deep.value_net_spec: 1-4 hidden layers, widths
<= 128, input <= 112, relu^2 / tanh / tanh^2), a catalogue problem whose h does not read t (one that does: below), with a scaled-identity sigma or --
EllipticSolver with full_hessian=True and hessian='directions' only -- a dense one, any domain, one rank.  ``pinn_eligibility`` names what keeps a
configuration on the composite plan.

An h that reads t (ExponentialOnSphereNonlinearParabolic): the reference hands it t_n as (K, 1), so the residual broadcasts to the
(K, K) matrix R[i, j] = A_j + nl(exp(2 al |x_j|^2 + 2 tau t_i) - y_j^2) and the loss is its mean square.  The default,
GeneralSolver(pinn_time_h='torch'), keeps that on the composite plan; pinn_time_h='native' runs it here: everything that passes
through the net is per sample j, the pair part is an elementwise function of (t_i, sample j), so per iteration
    psp_pinn_pairs_residual -> A_j;  psp_pinn_pairs_reduce -> the loss (a device scalar), rho_j = 2 a0 / K^2 sum_i R[i, j] and
    nu_j = 2 a0 / K^2 sum_i R[i, j] nl'(..) (-2 y_j);  psp_pinn_pairs_backward(rbar = rho, vadd = nu);  psp_adam_step
with nothing read on the host.
"""
import ctypes as C
import time

import torch

try:
    from . import kernel_config as kc
    from . import native as nat
    from . import plan_common as pc
    from . import sharding
    from .plan_general_deep import value_net_spec, deep_eligibility
except ImportError:
    import kernel_config as kc
    import native as nat
    import plan_common as pc
    import sharding
    from plan_general_deep import value_net_spec, deep_eligibility


def pinn_eligibility(solver):
    """None if the forward-Laplacian kernels take this solver's train_PINN(), else the reason it runs on the composite plan."""
    s = solver
    full = bool(s.full_hessian)
    if full and not s.elliptic:
        return ('full_hessian=True on GeneralSolver: the reference hands a d-column point to a net of d + 1 inputs there, '
                'so there is no reference behaviour to match (composite only)')
    if full and getattr(s, 'hessian', 'reference') != 'directions':
        return ("full_hessian=True takes trace(B B^T Hess V) sample by sample, as the reference does; "
                "EllipticSolver(hessian='directions') runs it on the direction-table kernels")
    if getattr(s, 'mlp_dtype', 'auto') not in ('auto', 'fp32'):
        return 'mlp_dtype=%r: the PINN kernels are fp32 MFMA only' % s.mlp_dtype
    if getattr(s, 'noise', 'reference') != 'reference':
        return "noise=%r: train_PINN draws its points from the host generator (noise='reference')" % s.noise
    if sharding.dist_info()[2] > 1:
        return 'more than one rank: the PINN kernels are single-rank'
    spec, why = kc.catalogue_spec(s.problem)
    if spec is None:
        return why
    dense = spec.get('sigma') is not None
    if dense and not full:
        return ('a dense sigma without full_hessian: the reference takes B[0,0]^2 times the Laplacian for it, which is no '
                'operator of the problem (composite only)')
    if spec['h'] == nat.GH_SINNORM2:
        return 'PSP_GH_SINNORM2 (SinNorm2.h) is built in the rollout kernels only, not in the PINN kernels'
    if dense and (spec['h'] == nat.GH_QUAD or (spec['h'] == nat.GH_AFFINE_EXP and spec['h_par'][2] != 0.0)):
        return 'an h that reads z = B grad V is not in the PINN kernels for a dense sigma'
    pairs = h_reads_t(spec)
    if pairs and getattr(s, 'pinn_time_h', 'torch') != 'native':
        return ("h reads t: the reference hands it t_n as (K, 1) and the residual broadcasts to (K, K) (composite by default; "
                "GeneralSolver(pinn_time_h='native') runs it on the pair kernel)")
    if spec['drift'][0] not in (nat.DRIFT_ZERO, nat.DRIFT_DIAG, nat.DRIFT_DOUBLE_WELL):
        return 'a dense drift is not in the PINN kernels'
    if not nat.is_built():
        raise nat.NativeLibraryError('libpsp_hip.so is not built; run __graft_entry__.build()')
    why = deep_eligibility(s)                                     # the net: structure, depth, widths
    if why is not None:
        return why
    if pairs:                                                     # what psp_pinn_pairs_query refuses (no GPU needed)
        net = value_net_spec(s.V, s.d + (0 if s.elliptic else 1))
        cfg = pinn_config(s, net, spec, torch.device('cpu'), [])
        if nat.load().psp_pinn_pairs_query(C.byref(cfg), C.byref(nat.PinnSizes()), C.byref(C.c_int64())) != 0:
            return 'h reads t and the pair kernel does not take this configuration: ' + nat.last_error()
    if s.device.type != 'cuda':
        if full:
            return 'full_hessian=True runs on the direction-table kernels, which need a GPU: device is %s' % s.device
        return 'device is %s (the HIP kernels need a GPU)' % s.device
    return None


def h_reads_t(spec):
    """h_par = (al, d, e, tau) of the exponential-on-the-ball kinds carries the time term; the later kinds read no t."""
    return (nat.GH_EXPBALL_LIN <= spec['h'] <= nat.GH_EXPBALL_SIN_FULL and len(spec.get('h_par', ())) > 3
            and spec['h_par'][3] != 0.0)


def pinn_config(s, net, spec, dev, keep):
    """psp_pinn_config of a solver for K_original points; the tensors its pointers name are appended to ``keep``."""
    cfg = nat.PinnConfig()
    cfg.d, cfg.K = s.d, s.K_original
    kc.fill_value_net(cfg, net, not s.elliptic)
    kc.fill_kinds(cfg, spec)
    if spec.get('sigma') is None:                              # (full_hessian with s I is s^2 times the Laplacian)
        cfg.sigma_kind = nat.GENL_SIGMA_SCALED
    else:                                                      # trace(B B^T Hess V) as sum_j u_j^T Hess V u_j
        dirs = kc.upload(direction_table(spec['sigma']), None, dev, keep, 'the direction table')
        cfg.sigma_kind, cfg.n_dirs, cfg.dirs = nat.GENL_SIGMA_DENSE, dirs.shape[0], nat.ptr(dirs)
    if spec['drift'][1] is not None:
        cfg.drift = nat.ptr(kc.upload(spec['drift'][1], None, dev, keep, 'the drift vector'))
    return cfg


def direction_table(B):
    """(r, d) float64 rows u_j = sqrt(lambda_j) q_j over the eigenpairs of B B^T above the default tolerance of
    torch.linalg.matrix_rank (largest eigenvalue times d times the float64 epsilon): sum_j u_j u_j^T = B B^T, so
    sum_j u_j^T H u_j = trace(B B^T H) for every symmetric H, in r = rank(B) directions."""
    B = torch.as_tensor(B).detach().to(device='cpu', dtype=torch.float64)
    lam, Q = torch.linalg.eigh(B @ B.t())
    keep = lam > lam.abs().max() * B.shape[0] * torch.finfo(torch.float64).eps
    return (Q[:, keep] * torch.sqrt(lam[keep])).t().contiguous()


class PinnNativePlan:
    def __init__(self, solver):
        s = solver
        self.s, self.lib, self.dev = s, nat.load(), s.device
        self.net, self.key = s.V, None
        self.elliptic = bool(s.elliptic)
        net = value_net_spec(s.V, s.d + (0 if self.elliptic else 1))
        assert not isinstance(net, str), net
        self.net_spec = net
        self.params = net['params']
        self.flat = pc.rehome_params(self.params, self.dev)       # the net's tensors become views of it
        self.P = self.flat.numel()
        self.grad = torch.empty(self.P, dtype=torch.float32, device=self.dev)
        spec = s.problem.general_native_spec()
        self._keep = []
        self.cfg = cfg = pinn_config(s, net, spec, self.dev, self._keep)
        self.pairs = h_reads_t(spec)                               # the (K, K) residual of an h that reads t
        sz = nat.PinnSizes()                                       # sized for the largest batch an iteration can see
        if self.pairs:
            work = C.c_int64()
            nat.check(self.lib.psp_pinn_pairs_query(C.byref(cfg), C.byref(sz), C.byref(work)), 'psp_pinn_pairs_query')
        else:
            nat.check(self.lib.psp_pinn_query(C.byref(cfg), C.byref(sz)), 'psp_pinn_query')
        assert sz.n_params == self.P, (sz.n_params, self.P)
        self.sizes, self.K_cap = sz, s.K_original
        dev, f32 = self.dev, torch.float32
        self.scratch = torch.empty(sz.scratch_bytes // 4, dtype=f32, device=dev)
        self.grad_partial = torch.empty(sz.grad_partial_bytes // 4, dtype=f32, device=dev)
        self.R = torch.empty(self.K_cap, dtype=f32, device=dev)
        self.rbar = torch.empty(self.K_cap, dtype=f32, device=dev)
        self.m = torch.zeros(self.P, dtype=f32, device=dev)
        self.v = torch.zeros(self.P, dtype=f32, device=dev)
        if self.pairs:
            self.pair_work = torch.empty(work.value, dtype=torch.uint8, device=dev)
            self.nu = torch.empty(self.K_cap, dtype=f32, device=dev)
            self.loss_dev = torch.empty(1, dtype=f32, device=dev)
        self.step = 0
        self.test_log = pc.device_test_log(s, net, self.elliptic, dev)

    def _data_terms(self, X, X_b, t_b):
        """The K_boundary-sized terms of solver.py:1288-1303 / :909-912, differentiated by autograd into p.grad.  Returns
        (weighted sum or None, the unweighted boundary residual the elliptic class logs)."""
        s, pb, dev = self.s, self.s.problem, self.dev
        if not s.boundary_loss and not (self.elliptic and s.log_loss_parts):
            return None, None
        if self.elliptic:
            res = torch.mean((s.V(X_b).squeeze() - s._g_on_boundary(X_b)) ** 2)
            if not s.boundary_loss:
                return None, res.detach()
            term = s.alpha[1] * res
        else:
            Kb, res = s.K_boundary, None
            X_T = torch.cat([X[:Kb, :], pb.T * torch.ones(Kb, device=dev).unsqueeze(1)], 1)
            term = s.alpha[1] * torch.mean((s.V(X_T).squeeze() - pb.f(X[:Kb, :])) ** 2)
            if s.bounded:
                term = term + s.alpha[2] * s.boundary_residual(torch.cat([X_b, t_b], 1), X_b, t_b)
        term.backward()
        return term.detach(), (res.detach() if res is not None else None)

    def residual(self, X, t):
        """R (K,) of the points X (K, d) [and times t (K,)] with the current parameters; leaves the backward's scratch."""
        K = X.shape[0]
        if self.pairs:
            raise RuntimeError('h reads t: the residual is a (K, K) matrix, see pairs_loss_and_grad()')
        if K <= 0 or K > self.K_cap:
            raise RuntimeError('batch of %d points outside the plan capacity %d' % (K, self.K_cap))
        self.cfg.K = K
        self._x = X.detach().to(torch.float32).contiguous()
        self._t = None if t is None else t.detach().to(torch.float32).reshape(-1).contiguous()
        st = nat.stream_ptr(self.dev)
        nat.check(self.lib.psp_pinn_residual(C.byref(self.cfg), nat.ptr(self.flat), nat.ptr(self._x), nat.ptr(self._t),
                                             nat.ptr(self.scratch), nat.ptr(self.R), st), 'psp_pinn_residual')
        return self.R[:K]

    def backward(self, rbar):
        """self.grad = sum_k rbar_k dR_k/dtheta for the batch of the last residual() call."""
        K = self.cfg.K
        self.rbar[:K].copy_(rbar)
        st = nat.stream_ptr(self.dev)
        nat.check(self.lib.psp_pinn_backward(C.byref(self.cfg), nat.ptr(self.flat), nat.ptr(self._x), nat.ptr(self._t),
                                             nat.ptr(self.scratch), nat.ptr(self.rbar), nat.ptr(self.grad_partial),
                                             nat.ptr(self.grad), st), 'psp_pinn_backward')
        return self.grad

    def pairs_loss_and_grad(self, X, t, a0):
        """An h that reads t: alpha0 mean over the (K, K) residual squared, as a device scalar, and its gradient in self.grad.
        self.R holds A, self.rbar holds rho."""
        K = X.shape[0]
        if K <= 0 or K > self.K_cap:
            raise RuntimeError('batch of %d points outside the plan capacity %d' % (K, self.K_cap))
        self.cfg.K = K
        self._x = X.detach().to(torch.float32).contiguous()
        self._t = t.detach().to(torch.float32).reshape(-1).contiguous()
        st, cfg, ptr = nat.stream_ptr(self.dev), C.byref(self.cfg), nat.ptr
        x, tt, scratch = ptr(self._x), ptr(self._t), ptr(self.scratch)
        nat.check(self.lib.psp_pinn_pairs_residual(cfg, ptr(self.flat), x, tt, scratch, ptr(self.R), st), 'psp_pinn_pairs_residual')
        nat.check(self.lib.psp_pinn_pairs_reduce(cfg, x, tt, scratch, ptr(self.R), float(a0), ptr(self.pair_work),
                                                 ptr(self.loss_dev), ptr(self.rbar), ptr(self.nu), st), 'psp_pinn_pairs_reduce')
        nat.check(self.lib.psp_pinn_pairs_backward(cfg, ptr(self.flat), x, tt, scratch, ptr(self.rbar), ptr(self.nu),
                                                   ptr(self.grad_partial), ptr(self.grad), st), 'psp_pinn_pairs_backward')
        return self.loss_dev[0].clone()                          # (the buffer is the next iteration's too)

    def iteration(self, l):
        s, pb, dev, ell = self.s, self.s.problem, self.dev, self.elliptic
        for p in self.params:
            p.grad = None
        # ---- host RNG in the reference's order
        X_b = s._sample_boundary() if s.bounded else None
        X = s.sample_domain()
        K = s.K                                                  # 'two_spheres': the rejection step has just set it
        t_n = t_b = None
        if not ell:
            t_n = torch.rand(K, 1).to(dev) * pb.T
            if s.boundary_loss and s.bounded:
                t_b = torch.rand(s.K_boundary, 1).to(dev) * pb.T
        term, res_b = self._data_terms(X, X_b, t_b)
        a0 = s.alpha[0]
        if self.pairs:                                           # the loss is a device scalar, the gradient is in self.grad
            loss = self.pairs_loss_and_grad(X, t_n, a0)
        else:
            R = self.residual(X, t_n)
            if ell and s.PINN_log_variance:
                loss = a0 * torch.var(R)
                rbar = (2.0 * a0 / (K - 1)) * (R - torch.mean(R))
            else:
                loss = a0 * torch.mean(R ** 2)
                rbar = (2.0 * a0 / K) * R
            self.backward(rbar)
        parts = (loss / a0, res_b) if s.log_loss_parts else None
        if term is not None:
            loss = loss + term
            self.grad += torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in self.params])
        self.step += 1
        st = nat.stream_ptr(dev)
        pc.adam_step(self.lib, self.flat, self.grad, self.m, self.v, self.P, self.step,
                     pc.adam_hyper(self.net, s.lr, NotImplementedError), st)
        v_l2 = None
        if ell:                                                  # solver.py:919: after the step, on this iteration's points
            with torch.no_grad():
                err = (s.V(X).squeeze() - torch.as_tensor(pb.v_true(X)).float().to(dev).squeeze()) ** 2
            v_l2 = torch.mean(err * s.delta_t_np)
        if s.K_test_log is not None and self.test_log is not None:
            self.test_log.enqueue(self.flat, s.seed, l, l, st)
        elif s.K_test_log is not None:
            s._log_test_error('elliptic' if ell else 'parabolic')
        return loss, v_l2, parts

    def train(self):
        return pc.train_with_test_log(self.s, self.test_log, self._train_loop)

    def _train_loop(self):
        s = self.s
        losses, vl2, parts = [], [], []
        t_block = time.time()
        for l in range(s.L):
            loss, v, pr = self.iteration(l)
            losses.append(loss)
            if v is not None:
                vl2.append(v)
            if pr is not None:
                parts.append(pr)
            if (s.verbose and l % s.print_every == 0) or l == s.L - 1:
                vals = torch.stack(losses).cpu().tolist()          # one sync per block
                now = time.time()
                s.loss_log += vals
                s.V_L2_log += torch.stack(vl2).cpu().tolist() if vl2 else [0] * len(vals)
                for dom, bnd in parts:
                    s.loss_log_domain.append(dom.item())
                    if bnd is not None:
                        s.loss_log_boundary.append(bnd.item())
                s.times += [(now - t_block) / len(vals)] * len(vals)
                t_block = now
                if s.verbose and l % s.print_every == 0:
                    print('%d - loss = %.4e - v L2 error = %.4e - %.4f s/iter' % (l, s.loss_log[-1], s.V_L2_log[-1], s.times[-1]))
                losses, vl2, parts = [], [], []
