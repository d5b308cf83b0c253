"""EigenvalueSolver: the eigenvalue experiments of the diffusion-loss paper -- `Eigenvalue - Fokker-Planck.ipynb` and
`Eigenvalue - nonlinear Schroedinger equation, d = 5 / d = 10.ipynb` of the reference -- as a class.  The notebooks keep their
problem classes, nets and training loop in their own cells; here the problems are ``problems.FokkerPlanckEigenvalue`` /
``problems.SchroedingerEigenvalue``, the nets are ``DenseNet(..., output_relu=True, ...)`` / ``DenseNet_tanh(..., output_relu=True)``
and the loop is ``train()``.

One iteration is the step of ``EllipticSolver.train`` with loss_method='diffusion', adaptive_forward_process=False,
detach_forward=True on the box [X_l, X_r]^d (the proposal is tested against both faces), with these differences:
  * a trainable scalar lambda (a SingleParam with its own Adam) enters the Y update:
        Y += ((-h(X, V(X), Z) - lambda V(X)) dt + Z . xi sqrt(dt)) act,     Y started at 0;
    lambda is stepped after V and logged after its step;
  * domain loss      alpha[0] mean((V(X_N) - V(X_0) - Y)^2);
  * periodic boundary terms instead of Dirichlet data: a boundary batch X_b and its reflection X_b' (the same np.random.shuffle
    and rand draws as the 'square' boundary), alpha[1] mean((V(X_b) - V(X_b'))^2) + alpha[1] mean((grad V(X_b) - grad V(X_b'))^2);
  * a normalisation: 'center' -- (V(X_0) - v_true(X_0))^2 at the single point problem.X_0 (Fokker-Planck) --, or 'l2' -- a fresh
    X_2 = rand(K, d) drawn BEFORE the boundary batch, hat(m) + 0.01 (m - 1)^2 with m = mean(V(X_2)^2) and
    hat(x) = exp(-200 x^2) 1[|x| < 0.2] (Schroedinger).
The loop draws xi before it tests whether every trajectory has stopped, exactly like EllipticSolver.

Execution plans, resolved in ``train()``: native (plan_eigen_native.py: rollout, its backward and V's Adam on the HIP kernels of
csrc/genl_kernels.h; the K_boundary- and K-sized boundary / normalisation terms by torch autograd) or composite (this file: the
notebooks' op sequence on torch autograd, used on the CPU and whenever the native plan declines).
"""
import time
import warnings

import numpy as np
import torch

try:
    from .function_space import DenseNet, SingleParam
    from .general_solver import EllipticSolver, _owns_parameters
except ImportError:
    from function_space import DenseNet, SingleParam
    from general_solver import EllipticSolver, _owns_parameters


def hat_function(x):
    """exp(-200 x^2) on |x| < 0.2, zero outside (the Schroedinger notebooks' penalty against the zero function)."""
    return torch.exp(-200 * x ** 2) * ((x > -0.2) & (x < 0.2))


def sample_periodic_pair_host(pb, Kb, d):
    """A boundary batch and its reflection through the box, drawn on the host in the notebooks' order: the 'square' boundary's
    np.random.shuffle and rand(Kb, d) draws; the picked coordinate sits on X_l (first half) / X_r (second half) in the batch and
    on the opposite face in the reflection."""
    half = int(Kb / 2)
    pick = np.concatenate([np.ones(half)[:, np.newaxis], np.zeros([half, d - 1])], 1)
    np.apply_along_axis(np.random.shuffle, 1, pick)
    lower = torch.tensor(np.concatenate([pick, np.zeros([half, d])]).astype(float)).bool()
    upper = torch.tensor(np.concatenate([np.zeros([half, d]), pick]).astype(float)).bool()
    Xb = (pb.X_r - pb.X_l) * torch.rand(Kb, d) + pb.X_l
    Xr = Xb.clone()
    Xb[lower] = pb.X_l
    Xr[lower] = pb.X_r
    Xb[upper] = pb.X_r
    Xr[upper] = pb.X_l
    return Xb, Xr


def periodic_terms(V, Xb, Xr):
    """(mean((V(X_b) - V(X_b'))^2), mean((grad V(X_b) - grad V(X_b'))^2)), both differentiable in V's parameters."""
    value = torch.mean((V(Xb).squeeze() - V(Xr).squeeze()) ** 2)
    Xb = Xb.detach().clone().requires_grad_(True)
    Xr = Xr.detach().clone().requires_grad_(True)
    grad_r, = torch.autograd.grad(V(Xr).squeeze().sum(), Xr, create_graph=True)
    grad_b, = torch.autograd.grad(V(Xb).squeeze().sum(), Xb, create_graph=True)
    return value, torch.mean((grad_b - grad_r) ** 2)


class EigenvalueSolver(EllipticSolver):
    LOGS = ('loss_log', 'loss_log_center', 'loss_log_boundary', 'loss_log_derivative_boundary', 'loss_log_domain', 'V_L2_log',
            'lambda_log', 'K_log', 'times')

    def __init__(self, problem, name, seed=42, delta_t=0.001, N=20, lr=0.001, lambda_init=0.5, lambda_lr=0.01, L=100000, K=500,
                 K_boundary=50, alpha=[50.0, 1.0], normalisation='center', print_every=100, verbose=True, device=None,
                 backend='auto', noise='reference', range_guard=True):
        if normalisation not in ('center', 'l2'):
            raise ValueError("normalisation must be 'center' or 'l2', got %r" % (normalisation,))
        if noise not in ('reference', 'philox'):
            raise ValueError("noise must be 'reference' or 'philox'")
        super().__init__(problem, name, seed=seed, delta_t=delta_t, N=N, lr=lr, L=L, K=K, K_boundary=K_boundary, alpha=alpha,
                         adaptive_forward_process=False, detach_forward=True, print_every=print_every, verbose=verbose,
                         approx_method='skip', loss_method='diffusion', device=device, backend=backend, noise=noise,
                         mlp_dtype='fp32', range_guard=range_guard)
        self.approx_method = 'Y'
        self.normalisation = normalisation
        # the Fokker-Planck notebook's net; `model.V = ...` swaps in another, as with the other solvers
        self.V = DenseNet(d_in=self.d, d_out=1, lr=lr, arch=[10, 10, 10, 10], seed=seed, output_relu=True, bias_init=0.8).to(self.device)
        self.lambda_ = SingleParam(lr=lambda_lr, initial=float(lambda_init), seed=seed).to(self.device)
        self.loss_log_center, self.loss_log_derivative_boundary = [], []

    # ---- scope --------------------------------------------------------------------------------------------------------------
    def _check_scope(self):
        pb = self.problem
        if getattr(pb, 'boundary', None) != 'square' or getattr(pb, 'one_boundary', False):
            raise NotImplementedError("EigenvalueSolver runs on the two-sided box (boundary='square', one_boundary=False)")
        if self.normalisation == 'center' and not hasattr(pb, 'v_true'):
            raise NotImplementedError("normalisation='center' needs problem.v_true")

    def train_PINN(self):
        raise NotImplementedError('the PINN loss is not built for EigenvalueSolver')

    # ---- the pieces both plans share: every draw in the notebooks' order ---------------------------------------------------
    def _normalisation_term(self, gen=None):
        """(term of the loss, c) with ``center_scale * c.item()`` the value the notebooks log as loss_log_center (the 'l2' notebooks
        scale the fp32 number by 0.01 on the host).  'l2' draws X_2 = rand(K, d) -- from the CPU generator, or from the device
        generator `gen` (noise='philox')."""
        pb, dev = self.problem, self.device
        if self.normalisation == 'center':
            Xc = pb.X_0.repeat(1, 1).to(dev)
            term = torch.mean((self.V(Xc).squeeze() - pb.v_true(Xc).squeeze()) ** 2)
            return term, term.detach()
        if gen is None:
            X2 = (pb.X_r - pb.X_l) * torch.rand(self.K, self.d).to(dev) + pb.X_l
        else:
            X2 = (pb.X_r - pb.X_l) * torch.rand(self.K, self.d, generator=gen, device=dev) + pb.X_l
        # (V(X_2) is evaluated once per use, as the notebooks write it: the backward then sums the branches in their order)
        term = 1.0 * hat_function(torch.mean(self.V(X2).squeeze() ** 2))
        term = term + 0.01 * (torch.mean(self.V(X2).squeeze() ** 2) - 1) ** 2
        return term, ((torch.mean(self.V(X2).squeeze() ** 2) - 1) ** 2).detach()

    @property
    def center_scale(self):
        return 1.0 if self.normalisation == 'center' else 0.01

    def _sample_periodic_pair(self):
        Xb, Xr = sample_periodic_pair_host(self.problem, self.K_boundary, self.d)
        return Xb.to(self.device), Xr.to(self.device)

    # ---- plans --------------------------------------------------------------------------------------------------------------
    def train(self):
        torch.manual_seed(self.seed)                              # (the notebooks do not seed; the goldens seed the same way)
        np.random.seed(self.seed)
        self._check_scope()
        plan = self._choose_plan()
        if plan is not None:
            return plan.train()
        self._train_composite()

    def _plan_key(self):
        return super()._plan_key() + (self.normalisation, id(self.lambda_))

    def _choose_plan(self):
        if self.backend == 'torch':
            self.plan_name, self.plan_reason = 'torch', "backend='torch' requested"
            return None
        try:
            from . import plan_eigen_native as pen
        except ImportError:
            import plan_eigen_native as pen
        reason = pen.eigen_eligibility(self)
        if reason is None:
            self.plan_name, self.plan_reason = 'native', None
            plan = getattr(self, '_gen_plan', None)
            key = self._plan_key()
            if plan is None or plan.net is not self.V or plan.key != key or not _owns_parameters(plan):
                plan = pen.EigenDeepPlan(self)
                plan.key = key
                self._gen_plan = plan
            return plan
        if self.backend == 'native':
            raise NotImplementedError('native plan unavailable: ' + reason)
        if self.device.type == 'cuda':
            warnings.warn('path-space EigenvalueSolver: running the composite torch plan (%s)' % reason)
        self.plan_name, self.plan_reason = 'torch', reason
        return None

    def composite_iteration(self):
        """One iteration of the notebooks' loop up to the loss: returns (loss, parts) with parts = dict(center, boundary,
        derivative_boundary, domain, V_L2, K_count) as tensors / numbers; nothing is stepped or logged."""
        pb, dev, dt, sq = self.problem, self.device, self.delta_t, self.sq_delta_t
        d, K = self.d, self.K
        norm, center = self._normalisation_term()
        Xb, Xr = self._sample_periodic_pair()
        t_val, t_grad = periodic_terms(self.V, Xb, Xr)
        loss = norm + self.alpha[1] * t_val + self.alpha[1] * t_grad
        X = ((pb.X_r - pb.X_l) * torch.rand(K, d).to(dev) + pb.X_l).requires_grad_(True)
        Y = torch.zeros(K).to(dev)
        stopped = torch.zeros(K).bool().to(dev)
        V_L2 = torch.zeros(K)
        phi_0 = self.V(X).squeeze()
        K_count = 0
        for n in range(self.N):
            V_now = self.V(X)
            Z, = torch.autograd.grad(V_now.squeeze().sum(), X, create_graph=True)
            sig = pb.sigma(X)
            Z = torch.mm(sig.t(), Z.t()).t()
            xi = torch.randn(K, d).to(dev)                       # drawn before the all-stopped test, as in EllipticSolver
            alive_b = ~stopped
            if int(torch.sum(alive_b)) == 0:
                break
            if hasattr(pb, 'v_true'):
                V_L2[alive_b.cpu()] += ((self.V(X[alive_b]).squeeze() - pb.v_true(X[alive_b].detach()).float().squeeze()) ** 2
                                        ).detach().cpu() * self.delta_t_np
            alive = alive_b.float().unsqueeze(1).repeat(1, d)
            X_prop = X + (pb.b(X) * dt + torch.mm(sig, xi.t()).t() * sq) * alive
            inside = torch.all((X_prop >= pb.X_l) & (X_prop <= pb.X_r), 1)
            act = inside & ~stopped
            actf = act.float()
            Y = Y + ((-pb.h(X, V_now.squeeze(), Z) - self.lambda_(X) * V_now.squeeze()) * dt + torch.sum(Z * xi, 1) * sq) * actf
            X = (X * (~inside | stopped).float().unsqueeze(1).repeat(1, d) + X_prop * actf.unsqueeze(1).repeat(1, d))
            K_count = K_count + int(torch.sum(act))
            stopped = stopped | (~inside & ~stopped)
        domain = torch.mean((self.V(X).squeeze() - phi_0 - Y) ** 2)
        loss = loss + self.alpha[0] * domain
        return loss, dict(center=center, boundary=t_val, derivative_boundary=t_grad, domain=domain,
                          V_L2=torch.mean(V_L2).item(), K_count=K_count)

    def _train_composite(self):
        for l in range(self.L):
            t_0 = time.time()
            loss, parts = self.composite_iteration()
            self.V.zero_grad()
            self.lambda_.zero_grad()
            loss.backward()
            self.V.optim.step()
            self.lambda_.optim.step()                             # after V, as in the notebooks
            self.loss_log.append(loss.item())
            self.loss_log_center.append(self.center_scale * parts['center'].item())
            self.loss_log_boundary.append(parts['boundary'].item())
            self.loss_log_derivative_boundary.append(parts['derivative_boundary'].item())
            self.loss_log_domain.append(parts['domain'].item())
            self.V_L2_log.append(parts['V_L2'])
            self.K_log.append(parts['K_count'])
            self.lambda_log.append(self.lambda_.Y_0[0].item())   # after the step
            self.times.append(time.time() - t_0)
            if self.verbose and l % self.print_every == 0:
                print('%d - loss = %.4e, v L2 error = %.4e, lambda = %.4e, %.2f'
                      % (l, self.loss_log[-1], self.V_L2_log[-1], self.lambda_log[-1], np.mean(self.times[-self.print_every:])))
