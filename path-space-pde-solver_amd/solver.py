"""Solver: path-space training loop for HJB / semilinear PDE problems -- API mirror of the
reference's ``solver.Solver`` (reference solver.py:18-557), MI355X-native underneath.

Same constructor keywords, attributes (``loss_log, u_L2_loss, Y_0_log, times, z_n, y_0, Phis,
p, N, K, L, lr, delta_t, delta_t_np, sq_delta_t, device, ...``) and methods (``train, Z_n, Z_n_,
update_Phis, b, sigma, h, f, g, zero_grad, optimization_step, save_networks, load_networks,
save_logs``) as the reference, so notebooks written against it run unchanged, including
``model.z_n = OtherNet(...); model.update_Phis()``.

``train()`` resolves every string switch ONCE into an execution plan:

* native plan (plan_native.HjbNativePlan): hand-written HIP kernels behind the C ABI of
  include/psp.h; used whenever (problem, net, loss, flags) is in the native catalogue.
* composite plan (this file): the reference's op sequence restated with torch ops on
  ``self.device`` for combinations outside the catalogue (other nets, ``time_approx='outer'``,
  other losses, ``detach_forward=False``, per-step ``u_true`` logging).

Extra keywords (all optional, appended after the reference's): ``device``, ``backend``
('auto' | 'native' | 'torch'), ``noise`` ('reference' = the reference's CPU-generator stream,
bit-compatible with its fixed-seed runs; 'philox' = on-device counter-based stream),
``widths`` (hidden widths of the default control net; the reference hard-codes [30, 30]),
``path_budget_bytes`` / ``path_chunks`` / ``chunk_mode`` (K-chunking of the native plan when the path store
would not fit in HBM; the reference holds the whole autograd graph instead).
"""
import json
import os
import math
import time
import warnings
from copy import deepcopy
from datetime import date

import numpy as np
import torch

try:
    from .function_space import DenseNet, MySequential, SingleParam
    from .plan_native import HjbNativePlan, PlanUnsupported, native_eligibility
    from .plan_dense_native import DenseNativePlan, dense_eligibility
    from .plan_value_native import ValueNativePlan, value_eligibility
    from .plan_affine_native import AffineNativePlan, affine_eligibility, control_class
    from . import native as _nat
    from .general_solver import GeneralSolver, EllipticSolver  # noqa: F401  (reference: `from solver import GeneralSolver`)
    from .utilities import do_importance_sampling_me
except ImportError:  # flat import: this directory itself is on sys.path, as with the reference
    from function_space import DenseNet, MySequential, SingleParam
    from plan_native import HjbNativePlan, PlanUnsupported, native_eligibility
    from plan_dense_native import DenseNativePlan, dense_eligibility
    from plan_value_native import ValueNativePlan, value_eligibility
    from plan_affine_native import AffineNativePlan, affine_eligibility, control_class
    import native as _nat
    from general_solver import GeneralSolver, EllipticSolver  # noqa: F401
    from utilities import do_importance_sampling_me


def _default_device():
    return torch.device('cuda' if torch.cuda.is_available() else 'cpu')


class Solver:

    def __init__(self, name, problem, lr=0.001, L=10000, K=50, delta_t=0.05,
                 approx_method='control', loss_method='log-variance', time_approx='outer',
                 learn_Y_0=False, adaptive_forward_process=True, detach_forward=False,
                 early_stopping_time=10000, random_X_0=False, compute_gradient_variance=0,
                 IS_variance_K=0, IS_variance_iter=1, metastability_logs=None, print_every=100,
                 plot_trajectories=None, seed=42, save_results=False, u_l2_error_flag=True,
                 log_gradient=False, burgers_drift=False, verbose=True,
                 device=None, backend='auto', noise='reference', widths=(30, 30), mlp_dtype='auto',
                 path_budget_bytes=None, path_chunks=None, chunk_mode='auto', use_graph='auto', range_guard=True,
                 path_noise='auto', state_basis='auto', value_state_path='torch', IS_wide_states='torch'):
        self.problem, self.name = problem, name
        self.date = date.today().strftime('%Y-%m-%d')
        self.d, self.T = problem.d, problem.T
        self.device = torch.device(device) if device is not None else getattr(problem, 'device', _default_device())
        self.X_0 = torch.as_tensor(problem.X_0, dtype=torch.float32).to(self.device)
        self.Y_0 = torch.tensor([0.0])
        self.X_u_opt = None
        if backend not in ('auto', 'native', 'torch'):
            raise ValueError("backend must be 'auto', 'native' or 'torch'")
        if noise not in ('reference', 'philox'):
            raise ValueError("noise must be 'reference' or 'philox'")
        self.backend, self.noise = backend, noise
        if mlp_dtype not in ('auto', 'fp32', 'bf16', 'f16x3'):
            raise ValueError("mlp_dtype must be 'auto', 'fp32', 'f16x3' or 'bf16'")
        # matrix products of the native HJB kernels: 'fp32' (fp32 MFMA), 'f16x3' (fp32-grade split products on the f16 matrix pipe,
        # same parity bounds, ~1.8x faster at large K), 'auto' (f16x3 where it exists and pays, plan_native.py); 'bf16': control-net
        # products of the forward rollout on bf16 MFMA (opt-in, own tolerance)
        self.mlp_dtype = mlp_dtype
        # split-product kernels: operands must stay below 65504 (f16 range).  range_guard=True (default) lets the library redo an
        # iteration on the fp32-MFMA kernels when an operand left that range (device-side flag + predicated launches, no host
        # sync; include/psp.h: range_flag), so that 'auto' / 'f16x3' never return a non-finite loss where 'fp32' is finite.
        # self.range_fallback_iterations counts them after train()
        self.range_guard = bool(range_guard)
        self.range_fallback_iterations = 0
        # path store of the native plan: 'auto' lets the backward regenerate the Brownian increments from the Philox counters
        # where that is exact (detached adaptive process, on-device noise, narrow kernel family: 960 instead of 1408 B per
        # trajectory-timestep at d = 100); 'store' always keeps them (psp_hjb_config.store_path 1 instead of 4)
        if path_noise not in ('auto', 'store'):
            raise ValueError("path_noise must be 'auto' or 'store'")
        self.path_noise = path_noise
        # native plan: 'auto' rolls the state out as B^-1 X (one d x d product per step instead of two) where that is exact and
        # well conditioned -- dense drift and sigma, linear terminal cost, fixed X_0, detached, d <= 112, cond_2(B) <= 4
        # (plan_native.py: state_basis_decision); 'x' never, 'sigma' raises where 'auto' would decline.  Parameters, gradients
        # and every logged quantity stay in the original basis.
        if state_basis not in ('auto', 'x', 'sigma'):
            raise ValueError("state_basis must be 'auto', 'x' or 'sigma'")
        self.state_basis = state_basis
        # value-function ansatz with adaptive_forward_process=True and detach_forward=False (gradients through the state path):
        # 'torch' (default) runs the composite plan, 'native' the adjoint sweep of the run-time-shaped value-net kernels between
        # their forward and backward (plan_value_native.py, csrc/genl_adj_kernels.h)
        if value_state_path not in ('torch', 'native'):
            raise ValueError("value_state_path must be 'torch' or 'native'")
        self.value_state_path = value_state_path
        # the in-loop importance-sampling log above d = 64 (utilities.do_importance_sampling_me wide_states): 'torch' (default) keeps
        # the composite evaluation of a Linear / Constant list there, 'native' runs it on psp_isw_rollout.  No plan reads it.
        if IS_wide_states not in ('torch', 'native'):
            raise ValueError("IS_wide_states must be 'torch' or 'native'")
        self.IS_wide_states = IS_wide_states
        # native plan: HBM budget of the path store kept for the backward pass (None: a third of the HBM); a larger store is
        # processed in K-chunks (plan_native.py).  path_chunks forces a chunk count; chunk_mode 'auto' | 'two_gradient' | 'recompute'
        self.path_budget_bytes, self.path_chunks, self.chunk_mode = path_budget_bytes, path_chunks, chunk_mode
        # native plan: replay the iteration as a captured hipGraph ('auto': when it is launch-bound, K <= 8192 on MI355X)
        self.use_graph = use_graph

        # hyper-parameters (reference solver.py:36-45): fp32 step, float64 step count
        self.seed = seed
        self.delta_t_np = delta_t
        self.delta_t = torch.tensor(self.delta_t_np).to(self.device)
        self.sq_delta_t = torch.sqrt(self.delta_t).to(self.device)
        self.N = int(np.floor(self.T / self.delta_t_np))
        self.lr, self.L, self.K = lr, L, K
        self.random_X_0 = random_X_0

        self.loss_method = loss_method
        self.approx_method = approx_method
        self.learn_Y_0 = learn_Y_0
        self.adaptive_forward_process = adaptive_forward_process
        self.detach_forward = detach_forward
        self.early_stopping_time = early_stopping_time
        self.burgers_drift = burgers_drift

        self.has_ref_solution = hasattr(problem, 'u_true')
        self.u_l2_error_flag = u_l2_error_flag and self.has_ref_solution
        if self.loss_method == 'relative_entropy':       # the two silent overrides of solver.py:61-64
            self.adaptive_forward_process = True
        if self.loss_method == 'cross_entropy':
            self.learn_Y_0 = False

        self.print_every, self.verbose, self.verbose_NN = print_every, verbose, False
        self.save_results = save_results
        self.compute_gradient_variance = compute_gradient_variance
        self.IS_variance_K, self.IS_variance_iter = IS_variance_K, IS_variance_iter
        self.metastability_logs = metastability_logs
        self.plot_trajectories = plot_trajectories
        self.log_gradient = log_gradient
        self.print_gradient_norm = False

        # ansatz spaces (solver.py:80-99); seeds as in the reference so initial weights agree
        self.Phis = []
        self.time_approx = time_approx
        torch.manual_seed(seed)
        if self.approx_method == 'control':
            self.y_0 = SingleParam(lr=self.lr).to(self.device)
            if self.time_approx == 'outer':
                self.z_n = [DenseNet(d_in=self.d, d_out=self.d, lr=self.lr, seed=seed) for _ in range(self.N)]
            elif self.time_approx == 'inner':
                self.z_n = MySequential(d_in=self.d + 1, d_out=self.d, lr=self.lr, seed=123, widths=widths)
        elif self.approx_method == 'value_function':
            if self.time_approx == 'outer':
                self.y_n = [DenseNet(d_in=self.d, d_out=1, lr=self.lr, seed=seed) for _ in range(self.N)]
            elif self.time_approx == 'inner':
                self.y_n = [DenseNet(d_in=self.d + 1, d_out=1, lr=self.lr, seed=seed)]
        self.update_Phis()
        for phi in self.Phis:
            phi.train()

        self.Y_0_log, self.loss_log, self.u_L2_loss = [], [], []
        self.IS_rel_log, self.times = [], []
        self.grads_rel_error_log, self.particles_close_to_target = [], []
        self.plan_name = None        # 'native' | 'torch', set by train()
        self.plan_reason = None      # why the composite plan was chosen (if it was)

    # ---- problem pass-throughs (solver.py:121-140) ------------------------------------------
    def b(self, x):
        return self.problem.b(x)

    def sigma(self, x):
        return self.problem.sigma(x)

    def h(self, t, x, y, z):
        return self.problem.h(t, x, y, z)

    def f(self, x, t):
        return self.problem.f(x, t)

    def g(self, x):
        return self.problem.g(x)

    def u_true(self, x, t):
        return self.problem.u_true(x, t)

    def v_true(self, x, t):
        return self.problem.v_true(x, t)

    # ---- ansatz bookkeeping -------------------------------------------------------------------
    def update_Phis(self):
        """Collect the trainable modules (solver.py:142-162); call after swapping ``z_n``."""
        if self.approx_method == 'control':
            nets = list(self.z_n) if self.time_approx == 'outer' else [self.z_n]
            self.Phis = nets + ([self.y_0] if self.learn_Y_0 else [])
        elif self.approx_method == 'value_function':
            self.Phis = self.y_n
        for phi in self.Phis:
            phi.to(self.device)
        self.p = sum(int(np.prod(q.size())) for q in self.Phis[0].parameters() if q.requires_grad)
        if self.log_gradient:
            self.gradient_log = torch.zeros(self.L, self.p)

    def zero_grad(self):
        for phi in self.Phis:
            phi.optim.zero_grad()

    def optimization_step(self):
        for phi in self.Phis:
            phi.optim.step()

    # ---- control evaluation (solver.py:334-362) -----------------------------------------------
    def Y_n(self, X, t):
        if self.time_approx == 'outer':
            n = int(torch.ceil(torch.as_tensor(t / self.delta_t)).item())     # (np.ceil of a device tensor fails on a GPU)
            return self.y_n[n](X)
        t_X = torch.cat([torch.ones([X.shape[0], 1]).to(X.device) * t, X], 1)
        return self.y_n[0](t_X)

    def compute_grad_Y(self, X, n):
        total = self.Y_n(X, n).squeeze(1).sum()
        grad, = torch.autograd.grad(total, X, create_graph=True)
        return torch.mm(self.sigma(X), grad.t()).t()

    def Z_n_(self, X, n):
        if self.approx_method == 'value_function':
            return self.compute_grad_Y(X, n)
        if self.time_approx == 'outer':
            return self.z_n[max(0, min(n, self.N - 1))](X)
        t_col = torch.ones([X.shape[0], 1]).to(self.device) * n * self.delta_t   # time is input column 0
        return self.z_n(torch.cat([t_col, X], 1))

    def Z_n(self, X, t):
        t = torch.as_tensor(t, dtype=torch.float32, device=self.delta_t.device)
        n = int(torch.ceil(t / self.delta_t))
        return self.Z_n_(X, n)

    # ---- losses (solver.py:164-192) -----------------------------------------------------------
    def loss_function(self, X, Y, Z_sum, l):
        m = self.loss_method
        if m in ('moment', 'log-variance', 'log-variance-repa') or (m == 'relative_entropy_log-variance' and l >= 1000):
            D = Y - self.g(X)
            if m == 'moment':
                return D.pow(2).mean()
            var = D.pow(2).mean() - D.mean().pow(2)
            return (l % 2 * 2 - 1) * var if m == 'log-variance-repa' else var
        if m == 'variance':
            return torch.var(torch.exp(-self.g(X) + Y))
        if m in ('relative_entropy', 'relative_entropy_BSDE', 'reparametrization', 'relative_entropy_log-variance'):
            return (Z_sum + self.g(X)).mean()
        if m == 'cross_entropy':
            w = torch.exp(-self.g(X) + Y.detach()) if self.adaptive_forward_process else torch.exp(-self.g(X))
            return (Y * w).mean()
        raise NotImplementedError('loss_method %r' % m)

    def gradient_descent(self, X, Y, Z_sum, l, additional_loss):
        self.zero_grad()
        loss = self.loss_function(X, Y, Z_sum, l) + additional_loss
        loss.backward()
        self.optimization_step()
        return loss

    # ---- per-sample gradient moments (solver.py:225-281) --------------------------------------
    def flatten_gradient(self, k, grads, grads_flat):
        """Row k of ``grads_flat`` <- the tensors of ``grads`` flattened one after the other; returns ``grads_flat``."""
        grads = [g.reshape(-1) for g in grads]
        if grads:
            row = torch.cat(grads)
            grads_flat[k, :row.numel()] = row
        return grads_flat

    def get_gradient_variances(self, X, Y):
        """The reference's gradient-variance diagnostic, composite plan: for every net n of ``z_n`` the per-trajectory loss
        gradients f_k (K rows of p entries), their mean and unbiased variance over k, and sqrt(var) / mean with NaN -> 0 (inf and
        negative values stay).  Returns the (N, p) matrix; train() logs its mean.  Two quirks of the reference are kept: the
        terminal-cost gradient is taken at trajectory 0 for every k, and the nets other than z_n[n] are ignored.
        Deliberate difference: the (K, p) work tensors live on self.device (the reference's are CPU tensors, which makes its own
        assignments fail on a GPU run).  adaptive_forward_process with detach_forward=True raises autograd's RuntimeError, as in
        the reference (g(X_N) does not depend on the parameters there)."""
        if self.approx_method != 'control' or self.time_approx != 'outer':
            raise NotImplementedError("compute_gradient_variance needs a control net per time step (time_approx='outer'), "
                                      "as in the reference")
        if self.loss_method not in ('moment', 'log-variance'):
            raise NotImplementedError("compute_gradient_variance is defined for loss_method 'moment' and 'log-variance' only "
                                      "(the reference fails on %r)" % self.loss_method)
        dev = self.device
        grads_mean = torch.zeros(self.N, self.p, device=dev)
        grads_var = torch.zeros(self.N, self.p, device=dev)
        resid = (Y - self.g(X)).detach().unsqueeze(1)
        for n in range(self.N):
            theta = [q for q in self.z_n[n].parameters() if q.requires_grad]
            G = torch.zeros(self.K, self.p, device=dev)
            for k in range(self.K):
                gk = torch.autograd.grad(Y[k], theta, retain_graph=True, allow_unused=True)
                G = self.flatten_gradient(k, [g for g in gk if g is not None], G)
            if self.adaptive_forward_process:
                g0 = torch.autograd.grad(self.g(X[0, :].unsqueeze(0)).sum(), theta, retain_graph=True, allow_unused=True)
                row = self.flatten_gradient(0, [g for g in g0 if g is not None], torch.zeros(1, self.p, device=dev))
                G = G - row                    # row 0 for every k
            if self.loss_method == 'moment':
                f = 2 * resid * G
            else:
                f = 2 * (resid - resid.mean(0, keepdim=True)) * (G - G.mean(0, keepdim=True))
            grads_mean[n, :] = f.mean(0)
            grads_var[n, :] = f.var(0)
        rel = torch.sqrt(grads_var) / grads_mean
        rel[rel != rel] = 0
        return rel

    def initialize_training_data(self):
        """Initial state, accumulators and the iteration's Brownian increments drawn on the CPU
        generator and moved to the device (solver.py:364-382)."""
        K, dev = self.K, self.device
        X = self.X_0.repeat(K, 1).to(dev)
        if self.random_X_0:
            X = torch.randn(K, self.d).to(dev)
        Y = self.Y_0.repeat(K).to(dev)
        if self.approx_method == 'value_function':
            X = X.clone().requires_grad_(True)
            Y = self.Y_n(X, 0)[:, 0]
        elif self.learn_Y_0:
            Y = self.y_0(X)
            self.Y_0_log.append(Y[0].item())
        zeros = [torch.zeros(K).to(dev) for _ in range(5)]
        xi = torch.randn(K, self.d, self.N + 1).to(dev)
        return (X, Y, *zeros, xi)

    # ---- training -----------------------------------------------------------------------------
    def _plan_key(self):
        """Everything a native plan sizes its buffers / fixes its kernel configuration from: a plan built for other values
        must not be reused (the nets themselves are compared by identity)."""
        nets = tuple(id(z) for z in self.z_n) if isinstance(getattr(self, 'z_n', None), list) else (id(getattr(self, 'z_n', None)),)
        nets = nets + tuple(id(v) for v in getattr(self, 'y_n', []))
        return (nets, self.noise, self.K, self.N, float(self.delta_t_np), self.loss_method, self.approx_method,
                self.time_approx, bool(self.learn_Y_0), bool(self.adaptive_forward_process), bool(self.detach_forward),
                bool(self.random_X_0), bool(self.u_l2_error_flag), self.mlp_dtype, getattr(self, 'range_guard', True), getattr(self, 'path_noise', 'auto'), getattr(self, 'state_basis', 'auto'), getattr(self, 'value_state_path', 'torch'), os.environ.get('PSP_STATE_BASIS', ''), self.path_budget_bytes, self.path_chunks,
                self.chunk_mode, id(self.problem), id(self.y_0) if hasattr(self, 'y_0') else None)

    def _choose_plan(self):
        """The execution plan of train(): a native plan object, or None for the composite torch plan.  A native plan that turns
        out not to cover the configuration while it is being built (PlanUnsupported from a constructor: e.g. mlp_dtype='bf16'
        with a DenseNet control, an Adam with weight decay) falls back to the composite plan under backend='auto' like every
        other out-of-catalogue combination (never an error); backend='native' raises."""
        try:
            return self._choose_plan_checked()
        except PlanUnsupported as e:
            if self.backend == 'native':
                raise
            if self.device.type == 'cuda':
                warnings.warn('path-space solver: running the composite torch plan (%s)' % e)
            self.plan_name, self.plan_reason = 'torch', str(e)
            self._native_plan = None
            return None

    def _native_plan_of(self, cls):
        """The solver's plan of class `cls`: the cached one if it was built for the present configuration, else a new one."""
        self.plan_name, self.plan_reason = 'native', None
        plan = getattr(self, '_native_plan', None)
        if plan is None or not isinstance(plan, cls) or getattr(plan, 'key', None) != self._plan_key():
            plan = cls(self, noise=self.noise)
            plan.key = self._plan_key()
            self._native_plan = plan
        if cls is HjbNativePlan:
            self.plan_reason = 'state basis %s: %s' % (plan.state_basis, plan.state_basis_reason)
        return plan

    def _choose_plan_checked(self):
        if self.backend == 'torch':
            self.plan_name, self.plan_reason = 'torch', "backend='torch' requested"
            return None
        z = getattr(self, 'z_n', None)                  # (approx_method='value_function' has y_n instead)
        value = self.approx_method == 'value_function'
        # the native plans in the order they are asked: (eligibility, plan class, is this configuration asked about it at all)
        chain = (
            # value-net ansatz (solver.py:93-97, 334-339, 438-440): the GeneralSolver kernels with per-sample weights
            (value_eligibility, ValueNativePlan, value),
            # (raises NativeLibraryError if the .so is missing on a GPU run; the plan owns the flat parameters and Adam moments)
            (native_eligibility, HjbNativePlan, not value),
            # DenseNet controls: time_approx='outer', DenseNet swapped into z_n
            (dense_eligibility, DenseNativePlan, not value),
            # a list of Linear / Affine / Constant modules, one per time step
            (affine_eligibility, AffineNativePlan, not value and control_class(z) is not None),
        )
        reason = None
        for eligibility, cls, asked in chain:
            if not asked:
                continue
            why = eligibility(self)
            if why is None:
                return self._native_plan_of(cls)
            # the reason reported is that of the last class asked, except that the DenseNet plan speaks only for a list or a DenseNet
            if cls is not DenseNativePlan or isinstance(z, list) or isinstance(z, DenseNet):
                reason = why
        if self.backend == 'native':
            raise PlanUnsupported('native plan unavailable: ' + reason)
        if self.device.type == 'cuda':
            warnings.warn('path-space solver: running the composite torch plan (%s)' % reason)
        self.plan_name, self.plan_reason = 'torch', reason
        return None

    def train(self):
        torch.manual_seed(self.seed)
        if self.verbose:
            print('d = %d, L = %d, K = %d, delta_t = %.2e, lr = %.2e, %s, %s, %s, %s'
                  % (self.d, self.L, self.K, self.delta_t_np, self.lr, self.approx_method,
                     self.time_approx, self.loss_method, 'adaptive' if self.adaptive_forward_process else ''))
        plan = self._choose_plan()
        if plan is not None:
            self._train_native(plan)
        else:
            self._train_composite()
        if self.save_results:
            self.save_logs()

    def _train_native(self, plan):
        """L iterations on the HIP plan.  Nothing synchronises with the host inside the loop
        (the reference syncs every iteration through loss.item(), solver.py:514); losses are
        gathered on the device and read back once per print_every block."""
        losses = torch.zeros(self.L, dtype=torch.float32, device=self.device)
        ul2 = torch.zeros(self.L, dtype=torch.float32, device=self.device) if self.u_l2_error_flag else None
        y0_hist = torch.zeros(self.L, dtype=torch.float32, device=self.device) if self.learn_Y_0 else None
        done = 0
        gv_done = 0
        if self.compute_gradient_variance > 0 and hasattr(plan, 'begin_gradient_log'):
            plan.begin_gradient_log(self.L)          # mean(sqrt(var) / mean) of the per-sample gradients, one device slot per logged l
        t_block = time.time()
        for l in range(self.L):
            if self.learn_Y_0:
                y0_hist[l:l + 1].copy_(self.y_0.Y_0.detach())       # Y_0 before the update (solver.py:374)
            plan.iteration(l, losses, ul2)
            if self.IS_variance_K > 0 and l % self.IS_variance_iter == 0:        # solver.py:521-528
                self.IS_rel_log.append(do_importance_sampling_me(self.problem, self, self.IS_variance_K,
                                                                 wide_states=self.IS_wide_states)[2])
            # early stopping reads the u_L2 log every iteration once l > early_stopping_time (solver.py:550-554)
            watch = ul2 is not None and self.early_stopping_time is not None and l > self.early_stopping_time
            if (self.verbose and l % self.print_every == 0) or l == self.L - 1 or watch:
                vals = losses[done:l + 1].cpu().tolist()          # one sync per block
                if getattr(plan, 'matrix_mode', 'fp32') == 'f16x3' and getattr(plan, 'range_flag', None) is None \
                        and not getattr(self, '_warned_range', False) and not all(math.isfinite(v) for v in vals):
                    import warnings
                    self._warned_range = True
                    warnings.warn("non-finite loss on the UNGUARDED split-product kernels (range_guard=False): their operands must "
                                  "stay below 65504 in magnitude (f16 range); use range_guard=True or mlp_dtype='fp32'")
                now = time.time()
                per = (now - t_block) / max(1, l + 1 - done)
                self.loss_log += vals
                self.u_L2_loss += ul2[done:l + 1].cpu().tolist() if ul2 is not None else [0.0] * len(vals)
                self.times += [per] * len(vals)
                if self.learn_Y_0:
                    self.Y_0_log += y0_hist[done:l + 1].cpu().tolist()
                if getattr(plan, 'gv_count', 0) > gv_done:          # read back with the block: no sync of its own
                    self.grads_rel_error_log += plan.gv_log[gv_done:plan.gv_count].cpu().tolist()
                    gv_done = plan.gv_count
                done, t_block = l + 1, now
                if self.verbose and l % self.print_every == 0:
                    msg = '%d - loss: %.4e - u L2: %.4e - time/iter: %.4fs' % (l, self.loss_log[-1], self.u_L2_loss[-1], per)
                    if self.learn_Y_0:
                        msg += ' - Y_0: %.4e' % self.Y_0_log[-1]
                    print(msg)
                if watch:
                    recent = self.u_L2_loss[-self.early_stopping_time:]
                    if np.std(recent) / self.u_L2_loss[-1] < 0.02:
                        break
        if hasattr(plan, 'range_fallbacks'):
            self.range_fallback_iterations = plan.range_fallbacks()
        if hasattr(plan, 'export_optimizer_state'):
            plan.export_optimizer_state()       # phi.optim carries the Adam state, as in the reference (function_space.py:185)

    def _train_composite(self):
        """The reference iteration restated with torch ops on self.device (solver.py:430-554)."""
        if self.approx_method not in ('control', 'value_function'):
            raise NotImplementedError("approx_method %r is not built" % self.approx_method)
        if self.approx_method == 'value_function' and self.time_approx != 'inner':
            # the reference itself fails here: Y_n(X, n) turns the STEP index into ceil(n / delta_t) (solver.py:342-345)
            raise NotImplementedError("approx_method='value_function' needs time_approx='inner' (as in the reference)")
        if self.loss_method == 'log-variance-repa':
            # the reference alternates per iteration between a FROZEN copy of the control in Z (even l) and a detached drift (odd
            # l), solver.py:444-447, 468-469; only the sign flip of its loss (:169-170) is restated here, so refuse rather than
            # train something else under that name
            raise NotImplementedError("loss_method='log-variance-repa' (alternating frozen control / detached drift) is not built")
        dev, dt, sq = self.device, self.delta_t, self.sq_delta_t
        repa = self.loss_method == 'reparametrization'
        rel_ent = 'relative_entropy' in self.loss_method
        for l in range(self.L):
            t_0 = time.time()
            X, Y, Z_sum, u_L2, _, _, _, xi = self.initialize_training_data()
            frozen = deepcopy(self.z_n) if repa else None
            extra = torch.zeros(self.K).to(dev)
            for n in range(self.N):
                if self.approx_method == 'value_function' and n > 0:
                    extra = extra + (self.Y_n(X, n)[:, 0] - Y).pow(2)       # solver.py:438-440
                Z = self.Z_n_(X, n)
                c = torch.zeros(self.d, self.K).to(dev)
                if self.adaptive_forward_process:
                    if self.burgers_drift:
                        c = torch.ones(self.d, self.K).to(dev) * (Y.unsqueeze(0) - (2 + self.d) / (2 * self.d))
                    else:
                        c = -self.Z_n_(X, n).t()           # second evaluation, as the reference does (:456)
                if repa:
                    if self.time_approx == 'outer':
                        v = -deepcopy(self.z_n[max(0, min(n, self.N - 1))])(X)
                    else:
                        v = -frozen(torch.cat([torch.ones([X.shape[0], 1]).to(dev) * n * dt, X], 1))
                if self.detach_forward:
                    c = c.detach()
                dW = xi[:, :, n + 1]
                sig = self.sigma(X)
                X = (X + (self.b(X) + torch.mm(sig, c).t()) * dt + torch.mm(sig, dW.t()).t() * sq)
                # h is evaluated at the UPDATED state with the old Y and time n*dt (:477)
                Y = (Y + (-self.h(dt * n, X, Y, Z) + torch.sum(Z * c.t(), 1)) * dt + torch.sum(Z * dW, 1) * sq)
                if repa:
                    Z_sum = Z_sum + (-0.5 * torch.sum(v ** 2, 1) * dt + torch.sum(v * c.t(), 1) * dt
                                     + torch.sum(v * dW, 1) * sq)
                if rel_ent:
                    Z_sum = Z_sum + (0.5 * torch.sum(Z ** 2, dim=1) + self.f(X, n * dt)) * dt
                    if self.loss_method == 'relative_entropy_BSDE':
                        Z_sum = Z_sum + torch.sum(-Z * dW, 1) * sq
                if self.u_l2_error_flag:
                    ref = torch.tensor(self.u_true(X.cpu().detach(), n * self.delta_t_np)).t().float().to(dev)
                    u_L2 = u_L2 + torch.sum((-Z - ref) ** 2 * dt, 1)
            if self.compute_gradient_variance > 0 and l % self.compute_gradient_variance == 0:      # solver.py:496-497
                self.grads_rel_error_log.append(torch.mean(self.get_gradient_variances(X, Y)).item())
            loss = self.gradient_descent(X, Y, Z_sum, l, extra.mean())
            if self.log_gradient:
                flat = torch.cat([q.grad.reshape(-1) for q in self.z_n.parameters() if q.grad is not None])
                self.gradient_log[l, :] = flat.cpu().detach()
            self.loss_log.append(loss.item())
            self.u_L2_loss.append(torch.mean(u_L2).item())
            if self.metastability_logs is not None:
                target, epsilon = self.metastability_logs
                self.particles_close_to_target.append(
                    torch.mean((torch.sqrt(torch.sum((X - target) ** 2, 1)) < epsilon).float()))
            if self.IS_variance_K > 0 and l % self.IS_variance_iter == 0:        # solver.py:521-528
                self.IS_rel_log.append(do_importance_sampling_me(self.problem, self, self.IS_variance_K,
                                                                 wide_states=self.IS_wide_states)[2])
            self.times.append(time.time() - t_0)
            if self.verbose and l % self.print_every == 0:
                msg = ('%d - loss: %.4e - u L2: %.4e - time/iter: %.2fs'
                       % (l, self.loss_log[-1], self.u_L2_loss[-1], np.mean(self.times[-self.print_every:])))
                if self.learn_Y_0:
                    msg += ' - Y_0: %.4e' % self.Y_0_log[-1]
                print(msg)
            if self.early_stopping_time is not None and l > self.early_stopping_time:
                recent = self.u_L2_loss[-self.early_stopping_time:]
                if np.std(recent) / self.u_L2_loss[-1] < 0.02:
                    break

    # ---- persistence (solver.py:283-332) ------------------------------------------------------
    @staticmethod
    def state_dict_to_list(sd):
        return {k: (v.detach().cpu().numpy().tolist() if isinstance(v, torch.Tensor) else v) for k, v in sd.items()}

    @staticmethod
    def list_to_state_dict(l):
        return {k: (torch.tensor(v) if isinstance(v, list) else v) for k, v in l.items()}

    def save_logs(self, model_name='model'):
        logs = {'name': self.name, 'date': self.date, 'd': self.d, 'T': self.T, 'seed': self.seed,
                'delta_t': self.delta_t_np, 'N': self.N, 'lr': self.lr, 'K': self.K,
                'loss_method': self.loss_method, 'learn_Y_0': self.learn_Y_0,
                'adaptive_forward_process': self.adaptive_forward_process,
                'Y_0_log': self.Y_0_log, 'loss_log': self.loss_log, 'u_L2_loss': self.u_L2_loss,
                'Phis_state_dict': [self.state_dict_to_list(z.state_dict()) for z in self.Phis]}
        os.makedirs('logs', exist_ok=True)
        path, i = 'logs/%s_%s_%s.json' % (model_name, self.name, self.date), 1
        while os.path.isfile(path):
            i += 1
            path = 'logs/%s_%s_%s_%d.json' % (model_name, self.name, self.date, i)
        with open(path, 'w') as fh:
            json.dump(logs, fh, indent=2)

    def save_networks(self):
        os.makedirs('output', exist_ok=True)
        path = 'output/%s_%s.pt' % (self.name, self.date)
        torch.save({'nn%d' % i: z.state_dict() for i, z in enumerate(self.Phis)}, path)
        print('\nnetworks data has been stored to file: %s' % path)

    def load_networks(self, cp_name):
        print('\nload network data from file: %s' % cp_name)
        checkpoint = torch.load(cp_name, map_location=self.device)
        for i, z in enumerate(self.Phis):
            z.load_state_dict(checkpoint['nn%d' % i])
            z.eval()
