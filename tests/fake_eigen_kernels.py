"""TEST INFRASTRUCTURE: a CPU stand-in for the three launches of EigenvalueSolver's native plan (plan_eigen_native.py), in the
pattern of tests/fake_kernels.py.  `FakeEigenKernels` wraps the REAL library (size queries and argument validation stay the
library's own) and answers psp_genl_rollout_fwd_eig / psp_genl_rollout_bwd / psp_adam_step on host tensors, reading the same
structs and raw pointers the HIP kernels would get: forward = the recursion of include/psp.h (psp_genl_eig) in torch fp32, with the
X_n images, the step counts per tile and S_k written where the plan reads them; backward = autograd of sum_k wY_k Y_N,k + wV_k V_N,k.
Only tests import this; nothing here is timed or shipped."""
import ctypes as C
import math

import torch

from fake_kernels import _f32, _val
from util_cases import psp

nat = psp.native


def _i32(ptr, n):
    return torch.frombuffer((C.c_int32 * n).from_address(ptr), dtype=torch.int32)


def _i64(ptr, n):
    return torch.frombuffer((C.c_int64 * n).from_address(ptr), dtype=torch.int64)


class FakeEigenKernels:
    def __init__(self):
        self.real = nat.load()
        self.state = None
        self.calls = []

    def __getattr__(self, name):
        return getattr(self.real, name)

    @staticmethod
    def _net(g, flat, x):
        """(o, params) of the dense-concat net described by the psp_genl_config g on the flat parameters."""
        dims = [g.base.d] + [int(g.widths[i]) for i in range(g.n_hidden)] + [1]
        off, fan = 0, 0
        a = x
        for i in range(len(dims) - 1):
            fan += dims[i]
            out = dims[i + 1]
            W = flat[off:off + fan * out]
            off += fan * out
            W = W.view(out, fan).t() if g.linear_layout else W.view(fan, out)
            b = flat[off:off + out]
            off += out
            z = a @ W + b
            if i == len(dims) - 2:
                return z[:, 0]
            r = torch.relu(z) if g.activation == nat.ACT_RELU2 else torch.tanh(z)
            a = torch.cat([a, r if g.activation == nat.ACT_TANH else r ** 2], 1)

    def psp_genl_rollout_fwd_eig(self, cfg_ref, eig_ref, params, x0, t0, xi, seed, it, tables, path, ahat, VN, YN, XN, tN, kcount,
                                 stream):
        g, e = cfg_ref._obj, eig_ref._obj
        c = g.base
        assert c.noise_mode == nat.NOISE_SUPPLIED and not g.has_time and c.domain_kind == nat.DOM_BOX and not c.adaptive
        sz = nat.GenlSizes()
        assert self.real.psp_genl_query_eig(cfg_ref, eig_ref, C.byref(sz)) == 0, self.real.psp_last_error()
        d, K, N = c.d, c.K_local, c.N
        flat = _f32(_val(params), int(sz.n_params)).clone().requires_grad_(True)
        lam = float(_f32(_val(e.lambda_), 1)[0]) if e.lambda_ else 0.0
        dt, sq, sig = torch.tensor(c.dt), torch.tensor(c.sqrt_dt), c.sigma_scale
        X = _f32(_val(x0), K * d).view(K, d).clone()
        noise = _f32(_val(xi), N * K * d).view(N, K, d)
        cv = _f32(c.drift, d).view(1, d) if c.drift_kind == nat.DRIFT_EIG_FP else None
        nt, DB0 = (K + 15) // 16, (d + 15) // 16
        PBL = 2 * DB0 * 256
        pstore = _f32(_val(path), (N + 1) * nt * PBL).view(N + 1, nt, PBL)

        def value(x):
            o = self._net(g, flat, x)
            return torch.relu(o) if e.output_relu else o

        def put_image(n, x):
            img = torch.zeros(nt * 16, DB0 * 16)
            img[:K, :d] = x
            pstore[n, :, :DB0 * 256] = img.view(nt, 16, DB0 * 4, 4).permute(0, 2, 3, 1).reshape(nt, DB0 * 256)
        stopped = torch.zeros(K, dtype=torch.bool)
        msteps = torch.zeros(K)
        S, Y, count = torch.zeros(K), None, 0
        for n in range(N):
            if not bool((~stopped).any()):
                break
            put_image(n, X)
            Xg = X.clone().requires_grad_(True)
            V = value(Xg)
            Z = sig * torch.autograd.grad(V.sum(), Xg, create_graph=True)[0]
            if Y is None:
                Y = V
            if cv is not None:
                Ssum = (cv * torch.cos(X)).sum(1)
                b = -torch.cos(Ssum).unsqueeze(1) * cv * torch.sin(X)
                h = V * (-(cv ** 2 * torch.sin(X) ** 2).sum(1) * torch.sin(Ssum) - torch.cos(Ssum) * Ssum)
            else:
                assert c.h_kind == nat.GH_EIG_NLS
                p0, dd = c.h_par[0], c.h_par[1]
                b = torch.zeros_like(X)
                h = -V ** 3 - V * (-p0 * torch.exp(2 / dd * torch.cos(X).sum(1)) + (torch.sin(X) ** 2 / dd ** 2 - torch.cos(X) / dd).sum(1) - 3)
            Xp = X + (b * dt + sig * noise[n] * sq) * (~stopped).float().unsqueeze(1)
            inside = ((Xp >= c.dom_a) & (Xp <= c.dom_b)).all(1)
            act = inside & ~stopped
            actf = act.float()
            Y = Y + ((-h - lam * V) * dt + (Z * noise[n]).sum(1) * sq) * actf
            S = S + actf * V.detach() * dt
            X = torch.where(act.unsqueeze(1), Xp, X).detach()
            msteps += actf
            count += int(act.sum())
            stopped = stopped | ~inside
        put_image(N, X)
        Vn = value(X)
        _f32(_val(VN), K).copy_(Vn.detach())
        _f32(_val(YN), K).copy_(Y.detach())
        _f32(_val(XN), K * d).copy_(X.reshape(-1))
        _f32(_val(tN), K).copy_(msteps * dt)
        _i64(_val(kcount), 1)[0] += count
        if e.s_out:
            _f32(e.s_out, K).copy_(S)
        m = torch.cat([msteps, -torch.ones(16 * nt - K)]).view(nt, 16).max(1).values
        _i32(_val(ahat) + 4 * (N + 1) * nt * 16, nt).copy_(torch.clamp(m + 1, max=N).int())
        self.state = (Y, Vn, flat)
        self.calls.append(("fwd", K, lam, int(e.output_relu)))
        return 0

    def psp_genl_rollout_bwd(self, cfg_ref, params, tables, path, ahat, wY, wV, grad_partial, grad_out, stream):
        Y, Vn, flat = self.state
        K = cfg_ref._obj.base.K_local
        loss = (_f32(_val(wY), K) * Y).sum() + (_f32(_val(wV), K) * Vn).sum()
        grad, = torch.autograd.grad(loss, flat, allow_unused=True)
        _f32(_val(grad_out), flat.numel()).copy_(grad if grad is not None else torch.zeros_like(flat))
        self.calls.append(("bwd", K))
        return 0

    def psp_adam_step(self, params, grad, m, v, n, step, lr, b1, b2, eps, stream):
        p, g = _f32(_val(params), n), _f32(_val(grad), n)
        mm, vv = _f32(_val(m), n), _f32(_val(v), n)
        mm.copy_(mm + (g - mm) * (1.0 - b1))
        vv.copy_(vv * b2 + (1.0 - b2) * g * g)
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        denom = vv.sqrt() / math.sqrt(bc2) + eps
        p.copy_(p - (lr / bc1) * (mm / denom))
        self.calls.append(("adam", int(n)))
        return 0


def install(monkeypatch):
    """Route EigenvalueSolver's native plan to the stand-in and let it accept a CPU device.  Returns the FakeEigenKernels object."""
    from path_space_pde_solver_amd import plan_eigen_native as pen
    fake = FakeEigenKernels()
    real_eligibility = pen.eigen_eligibility

    def eligibility(solver):
        class OnGpu:                                             # every check of the real function but the device's
            def __getattr__(self, name):
                return getattr(solver, name)
            device = torch.device("cuda")
        why = real_eligibility(OnGpu())
        return why
    monkeypatch.setattr(pen, "eigen_eligibility", eligibility)
    monkeypatch.setattr(nat, "load", lambda: fake)
    return fake
