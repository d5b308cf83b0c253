"""Host tests of plan_common.py (and of the loss arithmetic it sits on in sharding.py): the steps every native plan shares, at
the smallest sizes at which each can go wrong.  No GPU, no launch: the one C-ABI call that is reached (psp_adam_step, through
Y0Adam.step) is answered by the CPU stand-in of tests/fake_kernels.py.
"""
import types

import pytest
import torch

from util_cases import psp
from fake_kernels import FakeKernels

from path_space_pde_solver_amd import plan_common as pc, sharding  # noqa: E402

EPS = torch.finfo(torch.float32).eps


# ---- rehome_params ---------------------------------------------------------------------------------------------------------
def test_rehome_params_aliases_every_tensor_at_its_running_offset():
    torch.manual_seed(0)
    sets = [[torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(2)), torch.nn.Parameter(torch.randn(2, 5))],
            [torch.nn.Parameter(torch.randn(4, 3).t()), torch.nn.Parameter(torch.randn(1)), torch.nn.Parameter(torch.randn(2, 2, 2))]]
    params = [p for ps in sets for p in ps]
    assert not params[3].is_contiguous()
    before = [p.detach().clone() for p in params]
    flat = pc.rehome_params(params, torch.device('cpu'))
    assert flat.dtype == torch.float32 and flat.numel() == sum(p.numel() for p in params)
    off = 0
    for p, b in zip(params, before):
        assert torch.equal(p.detach(), b) and p.shape == b.shape
        assert p.data_ptr() == flat.data_ptr() + 4 * off and p.is_contiguous()
        assert torch.equal(flat[off:off + p.numel()], b.reshape(-1))
        off += p.numel()
    flat.mul_(2.0)                                                    # writing flat changes the tensors ...
    for p, b in zip(params, before):
        assert torch.equal(p.detach(), 2.0 * b)
    with torch.no_grad():
        params[4].fill_(7.0)                                          # ... and writing a tensor changes flat
    o4 = sum(p.numel() for p in params[:4])
    assert flat[o4].item() == 7.0 and flat[o4 - 1].item() == 2.0 * before[3].reshape(-1)[-1].item()


# ---- adam_hyper ------------------------------------------------------------------------------------------------------------
def _module(**adam):
    m = torch.nn.Linear(2, 2)
    if adam:
        m.optim = torch.optim.Adam(m.parameters(), **adam)
    return m


def test_adam_hyper_reads_the_modules_own_adam():
    m = _module(lr=3e-3, betas=(0.8, 0.95), eps=1e-6)
    assert pc.adam_hyper(m, 1.0, pc.PlanUnsupported) == (3e-3, 0.8, 0.95, 1e-6)
    assert pc.adam_hyper([m, _module(lr=3e-3, betas=(0.8, 0.95), eps=1e-6)], 1.0, pc.PlanUnsupported) == (3e-3, 0.8, 0.95, 1e-6)
    assert pc.adam_hyper(_module(), 0.25, pc.PlanUnsupported) == (0.25, 0.9, 0.999, 1e-8)


@pytest.mark.parametrize("error", [psp.PlanUnsupported, NotImplementedError])
@pytest.mark.parametrize("bad", [dict(weight_decay=0.01), dict(amsgrad=True)])
def test_adam_hyper_refuses_what_the_native_adam_lacks(error, bad):
    with pytest.raises(error, match="weight_decay") as e:
        pc.adam_hyper(_module(lr=1e-3, **bad), 1e-3, error)
    assert type(e.value) is error


@pytest.mark.parametrize("error", [psp.PlanUnsupported, NotImplementedError])
def test_adam_hyper_needs_one_setting_for_a_fused_step(error):
    a, b = _module(lr=1e-3), _module(lr=2e-3)
    with pytest.raises(error, match="different Adam settings") as e:
        pc.adam_hyper([a, b], 1e-3, error)
    assert type(e.value) is error
    assert pc.adam_hyper(a, 1e-3, error)[0] == 1e-3 and pc.adam_hyper([b], 1e-3, error)[0] == 2e-3


# ---- draw_noise ------------------------------------------------------------------------------------------------------------
K, D, N, DP = 6, 3, 2, 16
CPU = torch.device('cpu')


def _solver(random_X_0=False, seed=5):
    return types.SimpleNamespace(K=K, d=D, N=N, random_X_0=random_X_0, seed=seed)


def _reference_draw(s, lo=0, hi=K, d_pad=DP):
    torch.manual_seed(7)
    return pc.draw_noise(s, 0, 'reference', lo, hi - lo, d_pad, CPU)


def test_draw_noise_reference_is_the_references_draw_sliced_and_padded():
    s = _solver()
    xi, x0 = _reference_draw(s)
    state = torch.get_rng_state()
    assert x0 is None and xi.shape == (N + 1, K, DP) and xi.is_contiguous() and xi.dtype == torch.float32
    assert torch.count_nonzero(xi[:, :, D:]) == 0
    torch.manual_seed(7)
    want = torch.randn(K, D, N + 1)
    assert torch.equal(torch.get_rng_state(), state)                  # the generator stands where the reference leaves it
    assert torch.equal(xi[:, :, :D], want.permute(2, 0, 1))
    parts = [_reference_draw(s, lo, hi)[0] for lo, hi in ((0, 3), (3, 6))]      # ranks (0, 2) and (1, 2)
    assert all(p.shape == (N + 1, 3, DP) and p.is_contiguous() for p in parts)
    assert torch.equal(torch.cat(parts, 1), xi)
    assert torch.equal(_reference_draw(s, d_pad=D)[0], want.permute(2, 0, 1))    # nothing to pad


def test_draw_noise_reference_draws_a_random_X_0_first():
    s = _solver(random_X_0=True)
    xi, x0 = _reference_draw(s, 3, 6)
    state = torch.get_rng_state()
    torch.manual_seed(7)
    want_x0 = torch.randn(K, D)
    want_xi = torch.randn(K, D, N + 1)
    assert torch.equal(torch.get_rng_state(), state)
    assert x0.shape == (3, DP) and x0.is_contiguous() and torch.count_nonzero(x0[:, D:]) == 0
    assert torch.equal(x0[:, :D], want_x0[3:6]) and torch.equal(xi[:, :, :D], want_xi[3:6].permute(2, 0, 1))


def test_draw_noise_philox_seeds_X_0_by_seed_and_iteration():
    s = _solver(random_X_0=True)
    before = torch.get_rng_state()
    xi, a = pc.draw_noise(s, 4, 'philox', 2, 3, DP, CPU)
    assert xi is None and a.shape == (3, DP) and a.is_contiguous() and torch.count_nonzero(a[:, D:]) == 0
    assert torch.equal(torch.get_rng_state(), before)                 # the global generator is the reference's: untouched
    assert torch.equal(a, pc.draw_noise(s, 4, 'philox', 2, 3, DP, CPU)[1])
    assert not torch.equal(a, pc.draw_noise(s, 5, 'philox', 2, 3, DP, CPU)[1])
    g = torch.Generator().manual_seed(5 * 1000003 + 4)
    assert torch.equal(a[:, :D], torch.randn(K, D, generator=g)[2:5])
    assert pc.draw_noise(_solver(), 4, 'philox', 2, 3, DP, CPU) == (None, None)


# ---- trajectory weights against autograd of the losses as the reference writes them (solver.py:164-186) ------------------------
KW = 8


def _terminal_values():
    """Y_N and g(X_N) for 8 trajectories: fp64 draws rounded to fp32, so that fp64 autograd and the fp32 code see equal inputs."""
    gen = torch.Generator().manual_seed(11)
    Y = (0.7 * torch.randn(KW, generator=gen, dtype=torch.float64)).float()
    D = (0.9 * torch.randn(KW, generator=gen, dtype=torch.float64) + 0.3).float()
    return Y, D


def _reference_loss(loss_method, adaptive, Y, g):
    if loss_method == 'log-variance':
        return torch.mean((Y - g) ** 2) - torch.mean(Y - g) ** 2
    if loss_method == 'moment':
        return torch.mean((Y - g) ** 2)
    if loss_method == 'variance':
        return torch.var(torch.exp(-g + Y))
    if adaptive:
        return torch.mean(Y * torch.exp(-g + Y.detach()))
    return torch.mean(Y * torch.exp(-g))


@pytest.mark.parametrize("loss_method,adaptive", [("log-variance", True), ("moment", True), ("variance", True),
                                                  ("cross_entropy", True), ("cross_entropy", False)])
def test_attached_weights_equal_autograd_of_the_reference_loss(loss_method, adaptive):
    """Tolerance: every weight is an elementwise fp32 expression of at most four operations on fp32 inputs (the 8-term sums
    behind the means run in fp64 and add nothing at this level): with exp counted as one ulp, at most eight roundings of
    EPS / 2 relative to the largest intermediate M of that expression -- 4 EPS M; the bound asserted is twice that, 8 EPS M."""
    Y32, D32 = _terminal_values()
    Y = Y32.double().requires_grad_(True)
    g = (Y32.double() - D32.double()).requires_grad_(True)
    loss_ref = _reference_loss(loss_method, adaptive, Y, g)
    dY, dg = torch.autograd.grad(loss_ref, (Y, g))
    sums = torch.stack([D32.double().sum(), (D32.double() ** 2).sum()])
    Emax = float(torch.exp(D32 if adaptive else D32 - Y32).max())
    if loss_method in ('log-variance', 'moment'):
        loss = sharding.loss_from_sums(sums, KW, loss_method)
        w = sharding.loss_weights(D32, sums, KW, loss_method)
        M = (2.0 / KW) * (float(D32.abs().max()) + abs(float(sums[0]) / KW))
        loss_M = float(sums[1]) / KW
    else:
        loss, w = sharding.generic_loss_weights(loss_method, adaptive, D32, Y32, KW, torch.empty(KW))
        if loss_method == 'variance':
            M = (2.0 / (KW - 1)) * Emax * 2.0 * Emax
            loss_M = KW * Emax * Emax / (KW - 1)
        else:
            M = Emax / KW
            loss_M = float(Y32.abs().max()) * Emax
    mu, nu, wT_buf = torch.full((KW,), 9.0), torch.full((KW,), 9.0), torch.full((KW,), 9.0)
    wT = pc.attached_weights(loss_method, False, KW, w, Y32, mu, nu, wT_buf)
    err_w, err_l = float((w.double() - dY).abs().max()), abs(float(loss) - float(loss_ref.detach()))
    print("%s adaptive=%s: max |w - dL/dY| = %.3g = %.3g EPS M; |loss - ref| = %.3g = %.3g EPS M"
          % (loss_method, adaptive, err_w, err_w / (EPS * M), err_l, err_l / (EPS * loss_M)))
    assert w.dtype == torch.float32 and torch.equal(mu, w)
    assert err_w <= 8 * EPS * M
    assert err_l <= 8 * EPS * loss_M
    assert torch.all(nu == 9.0)                                       # nu belongs to relative entropy alone
    if loss_method == 'cross_entropy':
        MT = float(Y32.abs().max()) * M
        err_T = float((wT.double() - dg).abs().max())                 # lambda_N = dL/dg(X_N) grad g
        print("  max |wT - dL/dg| = %.3g = %.3g EPS M" % (err_T, err_T / (EPS * MT)))
        assert wT is wT_buf and torch.equal(wT, -Y32 * w)
        assert err_T <= 8 * EPS * MT
    else:
        assert wT is None and torch.all(wT_buf == 9.0)
        assert float(dg.add(dY).abs().max()) <= 1e-15               # these losses see g through D = Y - g alone


def test_attached_weights_relative_entropy():
    Y32, D32 = _terminal_values()
    zsum = (-D32.double() - 0.2).requires_grad_(True)                 # the kernels keep D = -(Zsum + g)
    y = Y32.double().requires_grad_(True)
    loss_ref = torch.mean(zsum + 0.2) + 0.0 * y.sum()                 # solver.py:179-180: no Y in it
    dZ, dY = torch.autograd.grad(loss_ref, (zsum, y))
    sums = torch.stack([D32.double().sum(), (D32.double() ** 2).sum()])
    assert abs(float(sharding.loss_from_sums(sums, KW, 'relative_entropy')) - float(loss_ref)) <= 8 * EPS * float(D32.abs().max())
    mu, nu, wT_buf = torch.full((KW,), 9.0), torch.full((KW,), 9.0), torch.full((KW,), 9.0)
    assert pc.attached_weights('relative_entropy', True, KW, None, None, mu, nu, wT_buf) is None
    assert torch.equal(mu.double(), dY) and torch.all(mu == 0)
    assert torch.equal(nu.double(), dZ) and torch.all(nu == 1.0 / KW)  # 1/8 is exact in fp32
    assert torch.all(wT_buf == 9.0)


# ---- Y0Adam ----------------------------------------------------------------------------------------------------------------
def _trained_y0():
    y = psp.SingleParam(lr=1e-2, initial=0.5)
    for grad in (0.5, -0.25):
        y.Y_0.grad = torch.tensor([grad])
        y.optim.step()
    return y


def test_y0_adam_imports_state_only_when_asked():
    y = _trained_y0()
    st = y.optim.state[y.Y_0]
    on = pc.Y0Adam(y, CPU, import_state=True)
    assert on.param is y.Y_0 and on.imported_step == 2
    assert torch.equal(on.m, st['exp_avg']) and torch.equal(on.v, st['exp_avg_sq']) and float(on.v) > 0
    off = pc.Y0Adam(y, CPU, import_state=False)
    assert off.imported_step == 0 and float(off.m) == 0 and float(off.v) == 0 and float(off.grad) == 0
    fresh = pc.Y0Adam(psp.SingleParam(lr=1e-2), CPU, import_state=True)
    assert fresh.imported_step == 0 and float(fresh.m) == 0 and float(fresh.v) == 0


def test_y0_adam_steps_and_exports():
    y = psp.SingleParam(lr=1e-2, initial=0.5)
    twin = psp.SingleParam(lr=1e-2, initial=0.5)
    y0 = pc.Y0Adam(y, CPU, import_state=False)
    lib = types.SimpleNamespace(psp_adam_step=lambda *a: FakeKernels.psp_adam_step(None, *a))
    hyper = pc.adam_hyper(y, 1.0, pc.PlanUnsupported)
    assert hyper == (1e-2, 0.9, 0.999, 1e-8)
    y0.export(0)                                                      # nothing stepped: nothing to write
    assert len(y.optim.state) == 0
    Kg = 4
    for step, sum_D in enumerate((3.0, -1.0, 0.5), start=1):
        sums = torch.tensor([sum_D, 7.0], dtype=torch.float64)
        y0.step(lib, sums, Kg, 'moment', None, step, hyper, None)
        assert float(y0.grad) == 2.0 * sum_D / Kg                     # (2/K) sum D
        twin.Y_0.grad = y0.grad.clone()
        twin.optim.step()
    y0.export(3)
    st = y.optim.state[y.Y_0]
    assert float(st['step']) == 3
    assert torch.equal(st['exp_avg'], y0.m) and torch.equal(st['exp_avg_sq'], y0.v)
    ref = twin.optim.state[twin.Y_0]                                  # torch's own Adam on the same gradients
    assert torch.allclose(y0.m, ref['exp_avg'], rtol=4 * EPS, atol=0) and torch.allclose(y0.v, ref['exp_avg_sq'], rtol=4 * EPS, atol=0)
    assert abs(float(y.Y_0) - float(twin.Y_0)) <= 8 * EPS
    y0.step(lib, torch.tensor([5.0, 7.0], dtype=torch.float64), Kg, 'log-variance', None, 4, hyper, None)
    assert float(y0.grad) == 0.0                                      # log-variance does not move Y_0


# ---- the rest --------------------------------------------------------------------------------------------------------------
def test_local_shard_and_log_mean_ul2_and_range_fallbacks():
    dist, rank, world, lo, hi = pc.local_shard(10)
    assert (dist, rank, world, lo, hi) == (None, 0, 1, 0, 10)
    out = torch.zeros(3)
    pc.log_mean_ul2(torch.tensor([1.0, 2.0, 3.0, 6.0]), 8, out, 1)     # the mean is over the GLOBAL K
    assert out.tolist() == [0.0, 1.5, 0.0]
    assert pc.range_fallbacks(None) == 0 and pc.range_fallbacks(torch.tensor([1, 3, 0, 0], dtype=torch.int32)) == 3


def test_fill_hjb_base_sets_the_common_fields_and_flags():
    nat = psp.native
    spec = dict(drift=(nat.DRIFT_DENSE, None), sigma=(nat.SIGMA_DENSE, None, 0.5), runcost=(nat.RUNCOST_ZERO, None),
                term=(nat.TERM_LINEAR, None))

    def solver(loss_method, adaptive, detach):
        return types.SimpleNamespace(K=64, N=5, delta_t=torch.tensor(0.01), sq_delta_t=torch.sqrt(torch.tensor(0.01)),
                                     loss_method=loss_method, adaptive_forward_process=adaptive, detach_forward=detach)
    cases = [("log-variance", True, True, 'philox', (False, False, False), nat.LOSS_LOG_VARIANCE, 1),
             ("moment", True, False, 'reference', (False, False, True), nat.LOSS_MOMENT, 2),
             ("cross_entropy", False, False, 'reference', (True, False, False), nat.LOSS_WEIGHTS, 1),
             ("relative_entropy", True, False, 'philox', (False, True, True), nat.LOSS_REL_ENTROPY, 3)]
    for loss_method, adaptive, detach, noise, flags, kind, store in cases:
        cfg = nat.HjbConfig()
        assert pc.fill_hjb_base(cfg, solver(loss_method, adaptive, detach), spec, noise, 16, 32) == flags
        assert (cfg.K_local, cfg.N, cfg.K_global, cfg.k_offset) == (16, 5, 64, 32)
        assert cfg.dt == pytest.approx(0.01, rel=1e-6) and cfg.sqrt_dt == pytest.approx(0.1, rel=1e-6)
        assert (cfg.drift_kind, cfg.sigma_kind, cfg.runcost_kind, cfg.term_kind) == (nat.DRIFT_DENSE, nat.SIGMA_DENSE,
                                                                                     nat.RUNCOST_ZERO, nat.TERM_LINEAR)
        assert cfg.sigma_scale == 0.5 and cfg.adaptive == int(adaptive) and cfg.loss_kind == kind and cfg.store_path == store
        assert cfg.noise_mode == (nat.NOISE_PHILOX if noise == 'philox' else nat.NOISE_SUPPLIED)
        assert (cfg.d, cfg.H, cfg.mlp_dtype) == (0, 0, 0) and not cfg.drift and not cfg.sigma   # the caller's
