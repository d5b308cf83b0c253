"""Host logic of the dense-sigma route, checked without a GPU and without the library: the translation of a problem's
general_native_spec() into psp_genl_config (plan_general_native.set_sigma), the appended ctypes fields, and QuadraticOnBox's
optional matrix."""
import ctypes as C

import pytest
import torch

from util_cases import psp
from path_space_pde_solver_amd import plan_general_native as pgn

nat = psp.native


def nonsymmetric(d, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(d, d, generator=g) / d ** 0.5


def test_set_sigma_dense_uploads_row_major_B():
    d = 5
    B = nonsymmetric(d)
    assert not torch.equal(B, B.t())
    pb = psp.QuadraticOnBox(d=d, B=B.double(), device="cpu")         # any dtype in, fp32 out
    spec = pb.general_native_spec()
    assert "sigma_scale" not in spec and torch.equal(spec["sigma"], B)
    gcfg = nat.GenlConfig()
    gcfg.base.d = d
    keep = []
    pgn.set_sigma(gcfg, spec, torch.device("cpu"), keep)
    assert gcfg.sigma_kind == nat.GENL_SIGMA_DENSE == 1
    assert len(keep) == 1 and keep[0].dtype == torch.float32 and keep[0].is_contiguous()
    assert gcfg.sigma == keep[0].data_ptr()
    back = (C.c_float * (d * d)).from_address(gcfg.sigma)
    assert list(back) == [float(v) for v in B.reshape(-1)]           # row-major B, not its transpose
    assert list(back) != [float(v) for v in B.t().reshape(-1)]
    # a transposed VIEW is uploaded by value, not by stride
    keep2 = []
    pgn.set_sigma(gcfg, {"sigma": B.t()}, torch.device("cpu"), keep2)
    assert list((C.c_float * (d * d)).from_address(gcfg.sigma)) == [float(v) for v in B.t().contiguous().reshape(-1)]
    with pytest.raises(ValueError):
        pgn.set_sigma(gcfg, {"sigma": torch.zeros(d, d + 1)}, torch.device("cpu"), [])


def test_set_sigma_scaled_identity():
    gcfg = nat.GenlConfig()
    gcfg.base.d = 4
    gcfg.sigma_kind, gcfg.sigma = 1, 12345                           # stale values are overwritten
    keep = []
    pgn.set_sigma(gcfg, psp.QuadraticOnBox(d=4, scale=1.5, device="cpu").general_native_spec(), torch.device("cpu"), keep)
    assert gcfg.sigma_kind == nat.GENL_SIGMA_SCALED == 0 and not gcfg.sigma and keep == []
    assert gcfg.base.sigma_scale == 1.5
    # a zero-initialised config means the scaled identity
    z = nat.GenlConfig()
    assert z.sigma_kind == 0 and not z.sigma


def test_quadratic_on_box_without_B_is_unchanged():
    pb = psp.QuadraticOnBox(d=3, scale=2.0, quad_h=False, device="cpu")
    assert pb.general_native_spec() == {"drift": (nat.DRIFT_ZERO, None), "sigma_scale": 2.0, "h": nat.GH_ZERO}
    assert torch.equal(pb.B, 2.0 * torch.eye(3))
    pq = psp.QuadraticOnBox(device="cpu")
    assert pq.general_native_spec() == {"drift": (nat.DRIFT_ZERO, None), "sigma_scale": 1.0, "h": nat.GH_QUAD}
    B = nonsymmetric(3)
    pd = psp.QuadraticOnBox(d=3, B=B, parabolic=False, device="cpu")
    assert pd.sigma(torch.zeros(2, 3)) is pd.B and torch.equal(pd.B, B) and pd.general_native_spec()["h"] == nat.GH_QUAD


def test_genl_config_layout_appends_the_new_fields():
    old = [("base", 0), ("has_time", 136), ("n_hidden", 140), ("widths", 144), ("activation", 160), ("linear_layout", 164),
           ("time_first", 168), ("time_scale", 172)]
    assert C.sizeof(nat.GenConfig) == 136                            # psp_gen_config stays byte-identical
    for name, off in old:
        assert getattr(nat.GenlConfig, name).offset == off, name
    names = [f[0] for f in nat.GenlConfig._fields_]
    assert names[:8] == [n for n, _ in old] and names[8:] == ["sigma_kind", "reserved", "sigma"]
    assert nat.GenlConfig.sigma_kind.offset == 176 and nat.GenlConfig.sigma.offset == 184
    assert C.sizeof(nat.GenlConfig) == 192


class _Solver:
    """The attributes native_eligibility reads."""

    def __init__(self, problem, V):
        self.device = torch.device("cuda")                           # (only its type is read; nothing is run on it)
        self.approx_method, self.loss_method = "Y", "diffusion"
        self.adaptive_forward_process, self.detach_forward, self.boundary_loss = False, True, True
        self.V, self.d, self.elliptic, self.problem = V, problem.d, True, problem


def test_dense_spec_is_routed_past_the_templated_kernels():
    d = 4
    V = psp.DenseNet(d_in=d, d_out=1, lr=1e-3, arch=[30, 30], seed=1)    # a shape the templated family would take
    dense = _Solver(psp.ExponentialOnBallNonlinearSinHessian(d=d, device="cpu"), V)
    reason = pgn.native_eligibility(dense)
    assert reason is not None and "dense sigma" in reason
    if nat.is_built():
        assert pgn.native_eligibility(dense, deep=True) is None
        plain = _Solver(psp.ExponentialOnBallNonlinearSin(d=d, device="cpu"), V)
        r = pgn.native_eligibility(plain)
        assert r is None or "dense sigma" not in r
