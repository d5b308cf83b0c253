"""Host side of the native PINN plan: psp_pinn_query's limits, the ABI struct sizes, and the reasons plan_pinn_native gives for
every composite-only configuration.  No GPU."""
import ctypes as C

import pytest
import torch

from conftest import load_golden
from pinn_cases import COMPOSITE_ONLY, GPU_SHAPES, NATIVE_SCOPE, build
from util_cases import psp

nat = psp.native


def config(d, has_time, widths, K=8, **over):
    c = nat.PinnConfig()
    c.d, c.K, c.has_time, c.n_hidden = d, K, has_time, len(widths)
    for i, h in enumerate(widths[:4]):
        c.widths[i] = h
    c.sigma_scale = 1.0
    for k, v in over.items():
        setattr(c, k, v)
    return c


def query(c):
    sz = nat.PinnSizes()
    return nat.load().psp_pinn_query(C.byref(c), C.byref(sz)), sz


@pytest.mark.parametrize("name", sorted(GPU_SHAPES))
def test_query_accepts_the_kernel_test_shapes(name):
    kw = GPU_SHAPES[name]
    n_in = kw["d"] + (1 if kw["parabolic"] else 0)
    rc, sz = query(config(kw["d"], int(kw["parabolic"]), kw["arch"], K=kw["K"]))
    assert rc == 0, nat.last_error()
    fan, P = n_in, 0
    for h in kw["arch"] + [1]:
        P += fan * h + h
        fan += h
    assert sz.n_params == P
    assert sz.dir_blocks == (n_in + 13) // 14 and sz.tiles == kw["K"] * sz.dir_blocks
    assert 0 < sz.bwd_workgroups <= sz.tiles and sz.grad_partial_bytes == 4 * P * sz.bwd_workgroups
    assert sz.scratch_bytes >= 4 * kw["K"] * (2 * n_in + 3)
    assert sz.lds_fwd_bytes < sz.lds_bwd_bytes <= 160 * 1024


def test_query_limits():
    assert query(config(112, 0, [128, 128, 128, 128]))[0] == 0          # the largest net: its images fit the LDS
    assert query(config(111, 1, [128]))[0] == 0
    assert query(config(113, 0, [20]))[0] == -2                           # input > 112
    assert query(config(112, 1, [20]))[0] == -2
    assert query(config(10, 1, [129]))[0] == -2                           # width > 128
    assert query(config(10, 1, []))[0] == -2                              # L = 0
    c = config(10, 1, [8, 8, 8, 8])
    c.n_hidden = 5
    assert query(c)[0] == -2                                              # L = 5
    rc, _ = query(config(10, 1, [20], sigma_kind=nat.GENL_SIGMA_DENSE))
    assert rc == -4 and "dense sigma" in nat.last_error()
    assert query(config(10, 1, [20], h_kind=nat.GH_EXPBALL_SIN, h_par=(C.c_float * 4)(0.5, 10.0, 1.0, 1.0)))[0] == -1   # h reads t
    assert query(config(10, 1, [20], drift_kind=nat.DRIFT_DOUBLE_WELL))[0] == -1      # no drift vector
    assert query(config(10, 1, [20], K=0))[0] == -1
    assert nat.load().psp_pinn_query(None, None) == -1


def test_abi_struct_sizes5():
    out = (C.c_int32 * 2)()
    assert nat.load().psp_abi_struct_sizes5(C.byref(out)) == 0
    assert list(out) == [C.sizeof(nat.PinnConfig), C.sizeof(nat.PinnSizes)]
    assert ("psp_abi_struct_sizes5", (nat.PinnConfig, nat.PinnSizes)) in nat.ABI_STRUCTS
    assert nat.load().psp_version() == 400                                # pure additions


def reason(model):
    return psp.plan_pinn_native.pinn_eligibility(model)


@pytest.mark.parametrize("name", NATIVE_SCOPE)
def test_native_scope_goldens_only_lack_a_gpu_here(name):
    _, model = build(load_golden(name)["case"])
    assert "need a GPU" in reason(model)


@pytest.mark.parametrize("name", sorted(COMPOSITE_ONLY))
def test_composite_only_goldens_give_their_reason(name):
    _, model = build(load_golden(name)["case"])
    assert COMPOSITE_ONLY[name] in reason(model)
    model.L = 1
    model.train_PINN()
    assert model.plan_name == "torch" and COMPOSITE_ONLY[name] in model.plan_reason


def test_reasons_of_the_other_composite_only_configurations(monkeypatch):
    case = load_golden("pinn_heat_d6")["case"]
    _, model = build(case)
    assert "need a GPU" in reason(model)                                 # CPU
    for dtype in ("f16x3", "bf16", "bf16_fwd"):
        assert "fp32 MFMA only" in reason(build(case, mlp_dtype=dtype)[1])
    prob, model = build(case)                                             # a dense sigma
    prob.general_native_spec = lambda: {"drift": (nat.DRIFT_ZERO, None), "sigma": torch.ones(6, 6), "h": nat.GH_ZERO}
    assert "dense sigma" in reason(model)
    prob, model = build(case)                                             # overridden coefficients
    prob.h = lambda t, x, y, z: y
    assert "problem.h" in reason(model)
    _, model = build(case)                                                # a user net that is no dense-concat net

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(7, 1)
            self.optim = torch.optim.Adam(self.parameters(), lr=1e-3)

        def forward(self, x):
            return self.lin(x)

    model.V = Net()
    assert "dense-concat" in reason(model)
    _, model = build(case)
    model.V = psp.DenseNet(d_in=7, d_out=1, lr=1e-3, arch=[8, 8, 8, 8, 8], seed=1)
    assert "hidden layers" in reason(model)
    _, model = build(case)                                                # more than one rank
    monkeypatch.setattr(psp.plan_pinn_native.sharding, "dist_info", lambda: (None, 0, 2))
    assert "more than one rank" in reason(model)


def test_backend_native_raises_where_the_plan_is_composite():
    _, model = build(load_golden("pinn_expball_hess_d4_full")["case"], backend="native")
    with pytest.raises(NotImplementedError, match="full_hessian"):
        model.train_PINN()
    _, model = build(load_golden("pinn_heat_d6")["case"], backend="torch", L=1)
    model.train_PINN()
    assert model.plan_name == "torch" and "backend='torch'" in model.plan_reason
