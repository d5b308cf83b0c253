"""Host logic of EigenvalueSolver's native plan (plan_eigen_native.py) without a GPU: the plan on the CPU stand-in of its three
launches (tests/fake_eigen_kernels.py) against the reference's notebooks -- which pins the RNG order of the two normalisations, the
rewind of the generator after the rollout, the loss assembly, lambda's gradient from S_k and the two Adam steps --, the reasons for
which the plan declines, and what psp_genl_query_eig refuses."""
import ctypes as C
import math

import pytest
import torch

import fake_eigen_kernels
from eigen_cases import GOLDENS, LOSS_LOGS, build, notebook_net
from util_cases import psp
from path_space_pde_solver_amd import plan_eigen_native as pen
from path_space_pde_solver_amd import plan_general_deep as pgd

nat = psp.native


@pytest.mark.parametrize("name", GOLDENS)
def test_plan_on_the_stand_in_follows_the_notebook(name, monkeypatch):
    """Both normalisations ('center' draws nothing, 'l2' draws X_2 before the boundary batch), exits and no exits: three iterations
    on the stand-in give the notebook's logs to fp32 rounding; a draw out of order would move every later number."""
    torch.set_num_threads(1)
    fake = fake_eigen_kernels.install(monkeypatch)
    rec, prob, model = build(name, backend="native")
    exp = rec["expected"]
    model.train()
    assert model.plan_name == "native" and type(model._gen_plan).__name__ == "EigenDeepPlan"
    assert [c[0] for c in fake.calls] == ["fwd", "bwd", "adam", "adam"] * 3
    assert [c[1] for c in fake.calls if c[0] == "adam"] == [model._gen_plan.P, 1] * 3          # V first, then lambda
    assert model.K_log == exp["K_log"]
    for log in LOSS_LOGS + ("V_L2_log", "lambda_log"):
        got, want = getattr(model, log), exp[log]
        assert len(got) == len(want) == 3
        for a, b in zip(got, want):
            assert math.isclose(a, b, rel_tol=2e-4, abs_tol=1e-7 * abs(exp["loss_log"][0])), (log, got, want)
    # the generator stands where the notebook's stands: the next draw is the same
    nxt = torch.rand(3)
    rec2, prob2, ref = build(name, backend="torch")
    ref.train()
    assert torch.equal(nxt, torch.rand(3))
    assert model.lambda_.Y_0.item() == pytest.approx(exp["lambda_final"], abs=1e-6)
    assert len(model.times) == 3


def test_lambda_reaches_the_forward_as_a_device_pointer(monkeypatch):
    fake = fake_eigen_kernels.install(monkeypatch)
    rec, prob, model = build("eig_fp_d5", backend="native")
    model.train()
    plan = model._gen_plan
    lams = [c[2] for c in fake.calls if c[0] == "fwd"]
    assert lams[0] == pytest.approx(0.5) and lams[1:] == pytest.approx(model.lambda_log[:2])     # the value after each lambda step
    assert plan.eig.lambda_ == model.lambda_.Y_0.data_ptr() and plan.eig.s_out == plan._S.data_ptr()
    assert plan.eig.struct_bytes == C.sizeof(nat.GenlEig) and plan.eig.output_relu == 1
    assert plan.cfg.h_kind == nat.GH_EIG_FP and plan.cfg.drift_kind == nat.DRIFT_EIG_FP and plan.cfg.domain_kind == nat.DOM_BOX
    assert plan.cfg.adaptive == 0 and plan.gcfg.has_time == 0


class OnGpu:
    """A solver as the eligibility check would see it on a GPU machine."""
    device = torch.device("cuda")

    def __init__(self, s):
        self._s = s

    def __getattr__(self, name):
        return getattr(self._s, name)


def reason(model):
    return pen.eigen_eligibility(OnGpu(model))


def test_eligibility_reasons():
    rec, prob, model = build("eig_nls10_d5")
    assert "needs a GPU" in pen.eigen_eligibility(model)
    assert reason(model) is None
    model.train()
    assert model.plan_name == "torch" and "needs a GPU" in model.plan_reason
    with pytest.raises(NotImplementedError, match="native plan unavailable"):
        build("eig_nls10_d5", backend="native")[2].train()
    # mlp_dtype
    model.mlp_dtype = "bf16"
    assert "fp32 only" in reason(model)
    model.mlp_dtype = "fp32"
    # nets
    model.V = psp.DenseNet(5, 1, 0.001, arch=[15] * 5, output_relu=True)
    assert "hidden layers" in reason(model)
    model.V = psp.DenseNet(5, 1, 0.001, arch=[15, 200], output_relu=True)
    assert "wider" in reason(model)
    model.V = psp.DenseNet(6, 1, 0.001, arch=[15, 15])
    assert "not a dense-concat net (5 -> 1)" in reason(model)
    model.V = psp.MySequential(5, 1, 0.001, seed=1)
    assert reason(model) is not None
    for kind in ("fp", "nls5", "nls10"):
        model.V = notebook_net(kind, 5)
        assert reason(model) is None
    model.V = psp.DenseNet(5, 1, 0.001, arch=[8], activation="tanh2")      # no output ReLU: fine too
    assert reason(model) is None
    # overridden coefficients
    model.V = notebook_net("nls10", 5)
    prob.h = lambda x, y, z: y
    assert "problem.h" in reason(model)
    del prob.h

    class Other(psp.SchroedingerEigenvalue):
        def b(self, x):
            return torch.ones_like(x)
    rec, _, model2 = build("eig_nls10_d5")
    model2.problem = Other(d=5)
    assert "problem.b" in reason(model2)
    # more than one rank
    from path_space_pde_solver_amd import sharding
    real = sharding.dist_info
    try:
        sharding.dist_info = lambda: (None, 0, 2)
        assert "one rank" in reason(model)
    finally:
        sharding.dist_info = real


class UserRelu2(torch.nn.Module):
    """A dense-concat net a notebook defines for itself, with or without a ReLU on the output."""

    def __init__(self, d, arch, relu, bias):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.nn_dims = [d] + arch + [1]
        self.W = []
        fan = 0
        for i in range(len(self.nn_dims) - 1):
            fan += self.nn_dims[i]
            self.W += [torch.nn.Parameter(0.1 * torch.randn(fan, self.nn_dims[i + 1], generator=g)),
                       torch.nn.Parameter(bias * torch.ones(self.nn_dims[i + 1]))]
        for i, w in enumerate(self.W):
            self.register_parameter("param %d" % i, w)
        self.relu = relu

    def forward(self, x):
        for i in range(len(self.nn_dims) - 2):
            x = torch.cat([x, torch.relu(x @ self.W[2 * i] + self.W[2 * i + 1]) ** 2], 1)
        x = x @ self.W[-2] + self.W[-1]
        return torch.relu(x) if self.relu else x


class UserTanhLinear(torch.nn.Module):
    def __init__(self, d, arch, relu):
        super().__init__()
        torch.manual_seed(5)
        self.nn_dims = [d] + arch + [1]
        self.layers = torch.nn.ModuleList([torch.nn.Linear(sum(self.nn_dims[:i + 1]), self.nn_dims[i + 1])
                                           for i in range(len(self.nn_dims) - 1)])
        self.relu = relu

    def forward(self, x):
        for layer in self.layers[:-1]:
            x = torch.cat([x, torch.tanh(layer(x))], 1)
        x = self.layers[-1](x)
        return torch.relu(x) if self.relu else x


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("bias", [0.8, -0.3])
def test_probe_recognises_the_output_relu(relu, bias):
    """With bias 0.8 no output of the probe batch is negative, so relu(o) = o there: the probe lowers the output bias to decide."""
    V = UserRelu2(4, [6, 6], relu, bias)
    before = [p.detach().clone() for p in V.parameters()]
    spec = pgd.value_net_spec(V, 4, output_relu_ok=True)
    assert not isinstance(spec, str) and spec["act"] == "relu2" and spec["output_relu"] is relu and spec["linear"] is False
    assert all(torch.equal(a, b) for a, b in zip(before, V.parameters()))          # the probe restores the bias
    plain = pgd.value_net_spec(V, 4)
    if relu:
        assert isinstance(plain, str)                                              # the other plans refuse the ReLU
    else:
        assert plain["act"] == "relu2" and plain["output_relu"] is False
    T = UserTanhLinear(4, [7, 5], relu)
    spec = pgd.value_net_spec(T, 4, output_relu_ok=True)
    assert not isinstance(spec, str) and spec["act"] == "tanh" and spec["linear"] is True and spec["output_relu"] is relu


def test_package_nets_with_output_relu_are_refused_elsewhere():
    V = psp.DenseNet(5, 1, 0.001, arch=[8, 8], output_relu=True)
    assert "ReLU" in pgd.value_net_spec(V, 5)
    assert "ReLU" in pgd.value_net_spec(psp.DenseNet_tanh(5, 1, 0.001, arch=[8, 8], output_relu=True), 5)
    assert pgd.value_net_spec(V, 5, output_relu_ok=True)["output_relu"] is True


def _config(d=5, widths=(10, 10), h_kind=None, drift_kind=None):
    c = nat.GenlConfig()
    c.base.d, c.base.K_local, c.base.N = d, 48, 20
    c.base.dt, c.base.sqrt_dt, c.base.T, c.base.sigma_scale = 0.001, 0.001 ** 0.5, float("inf"), 2 ** 0.5
    c.base.domain_kind, c.base.dom_a, c.base.dom_b = nat.DOM_BOX, 0.0, 2 * math.pi
    c.base.h_kind = nat.GH_EIG_NLS if h_kind is None else h_kind
    c.base.drift_kind = nat.DRIFT_ZERO if drift_kind is None else drift_kind
    c.base.h_par[0], c.base.h_par[1] = 0.8, float(d)
    c.base.store_path = 1
    c.n_hidden = len(widths)
    for i, w in enumerate(widths):
        c.widths[i] = w
    return c


def _eig(**kw):
    e = nat.GenlEig(struct_bytes=C.sizeof(nat.GenlEig))
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def test_query_eig_accepts_and_refuses_without_a_gpu():
    lib = nat.load()
    sz, sz0 = nat.GenlSizes(), nat.GenlSizes()
    keep = torch.zeros(5)
    # accepted: the two problems; the sizes are those of the plain query of the same net
    assert lib.psp_genl_query_eig(C.byref(_config()), C.byref(_eig(output_relu=1)), C.byref(sz)) == 0, nat.last_error()
    plain = _config(h_kind=nat.GH_ALLEN_CAHN)
    assert lib.psp_genl_query(C.byref(plain), C.byref(sz0)) == 0
    for f in ("table_bytes", "path_bytes", "ahat_bytes", "n_params", "grad_partial_bytes", "n_blocks", "waves_per_tile"):
        assert getattr(sz, f) == getattr(sz0, f), f
    fp = _config(h_kind=nat.GH_EIG_FP, drift_kind=nat.DRIFT_EIG_FP)
    fp.base.drift = nat.ptr(keep)
    assert lib.psp_genl_query_eig(C.byref(fp), C.byref(_eig()), C.byref(sz)) == 0, nat.last_error()
    # a NULL struct is psp_genl_query: the same sizes, and the same refusal of the kinds only the struct admits
    assert lib.psp_genl_query_eig(C.byref(plain), None, C.byref(sz)) == 0 and sz.table_bytes == sz0.table_bytes
    for cfg in (_config(), fp):
        assert lib.psp_genl_query(C.byref(cfg), C.byref(sz)) == -1 and "psp_genl_eig" in nat.last_error()
        assert lib.psp_genl_query_eig(C.byref(cfg), None, C.byref(sz)) == -1
        assert lib.psp_genl_query_lq(C.byref(cfg), None, C.byref(sz)) == -1

    def refused(cfg, eig, word):
        assert lib.psp_genl_query_eig(C.byref(cfg), C.byref(eig), C.byref(sz)) == -1
        assert word in nat.last_error(), nat.last_error()
    refused(_config(), _eig(struct_bytes=8), "struct_bytes")
    refused(_config(), _eig(output_relu=2), "output_relu")
    dense = _config()
    dense.sigma_kind, dense.sigma = nat.GENL_SIGMA_DENSE, nat.ptr(torch.zeros(25))
    refused(dense, _eig(), "sigma = s I")
    refused(_config(h_kind=nat.GH_SINNORM2), _eig(), "sigma = s I")
    ad = _config()
    ad.base.adaptive = 1
    refused(ad, _eig(), "adaptive")
    refused(_config(h_kind=nat.GH_EIG_FP), _eig(), "PSP_DRIFT_EIG_FP")
    nov = _config(h_kind=nat.GH_EIG_FP, drift_kind=nat.DRIFT_EIG_FP)
    refused(nov, _eig(), "drift vector missing")
    bad = _config()
    bad.base.h_par[1] = 0.0
    refused(bad, _eig(), "h_par")
    for k in (10, 15, 18):
        refused(_config(h_kind=k), _eig(), "enum out of range")
    refused(_config(drift_kind=17), _eig(), "enum out of range")
    # the backward takes the forward's config as it is
    assert nat.GH_EIG_FP == 16 and nat.GH_EIG_NLS == 17 and nat.DRIFT_EIG_FP == 16
