"""Cases of the float64 tests of the eigenvalue kernels (psp_genl_rollout_fwd_eig + psp_genl_rollout_bwd; csrc/genl_kernels.h, EIG
instances): one table for tests/test_ref64_eigenvalue.py (CPU: the judge against the fp32 composite plan, the conditions, the planted
error) and tests/test_gpu_eigenvalue_blocks.py (GPU, through the C ABI).

Shapes: d = 5 and 10 (the notebooks'), 17 (crosses a 16-feature block) and 2 (where half of the trajectories leave at
delta_t = 0.05); K = 40 (ragged last tile) and 48; N = 20; the notebooks' nets -- relu^2 [10] * 4 and [15] * 4, tanh with nn.Linear
[15] * 4 --, single-hidden-layer nets, and [40] * 3 (nine hidden blocks: the eight- and four-wave instances of the forward kernel;
the notebooks' nets all run on the one-wave instance); delta_t = 0.001 and 0.05; both problems; lambda at the notebooks' initial values.
Gate.  The 'init' cases carry the notebooks' initialisations, whatever share of the gates they close; the 'drawn' cases draw
weights and biases from a seeded generator, scale the output layer so that o has unit spread over the points the rollout evaluates,
and then set the OUTPUT bias into the widest gap between neighbouring values of o in the central 40 % of those points -- the state path carries no parameter, so those points do not move with the bias.  The CPU test
asserts on the float64 reference that 20 - 80 % of the evaluated o are negative and min |o| >= 1e-5, and min exit margin >= 1e-5.
Draws.  In EigenvalueSolver's order from torch.manual_seed / np.random.seed: [X_2 = rand(K, d) for 'l2'], the boundary pair,
X_0 = rand(K, d) scaled to the box, N x randn(K, d)."""
import math

import numpy as np
import torch

import ref64_eigenvalue as r64
from util_cases import psp

N = 20
KB = 20
ALPHA = [50.0, 1.0]
MIN_MARGIN = 1e-5


def _c(cid, kind, d, K, net, dt, gate, lam=None, relu=True, seed=42, nw=None, waves=1):
    """nw: PSP_GENL_NW for the GPU run (None: the library's own choice); waves: the forward waves per tile the GPU test asserts."""
    return dict(id=cid, kind=kind, d=d, K=K, net=net, dt=dt, gate=gate, relu=relu, seed=seed, nw=nw, waves=waves,
                lam=(0.5 if kind == "fp" else -2.0) if lam is None else lam)


RELU10, RELU15, TANH15 = ("relu2", [10] * 4, False), ("relu2", [15] * 4, False), ("tanh", [15] * 4, True)
CASES = [
    _c("fp-d5-K48-relu10-init", "fp", 5, 48, RELU10, 0.001, "init"),
    _c("fp-d10-K40-relu10-drawn-dt05", "fp", 10, 40, RELU10, 0.05, "drawn"),
    _c("nls-d5-K40-tanh15-drawn", "nls", 5, 40, TANH15, 0.001, "drawn"),
    _c("nls-d10-K48-relu15-init", "nls", 10, 48, RELU15, 0.001, "init"),
    _c("nls-d17-K40-relu15-drawn-dt05", "nls", 17, 40, RELU15, 0.05, "drawn"),
    _c("fp-d17-K48-tanh15-drawn", "fp", 17, 48, TANH15, 0.001, "drawn"),
    _c("fp-d5-K40-relu12x1-drawn-dt05", "fp", 5, 40, ("relu2", [12], False), 0.05, "drawn"),
    _c("nls-d5-K48-tanh20x1-drawn", "nls", 5, 48, ("tanh", [20], False), 0.001, "drawn"),
    _c("nls-d2-K48-relu10-drawn-dt05", "nls", 2, 48, RELU10, 0.05, "drawn"),
    _c("fp-d2-K40-tanh15-drawn-dt05", "fp", 2, 40, TANH15, 0.05, "drawn"),
    _c("fp-d10-K48-relu15-plain-dt05", "fp", 10, 48, RELU15, 0.05, "plain", relu=False),      # no output ReLU: lambda, S_k, the kinds alone
    # the notebooks' nets run one wave per tile; nine hidden blocks take the eight-wave instance, and PSP_GENL_NW=4 the four-wave one
    _c("fp-d10-K40-relu40x3-drawn-dt05-fwd8", "fp", 10, 40, ("relu2", [40] * 3, False), 0.05, "drawn", waves=8),
    _c("nls-d17-K48-tanh40x3-drawn-fwd4", "nls", 17, 48, ("tanh", [40] * 3, False), 0.001, "drawn", nw="4", waves=4),
]
GATED = [c for c in CASES if c["gate"] == "drawn"]


def problem(c, device="cpu"):
    return (psp.FokkerPlanckEigenvalue if c["kind"] == "fp" else psp.SchroedingerEigenvalue)(d=c["d"], device=device)


def normalisation(c):
    return "center" if c["kind"] == "fp" else "l2"


def draws(c):
    """The iteration's draws in EigenvalueSolver's order (fp32, CPU)."""
    from path_space_pde_solver_amd.eigenvalue_solver import sample_periodic_pair_host
    pb = problem(c)
    torch.manual_seed(c["seed"])
    np.random.seed(c["seed"])
    out = {}
    if normalisation(c) == "l2":
        out["X2"] = (pb.X_r - pb.X_l) * torch.rand(c["K"], c["d"]) + pb.X_l
    out["Xb"], out["Xr"] = sample_periodic_pair_host(pb, KB, c["d"])
    out["X0"] = (pb.X_r - pb.X_l) * torch.rand(c["K"], c["d"]) + pb.X_l
    out["xi"] = torch.stack([torch.randn(c["K"], c["d"]) for _ in range(N)])
    return out


def make_net(c, device="cpu"):
    """The case's net from the package's classes, with its parameters set (fp32).  'init': the notebooks' initialisation."""
    act, arch, linear = c["net"]
    d = c["d"]
    if c["gate"] == "init":
        if linear:
            return psp.DenseNet_tanh(d, 1, 0.001, arch=arch, output_relu=True).to(device)
        if c["kind"] == "fp":
            return psp.DenseNet(d, 1, 0.001, arch=arch, output_relu=True, bias_init=0.8).to(device)
        return psp.DenseNet(d, 1, 0.001, arch=arch, output_relu=True, weight_scale=0.01, weight_shift=0.01, bias_init=0.1).to(device)
    V = psp.DenseNet_tanh(d, 1, 0.001, arch=arch, output_relu=c["relu"]) if linear else \
        psp.DenseNet(d, 1, 0.001, arch=arch, activation=act, output_relu=c["relu"])
    g = torch.Generator().manual_seed(1000 + c["seed"])
    ps = list(V.parameters())
    with torch.no_grad():
        for p in ps:                                             # weights O(1 / sqrt(fan_in)), biases O(1): hidden units on both sides of zero
            if p.dim() == 2:
                fan = p.shape[1] if linear else p.shape[0]
                p.copy_(torch.randn(p.shape, generator=g) * (0.7 / math.sqrt(fan)))
            else:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
        ps[-1].zero_()
        # the output bias: minus the middle of the two central o over the evaluated points (they do not depend on the net)
        dr = draws(c)
        net = r64.net64(ps, act, linear, False)
        pts = visited_points(c, dr)
        ps[-2].div_(float(r64.linear_output(net, pts).std()))        # o = O(1): no term of h (y^3 in 'nls') swamps the others
        net = r64.net64(ps, act, linear, False)
        o = torch.sort(r64.linear_output(net, pts).detach()).values
        n = o.numel()                                            # (relu^2 nets give many points the same o: take the widest gap
        lo_, hi_ = (3 * n) // 10, (7 * n) // 10                  #  between neighbours in the central 40 %, not the median itself)
        gaps = o[lo_ + 1:hi_] - o[lo_:hi_ - 1]
        i = lo_ + int(torch.argmax(gaps))
        ps[-1].fill_(float(-(o[i] + o[i + 1]) / 2))
    return V.to(device)


def coeff_c(c):
    pb = problem(c)
    return pb.c.reshape(-1).double() if c["kind"] == "fp" else pb.c


def visited_points(c, dr):
    """Every point the rollout evaluates (the path carries no parameter): float64, (n_points, d)."""
    co = r64.coefficients(c["kind"], c["d"], coeff_c(c))
    dt, sq = r64.steps(c["dt"])
    sig, lo, hi = r64.f32(math.sqrt(2.0)), r64.f32(0.0), r64.f32(2 * math.pi)
    X = dr["X0"].double()
    stopped = torch.zeros(X.shape[0], dtype=torch.bool)
    pts = []
    for n in range(N):
        if not bool((~stopped).any()):
            break
        pts.append(X[~stopped].clone())
        Xp = X + (co["b"](X) * dt + sig * dr["xi"][n].double() * sq) * (~stopped).double().unsqueeze(1)
        inside = ((Xp >= lo) & (Xp <= hi)).all(1)
        X = torch.where((inside & ~stopped).unsqueeze(1), Xp, X)
        stopped = stopped | ~inside
    pts.append(X)
    return torch.cat(pts)


_CACHE = {}


def runs(c):
    """dict(draws, V (the fp32 net on the CPU), net (float64 leaves), ref (the float64 iteration: kernels' part only),
    full (with the boundary and normalisation terms)), computed once per case."""
    if c["id"] not in _CACHE:
        dr = draws(c)
        V = make_net(c)
        act, arch, linear = c["net"]
        params = [p for p in V.parameters()]
        net = r64.net64(params, act, linear, c["relu"])
        kw = dict(kind=c["kind"], d=c["d"], c=coeff_c(c), net=net, lam=c["lam"], draws=dr, delta_t=c["dt"], N=N, alpha=ALPHA)
        pb = problem(c)
        ref = r64.iteration(**kw)
        full = r64.iteration(normalisation=normalisation(c), X_center=pb.X_0, **kw)
        _CACHE[c["id"]] = dict(draws=dr, V=V, net=net, ref=ref, full=full, kw=kw)
    return _CACHE[c["id"]]


def layout(c):
    """(d, time_input, arch), dict(linear=) for general_block_cases.general_grad_blocks."""
    return (c["d"], False, list(c["net"][1])), dict(linear=c["net"][2])


def solver(c, V, device="cpu", backend="auto", **over):
    """EigenvalueSolver for the case with `V` swapped in: one iteration."""
    pb = problem(c, device)
    kw = dict(seed=c["seed"], delta_t=c["dt"], N=N, L=1, K=c["K"], K_boundary=KB, alpha=ALPHA, lambda_init=c["lam"], lambda_lr=0.01,
              normalisation=normalisation(c), verbose=False, device=device, backend=backend)
    kw.update(over)
    model = psp.EigenvalueSolver(pb, c["id"], **kw)
    model.V = V
    return pb, model
