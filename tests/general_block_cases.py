"""Blocks and cases of the per-block float64 gradient tests of the value-net kernels behind GeneralSolver.train / EllipticSolver.train:
the (d, H)-templated gen_* kernels (csrc/gen_kernels.h, plan_general_native.py) and the run-time-shaped genl_* kernels
(csrc/genl_kernels.h, plan_general_deep.py).  One table for tests/test_ref64_general.py (CPU: the judge, the conditions, the planted
errors) and tests/test_gpu_general_block_gradients.py (GPU).

Blocks.  The flat gradient is [W_1, b_1, .., W_out, b_out] in the net's registration order; layer i reads the concatenation
[x (d), t (parabolic only), h_1, .., h_{i-1}], so its weight splits into the row groups W{i}x, W{i}t, W{i}h{j} (columns, in
DenseNet_tanh's nn.Linear layout), and the output layer counts as a layer.  A block's error is max |g - g_ref| over the block divided
by max(max |g_ref| over the block, BLOCK_FLOOR max |g_ref|).

Cases.  The smallest shapes that reach every route (K <= 257, N <= 7); `route` is what the GPU test asserts on the plan.  A diffusion
loss whose h does not read y leaves the output bias without a domain gradient (dV(X_N)/db - dV(X_0)/db = 0), so those problems carry
the BSDE loss or loss_with_stopped here; alpha weighs the K_boundary-sized terms down until the kernels' part of every block is at
least half of it (asserted on the CPU).  `scale` multiplies the weight matrices and `bias_std` draws the biases of the dense-concat
nets (zero at initialisation), both sides from the same seeded generator, where the initial state leaves a block under the floor.

The bf16 modes (mlp_dtype 'bf16', 'bf16_fwd') stay out of CASES: against the exact float64 reference their documented bound is 2e-2
(tests/test_gpu_general_variants.py), a hundred times the per-block bound -- wide enough to have passed a weight table that overran
its LDS carve on every instance with d + 1 <= 12.  They have a table of their own, BF16_CASES, judged against the float64 reference
with bf16 OPERANDS (ref64_general.iteration(..., operands='bf16')) by tests/test_gpu_general_bf16_blocks.py: the kernels are held to
half the rounding error that reference predicts, on top of the fp32 bounds.

PHILOX_CASES is a table of its own for tests/test_gpu_general_philox_blocks.py: the same shapes on noise='philox', where other
compiled kernels run -- the PHILOX instances of gen_fwd_kernel, its specialised SPECK instances (unbounded, not adaptive: under
split products and bf16 only) and the counter branch of genl_fwd_kernel.  X_0 and t_0 come from a device generator there, so the
conditions on the reference are asserted by the GPU test itself.  Two bf16 cases are in it for the sake of their SPECK instances:
X_N and t_N, which no bf16 product touches, pin the noise to the fp32 bound."""
import copy
import dataclasses

import numpy as np
import torch

import ref64_general as r64
from util_cases import BLOCK_FLOOR, orc

BIAS_SEED = 11


# ---- blocks ------------------------------------------------------------------------------------------------------------------------
def general_grad_blocks(g, d, time_input, arch, linear=False, time_first=False):
    """(names, blocks) of the flat gradient of a value net (d [+ 1] -> 1, hidden widths `arch`).  linear: nn.Linear weights
    (out, in).  time_first: the input is [t, x] (Solver's value-function ansatz) instead of [x, t]."""
    g = g.detach().double().cpu().reshape(-1)
    t = 1 if time_input else 0
    dims = [d + t] + list(arch) + [1]
    names, blocks, off = [], [], 0
    for i in range(1, len(dims)):
        fan, out = sum(dims[:i]), dims[i]
        W = g[off:off + fan * out]
        off += fan * out
        W = W.view(out, fan).t() if linear else W.view(fan, out)         # rows = inputs
        xs, tr = (slice(1, d + 1), 0) if time_first else (slice(0, d), d)
        names.append("W%dx" % i)
        blocks.append(W[xs])
        if time_input:
            names.append("W%dt" % i)
            blocks.append(W[tr:tr + 1])
        r = d + t
        for j in range(1, i):
            names.append("W%dh%d" % (i, j))
            blocks.append(W[r:r + dims[j]])
            r += dims[j]
        assert r == fan
        names.append("b%d" % i)
        blocks.append(g[off:off + out])
        off += out
    assert off == g.numel(), (off, g.numel(), dims)
    return names, blocks


def general_block_errors(g, g_ref, *layout, **kw):
    names, ref = general_grad_blocks(g_ref, *layout, **kw)
    _, got = general_grad_blocks(g, *layout, **kw)
    floor = BLOCK_FLOOR * max(float(r.abs().max()) for r in ref)
    return names, [float((a - r).abs().max()) / max(float(r.abs().max()), floor, 1e-300) for a, r in zip(got, ref)]


def assert_general_blocks(g, g_ref, layout, bound, tag="", **kw):
    """Prints the block errors in one line, asserts each against `bound`, returns (names, errors)."""
    names, errs = general_block_errors(g, g_ref, *layout, **kw)
    print("%s blocks %s (<= %.3g)" % (tag, "  ".join("%s %.2e" % ne for ne in zip(names, errs)), bound))
    bad = [(n, e) for n, e in zip(names, errs) if not e <= bound]
    assert not bad, (tag, bad, bound)
    return names, errs


def layout(c):
    """(d, time_input, arch) and dict(linear=) of a case's net for the functions above."""
    return (c["problem"]["kwargs"]["d"], c["family"] != "elliptic", list(c["net"]["arch"])), dict(linear=c["net"]["kind"] == "densenet_tanh")


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def _c(cid, family, kind, kwargs, net, route, K=40, N=3, dt=0.01, loss="BSDE", adaptive=False, alpha=None, Kb=6, attrs=None,
       numpy_seed=None, stopped=False, mode=None, nw=None, scale=1.0, bias_std=0.0, early=False, seed=42, boundary_type=None,
       dense=None):
    solver = dict(seed=seed, delta_t=dt, N=N, lr=0.001, L=1, K=K, K_boundary=min(Kb, K), loss_method=loss,
                  adaptive_forward_process=adaptive, loss_with_stopped=stopped,
                  alpha=list(alpha or ([1.0, 1.0] if family == "elliptic" else [1.0, 1.0, 1.0])))
    if boundary_type is not None:
        solver["boundary_type"] = boundary_type
    c = dict(id=cid, name=cid, family=family, problem=dict(kind=kind, kwargs=dict(kwargs)), solver=solver, net=dict(net),
             route=route, mode=mode, nw=nw, scale=scale, bias_std=bias_std, early=early,
             dense="B" in kwargs if dense is None else dense)                 # a dense constant sigma
    if attrs:
        c["problem"]["attrs"] = dict(attrs)
    if numpy_seed is not None:
        c["numpy_seed"] = numpy_seed
    return c


def _relu2(H, seed=42):
    return dict(kind="densenet", arch=[H, H], seed=seed)


def random_B(d, seed):
    """Non-symmetric, entries O(1 / sqrt d)."""
    return torch.randn(d, d, generator=torch.Generator().manual_seed(seed)) / d ** 0.5


def _templated():
    out = []
    gen = lambda inst, mode: dict(plan="gen", inst=inst, mode=mode)
    ac = lambda d, T: ("general", "AllenCahn", dict(d=d, T=T, seed=42, modus="pt"))
    for mode in ("fp32", "f16x3"):
        # exact (6, 30): one input block, K = 257 (17 tiles, the last holds one trajectory), diffusion, not adaptive
        out.append(_c("gen-6x30-allencahn-K257-diff-%s" % mode, *ac(6, 0.105), _relu2(30), gen((6, 30), mode), K=257, N=7,
                      loss="diffusion", alpha=[1.0, 0.01, 1.0], Kb=10, mode=mode, scale=3.0, bias_std=0.1))
        # exact (10, 24): one input block, K = 40 (the last tile holds 8), BSDE, adaptive
        out.append(_c("gen-10x24-allencahn-K40-bsde-adp-%s" % mode, *ac(10, 0.045), _relu2(24), gen((10, 24), mode), K=40, N=3,
                      adaptive=True, mode=mode, scale=3.0, bias_std=0.1))
        # exact (100, 64): seven input blocks, element-wise drift
        out.append(_c("gen-100x64-dwell-K40-bsde-%s" % mode, "general", "DoubleWell_multidim_for_general_solver",
                      dict(d=100, d_1=50, d_2=50, T=0.045, eta=0.1, kappa=0.5, modus="HJB"), _relu2(64), gen((100, 64), mode),
                      K=40, N=3, mode=mode, bias_std=0.1))
        # d = 7, H = 20, padded: elliptic (the kernels' time row stays zero), Neumann, K = 16.  The plan takes the cheapest instance
        # that covers the shape (native_shapes.gen_candidates), which is (10, 24), not (16, 32); the box below runs on (16, 32)
        out.append(_c("gen-7x20-expball-K16-ell-neumann-%s" % mode, "elliptic", "ExponentialOnBallNonlinearSin",
                      dict(d=7, alpha=0.3, boundary_type="Neumann"), _relu2(20), gen((10, 24), mode), K=16, N=5, dt=0.005,
                      loss="diffusion", alpha=[1.0, 1e-4], boundary_type="Neumann", mode=mode, scale=3.0, bias_std=0.1))
        # d = 33, H = 40 padded onto (48, 48): three input blocks, a sphere with early exits, adaptive
        out.append(_c("gen-33x40-sphere-K40-bsde-adp-%s" % mode, "general_bounded", "ExponentialOnSphereNonlinearParabolic",
                      dict(d=33, T=0.0105, alpha=0.3), _relu2(40), gen((48, 48), mode), K=40, N=7, dt=0.001,
                      adaptive=True, mode=mode, scale=2.0, bias_std=0.1, early=True))
    # K = 1
    out.append(_c("gen-10x24-allencahn-K1-bsde-fp32", *ac(10, 0.045), _relu2(24), gen((10, 24), "fp32"), K=1, N=3, Kb=1, mode="fp32",
                  scale=3.0, bias_std=0.1))
    out.append(_c("gen-10x24-allencahn-K1-bsde-f16x3", *ac(10, 0.045), _relu2(24), gen((10, 24), "f16x3"), K=1, N=3, Kb=1,
                  mode="f16x3", adaptive=True, scale=3.0, bias_std=0.1))
    # d = 15, H = 20 on (16, 32), the time row alone in the second input block: a box with loss_with_stopped
    for mode in ("fp32", "f16x3"):
        out.append(_c("gen-15x20-box-K40-diff-stopped-%s" % mode, "general_bounded", "QuadraticOnBox",
                      dict(d=15, T=0.105, X_l=-1.0, X_r=1.0, one_boundary=False, scale=1.0, quad_h=True), _relu2(20),
                      gen((16, 32), mode), K=40, N=7, loss="diffusion", alpha=[1.0, 0.01, 0.01], stopped=True, numpy_seed=9,
                      mode=mode, scale=2.0, bias_std=0.1, early=True))
    return out


def _runtime_shaped():
    out = []
    genl = lambda fwd, bwd: dict(plan="genl", fwd=fwd, bwd="genl_bwd_kernel<%s>" % bwd)
    ac = lambda d, T=0.045: ("general", "AllenCahn", dict(d=d, T=T, seed=42, modus="pt"))
    dw = lambda d, T=0.045: ("general", "DoubleWell_multidim_for_general_solver",
                             dict(d=d, d_1=d // 2, d_2=d - d // 2, T=T, eta=0.1, kappa=0.5, modus="HJB"))
    net = lambda kind, arch, seed=42: dict(kind=kind, arch=list(arch), seed=seed)
    # depth 1, d_in = 2, one wave
    out.append(_c("genl-d1-a17-relu2", *ac(1), net("densenet", [17]), genl(1, "1"), adaptive=True, scale=3.0, bias_std=0.1))
    # depth 2 with a one-unit layer, d_in = 16, six hidden blocks forced onto one wave
    out.append(_c("genl-d15-a65x1-tanh-nw1", *ac(15, 0.135), net("densenet_concat_tanh", [65, 1]), genl(1, "1"), nw="1", dt=0.03, loss="diffusion",
                  alpha=[1.0, 1e-3, 1.0], scale=3.0, bias_std=0.1))
    # depth 3, d_in = 17, tanh^2, eight waves; the same net under four waves
    out.append(_c("genl-d16-a33x17x17-tanh2", "general", "HeatEquation", dict(d=16, T=0.045, seed=42), net("user_tanh2", [33, 17, 17]),
                  genl(8, "8, 3"), scale=3.0, bias_std=0.1))
    out.append(_c("genl-d16-a33x17x17-tanh2-nw4", "general", "HeatEquation", dict(d=16, T=0.045, seed=42),
                  net("user_tanh2", [33, 17, 17]), genl(4, "8, 3"), nw="4", adaptive=True, scale=3.0, bias_std=0.1))
    # the nn.Linear layout, four waves
    out.append(_c("genl-d16-a65x33-linear-nw4", *dw(16), net("densenet_tanh", [65, 33]), genl(4, "8, 3"), nw="4"))
    # width 110, relu^2, diffusion, adaptive
    out.append(_c("genl-d10-a110x17-relu2", *ac(10, 0.135), net("densenet", [110, 17]), genl(8, "8, 3"), dt=0.03, loss="diffusion", adaptive=True,
                  alpha=[1.0, 1e-4, 1.0], scale=2.0, bias_std=0.1))
    # HBsum = 24 and 25: the three- and the four-slot eight-wave backward
    out.append(_c("genl-d20-a128x3-relu2", *ac(20), net("densenet", [128, 128, 128]), genl(8, "8, 3"), K=33, bias_std=0.1))
    out.append(_c("genl-d20-a128x3x16-tanh", *ac(20), net("densenet_concat_tanh", [128, 128, 128, 16]), genl(8, "8, 4"), K=33,
                  adaptive=True, scale=2.0, bias_std=0.1))
    # d_in = 112 with 4 x 128: the largest images
    out.append(_c("genl-d111-a128x4-tanh2", *dw(111, 0.03), net("user_tanh2", [128, 128, 128, 128]), genl(8, "8, 4"), K=24, N=2,
                  scale=1.5, bias_std=0.1))
    # a dense sigma on an elliptic box, BSDE
    out.append(_c("genl-d5-a33-box-dense-sigma", "elliptic", "QuadraticOnBox",
                  dict(d=5, X_l=-1.0, X_r=1.0, one_boundary=False, parabolic=False, quad_h=True, B=random_B(5, 3).tolist()),
                  net("densenet", [33]), genl(1, "1"), K=40, N=5, numpy_seed=9, adaptive=True, scale=3.0, bias_std=0.1))
    # a one-sided box with a dense sigma, parabolic
    out.append(_c("genl-d4-a17x33-upper-box-dense-sigma", "general_bounded", "QuadraticOnBox",
                  dict(d=4, T=0.075, X_l=-1.0, X_r=0.7, one_boundary=True, scale=1.0, quad_h=False, B=random_B(4, 5).tolist()),
                  net("densenet_concat_tanh", [17, 33]), genl(1, "1"), K=40, N=5, numpy_seed=9, scale=3.0, bias_std=0.1))
    # a sphere on which every trajectory runs out of time before step N: tiles leave the time loop early, and so does the loop
    out.append(_c("genl-d3-a17x17-sphere-early", "general_bounded", "ExponentialOnSphereNonlinearParabolic",
                  dict(d=3, T=0.028, alpha=0.3), net("densenet_tanh", [17, 17]), genl(1, "1"), K=40, N=7, loss="diffusion",
                  alpha=[1.0, 1e-4, 1e-4], early=True))
    # BSDE with a Neumann boundary: the residual at the last executed step's points
    out.append(_c("genl-d3-a17-sphere-bsde-neumann", "general_bounded", "ExponentialOnSphereNonlinearParabolic",
                  dict(d=3, T=0.105, alpha=0.03), net("densenet", [17]), genl(1, "1"), K=40, N=7,
                  attrs=dict(boundary_type="Neumann"), scale=3.0, bias_std=0.1))
    # the remaining h of the catalogue: the linear and the squared exponential-on-the-ball problems, and the full Hessian (a dense
    # sigma = sqrt(2 / d) ones(d, d) with (sum_i x_i)^2 in h)
    out.append(_c("genl-d2-a17-expsphere-lin", "elliptic", "ExponentialOnSphere", dict(d=2, alpha=0.3), net("densenet", [17]),
                  genl(1, "1"), K=40, N=5, dt=0.02, loss="diffusion", alpha=[1.0, 1e-5], scale=3.0, bias_std=0.1))
    out.append(_c("genl-d5-a17x17-expball-sq", "elliptic", "ExponentialOnBallNonlinear", dict(d=5, alpha=0.3),
                  net("densenet_concat_tanh", [17, 17]), genl(1, "1"), K=40, N=5, dt=0.005, adaptive=True, scale=3.0, bias_std=0.1))
    out.append(_c("genl-d4-a17x17-expball-hessian", "elliptic", r64.HESS, dict(d=4, alpha=0.3), net("densenet_tanh", [17, 17]),
                  genl(1, "1"), K=40, N=5, dt=0.005, loss="diffusion", alpha=[1.0, 1e-4], dense=True))
    # the annulus and the cut corner (EllipticSolver)
    out.append(_c("genl-d3-a17x17-annulus", "elliptic", "Committor", dict(d=3), net("user_tanh2", [17, 17]), genl(1, "1"), K=64, N=5,
                  dt=0.02, scale=3.0, bias_std=0.1))
    out.append(_c("genl-d3-a33-corner", "elliptic", "QuadraticOnBox",
                  dict(d=3, X_l=-1.0, X_r=1.0, one_boundary=False, parabolic=False, quad_h=True), net("densenet", [33]), genl(1, "1"),
                  K=40, N=5, dt=0.02, attrs=dict(boundary="square-corner", X_corner=0.2), numpy_seed=9, scale=3.0, bias_std=0.1))
    return out


def _planted():
    """Two cases for the planted errors of tests/test_ref64_general.py only (no GPU run): Allen-Cahn on the dense-concat relu^2 nets
    with the weight matrices HALVED and the biases zero as initialised, where the hidden-to-hidden rows and the time rows are 1e-4 ..
    5e-4 of the whole gradient's maximum -- the regime in which the whole-gradient criterion is blind."""
    ac = lambda d: ("general", "AllenCahn", dict(d=d, T=0.035, seed=42, modus="pt"))
    none = dict(plan=None)
    return [_c("plant-d2-a128x128", *ac(2), dict(kind="densenet", arch=[128, 128], seed=42), none, K=40, adaptive=True, Kb=10, scale=0.5),
            _c("plant-d10-a24x24-K257", *ac(10), _relu2(24), none, K=257, adaptive=True, Kb=10, scale=0.5)]


CASES = _templated() + _runtime_shaped()
PLANTED = {c["id"]: c for c in _planted()}
assert len({c["id"] for c in CASES}) == len(CASES)
BY_ID = {c["id"]: c for c in CASES}


# ---- cases on the kernels' own Philox noise ----------------------------------------------------------------------------------------
SPEC_ALLEN_CAHN, SPEC_DWELL = "ZERO|ALLEN_CAHN", "DWELL|QUAD"          # the SPECK kinds of gen_fwd_kernel (GenLaunch::spec_kind)


def _philox(c, it=0, spec=None):
    """The case on noise='philox' (tests/test_gpu_general_philox_blocks.py): `it` is the iteration that is judged (L = it + 1 are
    trained), route['spec'] the SPECK kind of the specialised forward instance the launch must take, or None."""
    c = copy.deepcopy(c)
    c["id"] = c["name"] = "philox-%s%s" % (c["id"], "-it%d" % it if it else "")
    c["noise"], c["it"] = "philox", it
    c["solver"]["L"] = it + 1
    c["route"]["spec"] = spec
    return c


def _philox_templated():
    """Specialised instances (unbounded, not adaptive, the path store on: split products under 'auto', and bf16), then the PHILOX
    instances off the specialisation (fp32; split products with the adaptive shift or a bounded domain)."""
    x3 = "f16x3"
    gen = lambda inst, mode: dict(plan="gen", inst=inst, mode=mode)
    ac = lambda d, T=0.045: ("general", "AllenCahn", dict(d=d, T=T, seed=42, modus="pt"))
    dw = lambda d: ("general", "DoubleWell_multidim_for_general_solver",
                    dict(d=d, d_1=d // 2, d_2=d - d // 2, T=0.045, eta=0.1, kappa=0.5, modus="HJB"))
    ac10 = lambda cid, mode, **kw: _c(cid, *ac(10), _relu2(24), gen((10, 24), mode), N=3, mode=mode, scale=3.0, bias_std=0.1, **kw)
    dw100 = lambda cid, mode, **kw: _c(cid, *dw(100), _relu2(64), gen((100, 64), mode), K=40, N=3, mode=mode, bias_std=0.1, **kw)
    out = []
    # ---- spec<D, H>: exact (6, 30), (10, 24) at K = 1 and 40, (100, 64); padded (16, 32) -- the time row alone in the second input
    # block -- and (48, 48) -- three state blocks, the last with 15 zero-padded features
    out.append(_philox(BY_ID["gen-6x30-allencahn-K257-diff-f16x3"], spec=SPEC_ALLEN_CAHN))
    out.append(_philox(ac10("gen-10x24-allencahn-K1-bsde-plain-f16x3", x3, K=1, Kb=1), spec=SPEC_ALLEN_CAHN))
    k40 = ac10("gen-10x24-allencahn-K40-bsde-f16x3", x3, K=40)
    out += [_philox(k40, spec=SPEC_ALLEN_CAHN), _philox(k40, it=1, spec=SPEC_ALLEN_CAHN)]
    out.append(_philox(_c("gen-15x20-allencahn-K40-bsde-f16x3", *ac(15), _relu2(20), gen((16, 32), x3), K=40, N=3, mode=x3, scale=2.0,
                          bias_std=0.1), spec=SPEC_ALLEN_CAHN))
    out += [_philox(BY_ID["gen-100x64-dwell-K40-bsde-f16x3"], spec=SPEC_DWELL),
            _philox(BY_ID["gen-100x64-dwell-K40-bsde-f16x3"], it=1, spec=SPEC_DWELL)]
    out.append(_philox(_c("gen-33x40-dwell-K40-bsde-f16x3", *dw(33), _relu2(40), gen((48, 48), x3), K=40, N=3, mode=x3, scale=2.0,
                          bias_std=0.1), spec=SPEC_DWELL))
    # ---- the same two kinds on the bf16 products (judged by the bf16 bounds; X_N and t_N never pass through a bf16 product)
    out.append(_philox(ac10("gen-10x24-allencahn-K40-bsde-bf16", "bf16", K=40), spec=SPEC_ALLEN_CAHN))
    out.append(_philox(dw100("gen-100x64-dwell-K40-bsde-bf16", "bf16"), spec=SPEC_DWELL))
    # (6, 30), d + 1 = 7: two k-steps on the input side, where the bf16 image of a weight table is twice its fp32 image (GGeo::tbl)
    out.append(_philox(_c("gen-6x30-allencahn-K257-diff-bf16", *ac(6, 0.105), _relu2(30), gen((6, 30), "bf16"), K=257, N=7,
                          loss="diffusion", alpha=[1.0, 0.01, 1.0], Kb=10, mode="bf16", scale=3.0, bias_std=0.1), spec=SPEC_ALLEN_CAHN))
    # ---- gen_fwd_kernel<D, H, false, true> (fp32) and <D, H, false, true, true> (split products) off the specialisation
    for cid in ("gen-6x30-allencahn-K257-diff-fp32", "gen-7x20-expball-K16-ell-neumann-fp32", "gen-10x24-allencahn-K40-bsde-adp-f16x3",
                "gen-33x40-sphere-K40-bsde-adp-f16x3", "gen-15x20-box-K40-diff-stopped-f16x3"):
        out.append(_philox(BY_ID[cid]))
    out.append(_philox(dw100("gen-100x64-dwell-K40-bsde-adp-f16x3", x3, adaptive=True)))
    return out


def _philox_runtime_shaped():
    """Every run-time-shaped case, and two of them on the second iteration (iter = 1 in the counters): four waves with the adaptive
    shift, and d = 111 -- seven noise blocks, the last with 15 features -- on eight."""
    rt = _runtime_shaped()
    by = {c["id"]: c for c in rt}
    return [_philox(c) for c in rt] + [_philox(by[cid], it=1) for cid in ("genl-d16-a33x17x17-tanh2-nw4", "genl-d111-a128x4-tanh2")]


PHILOX_CASES = _philox_templated() + _philox_runtime_shaped()
assert len({c["id"] for c in PHILOX_CASES}) == len(PHILOX_CASES)
PHILOX_BY_ID = {c["id"]: c for c in PHILOX_CASES}
# the forward of rows 20 .. 39 alone (k_offset = 20, no multiple of 16): a specialised templated instance and a run-time-shaped case
PHILOX_SHARD_IDS = ("philox-gen-10x24-allencahn-K40-bsde-f16x3", "philox-genl-d16-a33x17x17-tanh2-nw4")


# ---- the bf16 forward mode ----------------------------------------------------------------------------------------------------------
def _bf16_cases():
    """GeneralSolver(mlp_dtype='bf16_fwd'): gen_fwd_kernel<D, H, /*BF16*/true, ..> and the fp32 gen_bwd2_kernel behind it.  Supplied
    noise: the three exact instances with d + 1 <= 12, whose input-side bf16 tables are larger than the fp32 ones (GGeo::tbl); the
    exact (16, 16) -- the time row alone in the second input block, one hidden block: a zero-filled half k-step on every product;
    d = 33, H = 40 padded onto (48, 48).  Philox noise: the two SPECK instances at (100, 64); off the specialisation the adaptive
    shift (bf16 products move the state) and a sphere with early exits.  All on the dense-concat relu^2 net: the templated plan takes
    no other (DenseNet_tanh runs on the genl_* kernels, which decline the bf16 modes: tests/test_gpu_general_bf16_blocks.py)."""
    m = "bf16_fwd"
    gen = lambda inst: dict(plan="gen", inst=inst, mode=m)
    ac = lambda d, T=0.045: ("general", "AllenCahn", dict(d=d, T=T, seed=42, modus="pt"))
    dw = lambda d: ("general", "DoubleWell_multidim_for_general_solver",
                    dict(d=d, d_1=d // 2, d_2=d - d // 2, T=0.045, eta=0.1, kappa=0.5, modus="HJB"))
    kw = dict(mode=m, bias_std=0.1)
    sup = [_c("bf16-gen-6x30-allencahn-K257-diff", *ac(6, 0.105), _relu2(30), gen((6, 30)), K=257, N=7, loss="diffusion",
              alpha=[1.0, 0.01, 1.0], Kb=10, scale=3.0, **kw),
           _c("bf16-gen-10x24-allencahn-K40-bsde", *ac(10), _relu2(24), gen((10, 24)), K=40, N=3, scale=3.0, **kw),
           _c("bf16-gen-10x32-allencahn-K37-bsde", *ac(10), _relu2(32), gen((10, 32)), K=37, N=3, scale=3.0, **kw),
           _c("bf16-gen-16x16-allencahn-K40-bsde", *ac(16), _relu2(16), gen((16, 16)), K=40, N=3, scale=3.0, **kw),
           _c("bf16-gen-33x40-dwell-K40-bsde", *dw(33), _relu2(40), gen((48, 48)), K=40, N=3, scale=2.0, **kw)]
    for c in sup:
        c["noise"], c["it"] = "reference", 0
        c["route"]["spec"] = None
    phx = [# (net seed 5: with 42 one relu^2 pre-activation of the oracle's draws lies within 4 fp32 roundings of zero)
           _philox(_c("bf16-gen-100x64-allencahn-K40-bsde", *ac(100), _relu2(64, seed=5), gen((100, 64)), K=40, N=3, **kw), spec=SPEC_ALLEN_CAHN),
           _philox(_c("bf16-gen-100x64-dwell-K40-bsde", *dw(100), _relu2(64), gen((100, 64)), K=40, N=3, **kw), spec=SPEC_DWELL),
           _philox(_c("bf16-gen-10x24-allencahn-K40-bsde-adp", *ac(10), _relu2(24), gen((10, 24)), K=40, N=3, adaptive=True, scale=3.0, **kw)),
           _philox(_c("bf16-gen-33x40-sphere-K40-bsde-adp", "general_bounded", "ExponentialOnSphereNonlinearParabolic",
                      dict(d=33, T=0.0105, alpha=0.3), _relu2(40), gen((48, 48)), K=40, N=7, dt=0.001, adaptive=True, scale=2.0,
                      early=True, **kw))]
    return sup + phx


def _bf16_full_cases():
    """GeneralSolver(mlp_dtype='bf16'): the same forward instances with the bf16-pair path store, and gen_bwd2_kernel<D, H, /*BF16*/
    true> -- every case of BF16_CASES again, and K = 299 over N = 20 steps on (10, 24): 19 tiles, the last with 11 trajectories,
    399 sample blocks, i.e. a hundred backward rounds of four."""
    out = []
    for c in _bf16_cases():
        c = copy.deepcopy(c)
        c["id"] = c["name"] = c["id"].replace("bf16-gen", "bf16full-gen")
        c["mode"] = c["route"]["mode"] = "bf16"
        out.append(c)
    c = _c("bf16full-gen-10x24-allencahn-K299-N20-bsde", "general", "AllenCahn", dict(d=10, T=0.215, seed=42, modus="pt"), _relu2(24),
           dict(plan="gen", inst=(10, 24), mode="bf16", spec=None), K=299, N=20, mode="bf16", scale=3.0, bias_std=0.1)
    c["noise"], c["it"] = "reference", 0
    return out + [c]


def bf16_reference(c, oprob, net, draws):
    """The float64 model of the case's mode on the given draws: bf16 operands in the forward sweeps, and for the full 'bf16' mode
    the kernel's backward with its rounding points."""
    return r64.iteration(c, oprob, net, draws, operands="bf16", backward="bf16" if c["mode"] == "bf16" else "autograd")


BF16_CASES = _bf16_cases()
BF16_FULL_CASES = _bf16_full_cases()
assert len({c["id"] for c in BF16_CASES + BF16_FULL_CASES}) == len(BF16_CASES) + len(BF16_FULL_CASES)
BF16_C = 0.5                # tests/test_gpu_general_bf16_blocks.py; the CPU stand-in is held to half of it
BF16_PRODUCT_BLOCKS = ("W1x", "W2x", "W2h1")        # the weight blocks of the bf16 products (W3 enters by fp32 dot products)


def bf16_errors(c, got, model, exact):
    """(e_kernel, e_model): dicts over YN, VN, XN, tN (of max(1, max |.|)), loss (relative) and `blocks` (names, errors), e_kernel =
    |got - model|, e_model = |model - exact|.  For the loss e_model is max(e_model(loss), e_model(YN)): one realised scalar
    difference can cancel by chance."""
    lay, kw = layout(c)

    def errs(a, r):
        out = {}
        for name in ("YN", "VN", "XN", "tN"):
            g, want = a[name].double().cpu(), r[name].double()
            assert g.shape == want.shape and bool(torch.isfinite(g).all()), name
            out[name] = float((g - want).abs().max()) / max(1.0, float(want.abs().max()))
        out["loss"] = abs(a["loss"] - r["loss"]) / abs(r["loss"])
        out["blocks"] = general_block_errors(a["grad"], r["grad"], *lay, **kw)
        return out
    ek, em = errs(got, model), errs(model, exact)
    em["loss"] = max(em["loss"], em["YN"])
    return ek, em


def assert_bf16(c, got, model, exact, coeff, d_tol, loss_tol, block_tol, tag=""):
    """e_kernel <= coeff e_model + (the fp32 siblings' bound) for YN, VN, the loss and every block; X_N and t_N likewise where a bf16
    product reaches the state (the adaptive shift) and to the plain fp32 bound where none does.  Prints every figure first."""
    ek, em = bf16_errors(c, got, model, exact)
    moved = c["solver"]["adaptive_forward_process"]
    rows = [(n, ek[n], em[n], d_tol) for n in ("YN", "VN")] + [(n, ek[n], em[n] if moved else 0.0, d_tol) for n in ("XN", "tN")]
    rows += [("loss", ek["loss"], em["loss"], loss_tol)]
    rows += [(n, a, b, block_tol) for n, a, b in zip(ek["blocks"][0], ek["blocks"][1], em["blocks"][1])]
    print("%s  " % tag + "  ".join("%s %.2e/%.2e" % r[:3] for r in rows) + "   (e_kernel/e_model)")
    bad = [r for r in rows if not r[1] <= coeff * r[2] + r[3]]
    assert not bad, (tag, coeff, bad)
    return ek, em


# ---- the oracle side ---------------------------------------------------------------------------------------------------------------
def oracle_problem(c):
    """orc.make_problem of the case; a 'B' keyword (QuadraticOnBox) becomes the oracle's dense constant sigma."""
    kw = dict(c["problem"]["kwargs"])
    kw.update(c["problem"].get("attrs", {}))
    B = kw.pop("B", None)
    if c["problem"]["kind"] == r64.HESS:                         # (not among the oracle's constructors: the sine problem with its own B and h)
        d, al = kw["d"], kw.get("alpha", 1.0)
        base = orc.make_problem("ExponentialOnBallNonlinearSin", **kw)
        B = (2.0 / d) ** 0.5 * torch.ones(d, d)

        def h(x, y, z):
            return -2 * al * y * (2 * al * torch.sum(x, 1) ** 2 + d) + torch.sin(torch.exp(2 * al * torch.sum(x ** 2, 1)) - y ** 2)
        return dataclasses.replace(base, kind=r64.HESS, B=B, sigma=lambda x: B, h=h)
    pb = orc.make_problem(c["problem"]["kind"], **kw)
    if B is None:
        return pb
    B = torch.as_tensor(B, dtype=torch.float32)
    return dataclasses.replace(pb, B=B, sigma=lambda x: B)


def prepare_net(c, net):
    """Weight matrices x scale; with bias_std > 0 the biases N(0, bias_std) from one seeded CPU generator in parameter order -- the
    same numbers on the oracle's net and on the package's."""
    gen = torch.Generator().manual_seed(BIAS_SEED)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                if c["bias_std"] > 0:
                    p.copy_((torch.randn(p.shape, generator=gen) * c["bias_std"]).to(p.device))
            elif c["scale"] != 1.0:
                p.mul_(c["scale"])


def _oracle_config(c):
    s = c["solver"]
    common = dict(K=s["K"], N=s["N"], delta_t=s["delta_t"], lr=s["lr"], L=1, seed=s["seed"], K_boundary=s["K_boundary"],
                  loss_method=s["loss_method"], adaptive_forward_process=s["adaptive_forward_process"],
                  loss_with_stopped=s["loss_with_stopped"])
    if c["family"] == "elliptic":
        return orc.EllipticConfig(alpha=tuple(s["alpha"]), boundary_type=s.get("boundary_type", "Dirichlet"), **common)
    return orc.GeneralConfig(alpha=tuple(s["alpha"]), **common)


def reference_net(c, flat=None):
    """(oracle problem, ref64_general.net64 of the oracle-built net after prepare_net) of a case, as runs() takes them, without an
    oracle run.  flat: a flat parameter vector in registration order -- the package's before a later iteration -- loaded into it."""
    oprob, cfg = oracle_problem(c), _oracle_config(c)
    V = (orc.elliptic_build if c["family"] == "elliptic" else orc.general_build)(oprob, cfg, net=c["net"])
    prepare_net(c, V)
    net = r64.net64(V)
    if flat is not None:
        flat = flat.detach().to(device="cpu", dtype=r64.F64).reshape(-1)
        assert flat.numel() == sum(p.numel() for p in net["params"])
        off = 0
        with torch.no_grad():
            for p in net["params"]:
                p.copy_(flat[off:off + p.numel()].view_as(p))
                off += p.numel()
    return oprob, net


_RUNS = {}


def runs(c):
    """dict(oprob, net (ref64_general.net64), trace (the fp32 oracle's first iteration), loss32, K_log32, ref (ref64_general.iteration on the oracle's draws)) of
    a case, computed once and never modified.  The float64 net is taken before the oracle's Adam step."""
    if c["id"] not in _RUNS:
        torch.set_num_threads(4)
        oprob, cfg = oracle_problem(c), _oracle_config(c)
        elliptic = c["family"] == "elliptic"
        V = (orc.elliptic_build if elliptic else orc.general_build)(oprob, cfg, net=c["net"])
        prepare_net(c, V)
        net = r64.net64(V)
        if "numpy_seed" in c:
            np.random.seed(c["numpy_seed"])
        out = (orc.elliptic_train if elliptic else orc.general_train)(oprob, cfg, V=V, trace=True)
        tr = out["traces"][0]
        _RUNS[c["id"]] = dict(oprob=oprob, trace=tr, net=net, loss32=out["loss_log"][0], K_log32=out["K_log"][0],
                              ref=r64.iteration(c, oprob, net, tr))
    return _RUNS[c["id"]]
