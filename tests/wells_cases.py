"""The case table of tests/test_gpu_wells.py (GPU) and of the regime check in tests/test_ref64_wells.py (CPU): the coefficient kinds
of DoubleWell_OU (per-coordinate drift and terminal cost) and DoubleWell_multidim_2 (radial) on the DenseNet-control kernels
(csrc/hjbd_kernels.h), time_approx='outer', first iteration, against tests/ref64_wells.py.

As in tests/dense_block_cases.py the weight matrices are scaled and the biases drawn N(0, 0.1), so that every gradient block of every
per-step net carries signal.  Cases (class, d, H -> instance; K, N):
  a   OU d = 3, H = 16 -> (16, 32); K = 37, N = 4      ragged tile, the split inside block 0
  b   _2 d = 20, H = 30 -> (32, 32); K = 37, N = 4     r^2 over two 16-blocks and the four q-lanes
  c   OU d = 20 with native_spec()['split'] in {0, 1, 5, 17, 20}: both ends, a split in the second block
  d   OU and _2 d = 65, H = 30 -> (112, 32); K = 50, N = 4: seven blocks
  e   _2 d = 4, N = 1
  f   Philox noise, one fp32 and one f16x3 case
flags: 'det' (detach_forward=True), 'att' (the constructor defaults), 'non' (moment loss, non-adaptive), 'rel' (relative entropy,
attached).  Every case a .. e runs det, att and non in fp32 and in f16x3; a and b -- one per kind -- also run rel.  `refused`: the one
combination the C ABI answers -3 to (e, att, f16x3: the split-product adjoint sweep of (16, 32) does not carry the radial drift,
csrc/hjbd_kernels.h dnet_adj_x3_has_radial); the GPU test asserts that answer and that mlp_dtype='auto' runs the case in fp32.
"""
import torch

import dense_block_cases as dc
import ref64_wells
from util_cases import psp

DT = 0.05
FLAGS = dict(det=dict(loss="log-variance", adaptive=True, detach=True), att=dict(loss="log-variance", adaptive=True, detach=False),
             non=dict(loss="moment", adaptive=False, detach=False), rel=dict(loss="relative_entropy", adaptive=True, detach=False))


def _c(tag, cls, d, H, K, N, expect, flag, mode, split=None, noise="reference", scale=None, **kwargs):
    cid = "%s-%s-d%d-H%d-K%d-N%d-%s-%s%s%s" % (tag, cls, d, H, K, N, flag, mode, "" if split is None else "-split%d" % split,
                                              "-philox" if noise == "philox" else "")
    if scale is None:
        scale = 2.5 if d <= 4 else (0.8 if d <= 24 else 0.5)       # chosen on the CPU (tests/test_ref64_wells.py asserts the outcome)
    refused = cls == "DoubleWell_multidim_2" and expect == (16, 32) and mode == "f16x3" and flag in ("att", "rel")
    return dict(id=cid, cls=cls, d=d, H=H, K=K, N=N, expect=expect, flag=flag, mode=mode, split=split, noise=noise, kwargs=kwargs,
                scale=scale, bias_std=dc.BIAS_STD, refused=refused, **FLAGS[flag])


def _cases():
    out = []
    OU, RAD = "DoubleWell_OU", "DoubleWell_multidim_2"
    for mode in ("fp32", "f16x3"):
        for flag in ("det", "att", "non", "rel"):
            out.append(_c("a", OU, 3, 16, 37, 4, (16, 32), flag, mode, alpha=0.5, kappa=1.0))
            out.append(_c("b", RAD, 20, 30, 37, 4, (32, 32), flag, mode, alpha=1.0, kappa=0.5))
    for mode in ("fp32", "f16x3"):
        for flag in ("det", "att", "non"):
            for split in (0, 1, 5, 17, 20):
                out.append(_c("c", OU, 20, 30, 37, 4, (32, 32), flag, mode, split=split, alpha=0.5, kappa=1.0))
            for cls, kw in ((OU, dict(alpha=0.5, kappa=1.0)), (RAD, dict(alpha=1.0, kappa=0.5))):
                out.append(_c("d", cls, 65, 30, 50, 4, (112, 32), flag, mode, **kw))
            out.append(_c("e", RAD, 4, 30, 37, 1, (16, 32), flag, mode, alpha=1.0, kappa=1.0))
    out.append(_c("f", RAD, 20, 30, 37, 4, (32, 32), "att", "fp32", noise="philox", alpha=1.0, kappa=0.5))
    out.append(_c("f", OU, 3, 16, 37, 4, (16, 32), "att", "f16x3", noise="philox", alpha=0.5, kappa=1.0))
    return out


CASES = _cases()
IDS = [c["id"] for c in CASES]
assert len(set(IDS)) == len(IDS)


def problem(c, device):
    """The package's problem of the case; case c gives the OU instance another split (and the coefficient vectors to go with it)."""
    T = (c["N"] + 0.5) * DT                                    # floor(T / dt) = N whatever the rounding of N * dt
    pb = getattr(psp, c["cls"])(d=c["d"], T=T, device=device, **c["kwargs"])
    if c["split"] is not None:
        s, d = c["split"], c["d"]
        spec = pb.native_spec()
        gen = torch.Generator().manual_seed(31)
        kap = 0.5 + torch.rand(d, generator=gen)               # wells: kappa_i, eta_i; linear part: a_i < 0, alpha_i
        lin = -(3.0 + 3.0 * torch.rand(d, generator=gen))
        spec["drift"] = (spec["drift"][0], torch.cat([kap[:s], lin[s:]]))
        spec["term"] = (spec["term"][0], 0.2 + 0.5 * torch.rand(d, generator=gen))
        spec["split"] = s
        pb.native_spec = lambda: spec                          # (b / g are not called on the native plan)
        pb.X_0 = (-1.0 + 0.3 * torch.cos(torch.arange(d, dtype=torch.float32))).to(device)
    return pb


def nets(c, device):
    out = [psp.DenseNet(d_in=c["d"], d_out=c["d"], lr=0.0, arch=[c["H"], c["H"]], seed=5 + n).to(device) for n in range(c["N"])]
    dc.prepare_nets(c, out)
    return out


_REFS = {}


def reference(c, noise, jacobian=True, stream="host"):
    """ref64_wells.iteration of the case, once per (problem, shape, flags, noise) -- the matrix mode does not enter."""
    key = (c["cls"], c["d"], c["H"], c["K"], c["N"], c["flag"], c["split"], c["noise"], jacobian,
           stream if c["noise"] == "philox" else "")
    if key not in _REFS:
        pb = problem(c, "cpu")
        _REFS[key] = ref64_wells.iteration(pb.native_spec(), pb.X_0, c["N"], DT, nets(c, "cpu"), noise(), loss=c["loss"],
                                           adaptive=c["adaptive"], detach=c["detach"], jacobian=jacobian)
    return _REFS[key]
