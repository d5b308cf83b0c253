"""Shared by the EigenvalueSolver tests: the goldens of tests/golden/make_golden_eigenvalue.py and the package objects of a case."""
import torch

from conftest import load_golden
from util_cases import psp

GOLDENS = ["eig_fp_d5", "eig_fp_d10", "eig_nls5_d5", "eig_nls5_d10", "eig_nls10_d5", "eig_nls10_d10",
           "eig_fp_d2_exits", "eig_nls10_d2_exits"]
LOSS_LOGS = ("loss_log", "loss_log_center", "loss_log_boundary", "loss_log_derivative_boundary", "loss_log_domain")


def notebook_net(kind, d, device="cpu", arch=None):
    """The three notebooks' nets from the package's classes (seed 42, lr 0.001, as the notebooks build them)."""
    if kind == "fp":        # relu^2, weights randn * 0.1, biases 0.8
        return psp.DenseNet(d, 1, lr=0.001, arch=arch or [10] * 4, output_relu=True, bias_init=0.8).to(device)
    if kind == "nls10":     # relu^2, weights randn * 0.01 + 0.01, biases 0.1
        return psp.DenseNet(d, 1, lr=0.001, arch=arch or [15] * 4, output_relu=True, weight_scale=0.01, weight_shift=0.01,
                            bias_init=0.1).to(device)
    assert kind == "nls5"   # tanh, nn.Linear layers
    return psp.DenseNet_tanh(d, 1, lr=0.001, arch=arch or [15] * 4, output_relu=True).to(device)


def kind_of(name):
    return name.split("_")[1]


def build(name, device="cpu", backend="auto", **over):
    """(record, problem, solver) of a golden: nothing but the problem, the notebook's settings and its net."""
    rec = load_golden(name)
    case, exp = rec["case"], rec["expected"]
    kind = kind_of(name)
    fp = kind == "fp"
    prob = (psp.FokkerPlanckEigenvalue if fp else psp.SchroedingerEigenvalue)(d=case["d"], device=device)
    kw = dict(seed=case["seed"], delta_t=exp["settings"]["delta_t"] if case["delta_t"] is None else case["delta_t"],
              N=case["N"], L=case["L"], K=case["K"], K_boundary=case["K_boundary"], alpha=exp["settings"]["alpha"],
              lambda_init=exp["lambda_init"], lambda_lr=exp["settings"]["lambda_lr"], normalisation="center" if fp else "l2",
              verbose=False, device=device, backend=backend)
    kw.update(over)
    model = psp.EigenvalueSolver(prob, name, **kw)
    model.V = notebook_net(kind, case["d"], device)
    net = exp["net"]
    assert list(model.V.nn_dims) == net["dims"] and bool(model.V.output_relu) == net["output_relu"]
    return rec, prob, model


def fingerprint(module):
    out = []
    for name, p in module.named_parameters():
        q = p.detach().to(torch.float64).cpu()
        out.append({"shape": list(p.shape), "sum": float(q.sum()), "abs_sum": float(q.abs().sum())})
    return out
