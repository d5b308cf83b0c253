"""bench.py --dump-outputs: the plan buffers and the per-step arrays land as float32 / float64 .npy files, and the total stays
under the byte limit (a larger array becomes a fixed, seeded sample with its index)."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _plan(K=1000, P=300):
    g = torch.Generator().manual_seed(0)
    return types.SimpleNamespace(flat=torch.randn(P, generator=g), grad=torch.randn(P, generator=g),
                                 m=torch.randn(P, generator=g), v=torch.rand(P, generator=g),
                                 D=torch.randn(K, generator=g), sums=torch.randn(2, generator=g, dtype=torch.float64),
                                 y0_param=torch.zeros(1), learn_y0=False)


def test_dump_writes_the_plan_buffers_and_the_losses(tmp_path):
    plan = _plan()
    loss = torch.arange(5, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path), plan, {"loss": loss})
    names = sorted(f[:-4] for f in os.listdir(tmp_path))
    assert names == ["adam_m", "adam_v", "grad", "loss", "loss_sums", "params", "terminal_D"]   # y0 only when learned
    assert np.load(tmp_path / "loss_sums.npy").dtype == np.float64
    for name, t in (("params", plan.flat), ("grad", plan.grad), ("terminal_D", plan.D), ("loss", loss)):
        a = np.load(tmp_path / (name + ".npy"))
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, t.numpy())


def test_dump_samples_what_exceeds_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 12000)
    plan = _plan(K=100000, P=300)
    bench.dump_outputs(str(tmp_path / "a"), plan, {})
    bench.dump_outputs(str(tmp_path / "b"), plan, {})
    total = sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a"))   # (128-byte .npy headers)
    assert total <= 12000
    idx = np.load(tmp_path / "a" / "terminal_D_sample_index.npy")
    D = np.load(tmp_path / "a" / "terminal_D.npy")
    assert idx.dtype == np.float64 and 0 < D.size == idx.size < 100000
    np.testing.assert_array_equal(D, plan.D.numpy()[idx.astype(np.int64)])
    np.testing.assert_array_equal(idx, np.load(tmp_path / "b" / "terminal_D_sample_index.npy"))   # the same sample every run
