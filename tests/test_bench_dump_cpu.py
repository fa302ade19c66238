"""bench.dump_outputs (bench.py --dump-outputs DIR) on the host: what it writes for a model below
and above the sample size, and that two calls on the same state write the same bytes."""
import os

import numpy as np
import torch

import bench


def _model(seed):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.Conv2d(5, 7, 1, bias=False))
    for i, p in enumerate(m.parameters()):
        if i != 1:   # one parameter without a gradient: dumped as zeros
            p.grad = torch.randn_like(p)
    return m


def test_dump_outputs_writes_losses_parameters_and_gradients(tmp_path, monkeypatch):
    m = _model(3)
    flat_p = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()
    flat_g = torch.cat([(torch.zeros_like(p) if p.grad is None else p.grad).reshape(-1)
                        for p in m.parameters()]).numpy()
    n = flat_p.size
    d = str(tmp_path / "whole")
    bench.dump_outputs(d, {"loss_seg2": 1.5, "loss_D2": 0.25}, {"G": m, "D1": None, "D2": m})
    assert sorted(os.listdir(d)) == ["D2_grads.npy", "D2_params.npy", "G_grads.npy", "G_params.npy",
                                     "loss_D2.npy", "loss_seg2.npy"]
    for f in os.listdir(d):
        assert np.load(os.path.join(d, f)).dtype == np.float32, f
    assert np.load(os.path.join(d, "loss_seg2.npy")).tolist() == [1.5]
    assert np.array_equal(np.load(os.path.join(d, "G_params.npy")), flat_p)
    assert np.array_equal(np.load(os.path.join(d, "G_grads.npy")), flat_g)
    assert not np.load(os.path.join(d, "G_grads.npy"))[135:140].any()   # the bias without a gradient

    # past the sample size: the same seeded positions of both arrays, in order, on every call
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 50)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, {}, {"G": m})
    bench.dump_outputs(b, {}, {"G": m})
    idx = np.sort(np.random.default_rng(1338).choice(n, 50, replace=False))
    assert np.array_equal(np.load(os.path.join(a, "G_params.npy")), flat_p[idx])
    assert np.array_equal(np.load(os.path.join(a, "G_grads.npy")), flat_g[idx])
    for f in ("G_params.npy", "G_grads.npy"):
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read()
