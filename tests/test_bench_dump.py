"""bench.py --dump-outputs: what the timed path computed, as float32 .npy files under a size cap (no GPU needed for the writer)."""
import importlib.util
import os
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _fake_learner(n_params, T, N, seed):
    g = torch.Generator().manual_seed(seed)
    net = lambda: types.SimpleNamespace(P=types.SimpleNamespace(flat=torch.randn(n_params, generator=g)))
    opt = lambda: types.SimpleNamespace(mu=torch.randn(n_params, generator=g), nu=torch.rand(n_params, generator=g))
    metrics = dict(episode_return=torch.randn(T, N, generator=g), episode_length=torch.randint(0, 100, (T, N), generator=g, dtype=torch.int32),
                   is_terminal_step=torch.randint(0, 2, (T, N), generator=g, dtype=torch.uint8))
    return types.SimpleNamespace(guider=net(), actor=net(), g_opt=opt(), a_opt=opt(), metrics=metrics)


def test_dump_writes_float32_arrays_with_a_fixed_sample_under_the_cap(tmp_path):
    b = _bench()
    T, N = 128, 16384                                   # the headline's metrics: 2 M elements each, over the per-array cap
    learner = _fake_learner(5000, T, N, seed=1)
    losses = torch.randn(4, 2, 9)
    info = b.dump_outputs(str(tmp_path / "a"), learner, losses)
    names = {"losses", "guider_params", "actor_params", "guider_adam_mu", "guider_adam_nu", "actor_adam_mu", "actor_adam_nu",
             "metrics_episode_return", "metrics_episode_length", "metrics_is_terminal_step"}
    assert set(info) == names and sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in names)
    total = 0
    for n in names:
        a = np.load(tmp_path / "a" / (n + ".npy"))
        assert a.dtype == np.float32
        total += a.nbytes
    assert total <= 64 << 20
    assert np.array_equal(np.load(tmp_path / "a" / "losses.npy"), losses.numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "guider_params.npy"), learner.guider.P.flat.numpy())
    ret = np.load(tmp_path / "a" / "metrics_episode_return.npy")
    assert info["metrics_episode_return"] == [[T, N], True] and ret.shape == (b.DUMP_MAX_ELEMS,)
    # the sample is the same set of elements every time: a second dump of the same arrays is identical file for file
    b.dump_outputs(str(tmp_path / "b"), learner, losses)
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))), n
    # and it is a sample of the array's own elements
    full = learner.metrics["episode_return"].numpy().reshape(-1)
    assert np.isin(ret, full).all()
