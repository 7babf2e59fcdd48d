"""bench.py's host-side helpers (no GPU): how `--steps` / `--repeats` become timed regions, and what `--dump-outputs`
writes — within the byte budget, one seeded sample of rows / pixels shared by the arrays, the same from call to call."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_host_for_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("steps,repeats,expect", [(20, 5, [4] * 5), (7, 5, [2, 2, 1, 1, 1]), (3, 5, [1, 1, 1]),
                                                  (1, 5, [1]), (10, 1, [10]), (4, 0, [4])])
def test_timed_regions_run_exactly_the_asked_steps(bench, steps, repeats, expect):
    assert bench.timed_regions(steps, repeats) == expect


def _views(P, C, H, W, V, seed=0):
    g = torch.Generator().manual_seed(seed)
    views = []
    for _ in range(V):
        m2 = torch.zeros(P, 3, requires_grad=True)
        m2.grad = torch.randn(P, 3, generator=g)
        views.append((torch.randn(C, H, W, generator=g), torch.randn(1, H, W, generator=g), torch.rand(1, H, W, generator=g),
                      torch.randint(0, 40, (P,), generator=g, dtype=torch.int32), m2))
    params = []
    for shape in ((P, 3), (P, C), (P, 1), (P, 3), (P, 4)):
        p = torch.zeros(shape, requires_grad=True)
        p.grad = torch.randn(shape, generator=g)
        params.append(p)
    return views, params


def test_dump_outputs_samples_within_budget_and_repeats(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 2_000_000)
    P, C, H, W, V = 20_000, 6, 120, 160, 3
    views, params = _views(P, C, H, W, V)
    infos = [bench.dump_outputs(str(tmp_path / f"d{k}"), views, params, P, H * W) for k in range(2)]
    assert infos[0] == dict(infos[1], dir=infos[0]["dir"])
    info = infos[0]
    assert info["bytes"] <= 2_000_000
    assert sum(os.path.getsize(tmp_path / "d0" / f) for f in os.listdir(tmp_path / "d0")) == info["bytes"]
    ng, npx = info["gaussians"][0], info["pixels"][0]
    assert 0 < ng < P and 0 < npx < H * W          # both kinds sampled at this budget
    load = lambda d, n: np.load(tmp_path / d / f"{n}.npy")  # noqa: E731
    gi, pi = load("d0", "gaussian_index"), load("d0", "pixel_index")
    assert gi.dtype == np.float64 and gi.shape == (ng,) and (np.diff(gi) > 0).all() and gi.max() < P
    assert pi.dtype == np.float64 and pi.shape == (npx,) and (np.diff(pi) > 0).all() and pi.max() < H * W
    gi, pi = gi.astype(np.int64), pi.astype(np.int64)
    for k, (color, depth, alpha, radii, m2) in enumerate(views):
        assert np.array_equal(load("d0", f"view{k}_color"), color.reshape(C, -1).numpy()[:, pi])
        assert np.array_equal(load("d0", f"view{k}_depth"), depth.reshape(1, -1).numpy()[:, pi])
        assert np.array_equal(load("d0", f"view{k}_alpha"), alpha.reshape(1, -1).numpy()[:, pi])
        assert np.array_equal(load("d0", f"view{k}_radii"), radii.numpy()[gi].astype(np.float32))
        assert np.array_equal(load("d0", f"view{k}_grad_means2D"), m2.grad.numpy()[gi])
    for n, p in zip(("means3D", "colors", "opacities", "scales", "rotations"), params):
        a = load("d0", f"grad_{n}")
        assert a.dtype == np.float32 and np.array_equal(a, p.grad.numpy()[gi])
    for f in os.listdir(tmp_path / "d0"):
        assert np.array_equal(load("d0", f[:-4]), load("d1", f[:-4]))


def test_dump_outputs_writes_a_small_workload_whole(bench, tmp_path):
    P, C, H, W, V = 500, 3, 32, 48, 2
    views, params = _views(P, C, H, W, V, seed=1)
    info = bench.dump_outputs(str(tmp_path), views, params, P, H * W)
    assert info["gaussians"] == [P, P] and info["pixels"] == [H * W, H * W]
    assert np.array_equal(np.load(tmp_path / "view1_color.npy"), views[1][0].reshape(C, -1).numpy())
    assert np.array_equal(np.load(tmp_path / "grad_colors.npy"), params[1].grad.numpy())
