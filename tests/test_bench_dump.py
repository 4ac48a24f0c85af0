"""bench.py --dump-outputs on the host (no GPU): file per output, dtypes, complex as (re, im), the 64 MB bound and the seeded
sample that lets two builds be compared output for output."""
import os

import numpy as np
import torch

import bench


def test_dump_bound_is_64_mb():
    assert bench.DUMP_BYTES <= 64_000_000


def test_small_outputs_are_written_whole(tmp_path):
    c = (np.arange(12) - 1j * np.arange(12)).astype(np.complex64).reshape(3, 4)
    d = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    info = bench.dump_outputs(str(tmp_path), {"d": d, "c": torch.from_numpy(c)})
    assert sorted(os.listdir(tmp_path)) == ["c.npy", "d.npy"]
    got_d, got_c = np.load(tmp_path / "d.npy"), np.load(tmp_path / "c.npy")
    assert got_d.dtype == np.float64 and np.array_equal(got_d, d.numpy())
    assert got_c.dtype == np.float32 and got_c.shape == (3, 4, 2)
    assert np.array_equal(got_c[..., 0], c.real) and np.array_equal(got_c[..., 1], c.imag)
    assert info["d"] == {"shape": [2, 3], "dtype": "float64", "entries_written": 6, "selection": None, "sample": None}
    assert info["c"]["shape"] == [3, 4, 2] and info["c"]["sample"] is None


def test_large_outputs_are_a_fixed_sample_under_the_bound(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 400_000)
    rng = np.random.default_rng(0)
    big = {"p": rng.standard_normal((50, 1000)).astype(np.float32), "q": rng.standard_normal((50, 1000))}   # 600 kB in all
    info = bench.dump_outputs(str(tmp_path / "one"), big)
    bench.dump_outputs(str(tmp_path / "two"), big)
    for run in ("one", "two"):
        assert sum(os.path.getsize(tmp_path / run / f) for f in os.listdir(tmp_path / run)) <= 400_000
    for name, a in big.items():
        got = np.load(tmp_path / "one" / (name + ".npy"))
        assert np.array_equal(got, np.load(tmp_path / "two" / (name + ".npy")))
        assert got.dtype == a.dtype and got.ndim == 1 and 0 < got.size < a.size
        assert info[name]["entries_written"] == got.size and info[name]["shape"] == list(a.shape)
        assert np.array_equal(got, a.reshape(-1)[bench.dump_positions(a.size, got.size)])
    assert info["p"]["entries_written"] == info["q"]["entries_written"]        # the same share of every output


def test_off_diagonal_keeps_the_pairs_i_ne_j():
    """A coherence-like [bins, C, C] result, NaN on the diagonal as the measure defines it: the dump's selection is the finite
    pairs i != j, row-major."""
    t = torch.arange(2 * 3 * 3, dtype=torch.float32).reshape(2, 3, 3)
    t[:, [0, 1, 2], [0, 1, 2]] = float("nan")
    got = bench.off_diagonal(t)
    assert got.shape == (2, 6) and torch.isfinite(got).all()
    want = [[1, 2, 3, 5, 6, 7], [10, 11, 12, 14, 15, 16]]
    assert got.tolist() == want
    c = torch.complex(t, -t)
    assert bench.off_diagonal(c).shape == (2, 6) and torch.equal(bench.off_diagonal(c).real, got)
