"""CPU: bench.py --dump-outputs writes finite float32 / float64 arrays (a non-finite entry as bench.DUMP_NONFINITE, its
kind in <name>.nonfinite.npy), whole when small and a seeded row sample of the large ones that depends only on the
name and the shape (two runs give the same files), within the budget.  A host-array stand-in replaces the device
arrays (same offset / to_host surface); the budget is scaled down so that small arrays take the sampling path."""
import glob
import os

import numpy as np

import bench


class HostArray:
    def __init__(self, a, flat=None, start=0):
        self.a, self.flat, self.start = a, a.ravel() if flat is None else flat, start
        self.shape, self.dtype = a.shape, a.dtype

    def to_host(self):
        return self.a.copy()

    def offset(self, n, shape):
        m = int(np.prod(shape))
        return HostArray(self.flat[self.start + n: self.start + n + m].reshape(shape), self.flat, self.start + n)


def _outputs(rng, n=4000, s=50):
    ps = rng.random((n, s), dtype=np.float32)
    ps[rng.integers(0, n, 500), rng.integers(0, s, 500)] = np.nan          # PS of 0 / 0
    ps[rng.integers(0, n, 20), rng.integers(0, s, 20)] = np.inf
    ps[rng.integers(0, n, 20), rng.integers(0, s, 20)] = -np.inf
    return [("row_of", HostArray(rng.permutation(n).astype(np.int32))),
            ("tested", HostArray(rng.integers(0, 2, 300).astype(np.uint8))),
            ("ps", HostArray(ps))]


def test_dump_outputs_sample_is_reproducible_finite_and_bounded(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 256 << 10)
    outs = _outputs(np.random.default_rng(5))
    n, ps = outs[0][1].shape[0], outs[2][1].a
    a, b = bench.dump_outputs(str(tmp_path / "a"), outs), bench.dump_outputs(str(tmp_path / "b"), outs)
    assert a == b and a["tested"] == 300 and a["row_of"] == n and 0 < a["ps"] < n     # small ones whole
    assert not os.path.exists(tmp_path / "a" / "row_of.rows.npy")
    total = 0
    for f in sorted(glob.glob(str(tmp_path / "a" / "*.npy"))):
        x, y = np.load(f), np.load(f.replace(os.sep + "a" + os.sep, os.sep + "b" + os.sep))
        assert x.dtype in (np.float32, np.float64) and np.all(np.isfinite(x)) and np.array_equal(x, y)
        total += os.path.getsize(f)
    assert total <= bench.DUMP_BUDGET + 16 * 128                                      # (+ .npy headers)
    assert np.array_equal(np.load(tmp_path / "a" / "row_of.npy"), outs[0][1].a.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "tested.npy"), outs[1][1].a.astype(np.float64))
    assert not os.path.exists(tmp_path / "a" / "row_of.nonfinite.npy")              # (integer outputs have no codes)
    rows = np.load(tmp_path / "a" / "ps.rows.npy").astype(np.int64)
    assert rows.size == a["ps"] and np.all(np.diff(rows) > 0)
    got, code, want = np.load(tmp_path / "a" / "ps.npy"), np.load(tmp_path / "a" / "ps.nonfinite.npy"), ps[rows]
    assert got.dtype == np.float32 and code.shape == got.shape
    assert np.array_equal(code != 0, ~np.isfinite(want)) and np.all(got[code != 0] == np.float32(bench.DUMP_NONFINITE))
    back = got.copy()
    back[code == 1], back[code == 2], back[code == 3] = np.nan, np.inf, -np.inf
    assert np.array_equal(back, want, equal_nan=True)


def test_dump_outputs_a_nan_turned_into_zero_changes_the_values_file(tmp_path):
    ps = np.random.default_rng(6).random((50, 8), dtype=np.float32)
    ps[3, 4] = np.nan
    wrong = ps.copy()
    wrong[3, 4] = 0
    bench.dump_outputs(str(tmp_path / "right"), [("ps", HostArray(ps))])
    bench.dump_outputs(str(tmp_path / "wrong"), [("ps", HostArray(wrong))])
    right_v, wrong_v = np.load(tmp_path / "right" / "ps.npy"), np.load(tmp_path / "wrong" / "ps.npy")
    assert not np.allclose(right_v, wrong_v)
    assert os.path.exists(tmp_path / "wrong" / "ps.nonfinite.npy")                  # written even with no NaN
