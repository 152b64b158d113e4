"""bench.py --dump-outputs, host side (no GPU): the files written, their dtype, and the 64 MB cap on all of them together."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_outputs_are_written_whole_in_float32(tmp_path):
    a = np.random.default_rng(1).standard_normal((2, 300, 64)).astype(np.float16)
    bench.dump_outputs(str(tmp_path / "d"), {"final_latents": a})
    got = np.load(tmp_path / "d" / "final_latents.npy")
    assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32))


def test_large_outputs_keep_a_fixed_sample_of_rows_under_the_cap(tmp_path):
    limit = 1 << 20
    a = np.arange(4 * 3000 * 64, dtype=np.float32).reshape(4, 3000, 64)           # 3 MB against a 1 MB cap
    b = np.arange(1 * 500 * 64, dtype=np.float32).reshape(1, 500, 64)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b}, limit=limit)
    sizes = [os.path.getsize(tmp_path / "x" / f) - 128 for f in ("a.npy", "b.npy")]    # 128-byte .npy header
    assert sum(sizes) <= limit
    ga, gb = np.load(tmp_path / "x" / "a.npy"), np.load(tmp_path / "x" / "b.npy")
    assert ga.shape[0] == 4 and ga.shape[2] == 64 and 0 < ga.shape[1] < 3000
    rows = ga[0, :, 0].astype(np.int64) // 64                                           # every kept row is a whole row of `a`, in order
    assert np.array_equal(ga, a[:, rows]) and bool((rows[1:] > rows[:-1]).all())
    assert np.array_equal(gb, b[:, gb[0, :, 0].astype(np.int64) // 64])
    assert np.array_equal(ga, np.load(tmp_path / "y" / "a.npy"))                        # the same sample every run
