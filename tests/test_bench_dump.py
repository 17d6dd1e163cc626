"""bench.py --dump-outputs without a GPU: the files it writes for a frame (float32, the values exact), the fixed seeded
sample of pixels that keeps a large frame under 64 MB, and the argument checks that run before any GPU work."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _frame(h, w, seed):
    rng = np.random.default_rng(seed)
    return {"color": rng.integers(0, 256, (h, w, 4), dtype=np.uint8), "depth": rng.random((h, w), dtype=np.float32)}


def test_small_frame_is_written_whole(tmp_path):
    bench = _bench_module()
    frame = _frame(54, 96, 1)
    bench.dump_outputs(str(tmp_path / "out"), frame)
    assert sorted(os.listdir(tmp_path / "out")) == ["color.npy", "depth.npy"]
    for name, a in frame.items():
        got = np.load(tmp_path / "out" / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == a.shape and np.array_equal(got, a.astype(np.float32))


def test_large_frame_is_a_fixed_sample_under_64mb(tmp_path):
    bench = _bench_module()
    h, w = 2160, 3840                                   # configs[3] / configs[4]
    frame = _frame(h, w, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), frame)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["color.npy", "depth.npy", "pixel_index.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10**6
    idx = np.load(tmp_path / "a" / "pixel_index.npy")
    assert idx.dtype == np.float64 and len(idx) == bench.DUMP_MAX_PIXELS and (np.diff(idx) > 0).all()
    assert idx[0] >= 0 and idx[-1] < h * w
    ii = idx.astype(np.int64)
    color, depth = np.load(tmp_path / "a" / "color.npy"), np.load(tmp_path / "a" / "depth.npy")
    assert color.dtype == np.float32 and color.shape == (len(ii), 4)
    assert np.array_equal(color, frame["color"].reshape(-1, 4)[ii].astype(np.float32))
    assert np.array_equal(depth, frame["depth"].reshape(-1)[ii])
    for f in files:                                     # the same pixels in every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--warmup", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr and r.stdout.strip() == ""
