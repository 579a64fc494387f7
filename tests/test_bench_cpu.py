"""bench.py's options and its output dump, without a GPU: a plain run is lean by default (the secondary measurements and the CPU
baseline only with --full), --steps is the number of timed steps, and --dump-outputs stays within its budget and writes the
same values for the same input."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_is_lean_by_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_steps_must_be_positive():
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_small_arrays_whole(tmp_path):
    img = np.random.default_rng(1).random((200, 320, 4), dtype=np.float32)
    img8 = (img * 255).astype(np.uint8)
    bench.dump_outputs(str(tmp_path), [("image", img), ("image_u8", img8)])
    assert sorted(os.listdir(tmp_path)) == ["image.npy", "image_u8.npy"]
    a, b = np.load(tmp_path / "image.npy"), np.load(tmp_path / "image_u8.npy")
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(a, img) and np.array_equal(b, img8.astype(np.float32))


def test_dump_outputs_of_the_metric_frame_fit_the_budget_and_repeat(tmp_path):
    """1920x1080 RGBA f32 + u8 as f32 exceed 64 MB together: the f32 image is written whole, the u8 image as a fixed sample of
    pixels, identical on every run."""
    rng = np.random.default_rng(2)
    img = rng.random((1080, 1920, 4), dtype=np.float32)
    img8 = rng.integers(0, 256, (1080, 1920, 4), dtype=np.uint8)
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        bench.dump_outputs(str(d), [("image", img), ("image_u8", img8)])
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= bench.DUMP_BUDGET
    a = np.load(dirs[0] / "image.npy")
    s = np.load(dirs[0] / "image_u8.npy")
    assert np.array_equal(a, img)
    assert s.ndim == 2 and s.shape[1] == 4 and 1_000_000 < s.shape[0] < 1080 * 1920
    rows = img8.reshape(-1, 4).astype(np.float32)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(rows.shape[0], size=s.shape[0], replace=False))
    assert np.array_equal(s, rows[idx])
    for f in ("image.npy", "image_u8.npy"):
        assert open(dirs[0] / f, "rb").read() == open(dirs[1] / f, "rb").read()
