"""bench.py --dump-outputs: what the last timed step computed goes to DIR/<name>.npy in float32, at most DUMP_LIMIT bytes in all;
arrays too large for their share are replaced by a fixed seeded sample, so that two runs (two builds) compare element for element."""
import os
import sys

import numpy as np

import bench


def files(d):
    return sorted(os.listdir(d))


def total_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole(tmp_path):
    mask = np.arange(24 * 32 * 4, dtype=np.uint32).reshape(24, 32, 4).astype(np.uint8)
    lo = np.random.default_rng(1).standard_normal((21, 3, 4)).astype(np.float32)
    bench.dump_outputs(str(tmp_path), {"mask_f0": mask, "out_low_f0": lo})
    assert files(tmp_path) == ["mask_f0.npy", "out_low_f0.npy"]
    m = np.load(tmp_path / "mask_f0.npy")
    assert m.dtype == np.float32 and m.shape == mask.shape and (m == mask).all()
    assert (np.load(tmp_path / "out_low_f0.npy") == lo).all()


def test_large_outputs_are_sampled_under_the_limit_and_reproducibly(tmp_path):
    limit = 1 << 20
    rng = np.random.default_rng(2)
    arrays = {"mask_f0": rng.integers(0, 256, (512, 512, 4), dtype=np.uint8),  # 4 MB as float32: sampled
              "out_low_f0": rng.standard_normal((21, 8, 8)).astype(np.float32)}  # small: whole
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), arrays, limit=limit)
    bench.dump_outputs(str(b), arrays, limit=limit)
    assert files(a) == ["mask_f0.npy", "mask_f0_index.npy", "out_low_f0.npy"]
    assert total_bytes(a) <= limit
    idx = np.load(a / "mask_f0_index.npy")
    val = np.load(a / "mask_f0.npy")
    assert idx.dtype == np.float64 and val.dtype == np.float32 and idx.shape == val.shape and idx.size > 10000
    assert (np.diff(idx) > 0).all()  # sorted, no repeats
    assert (val == arrays["mask_f0"].reshape(-1)[idx.astype(np.int64)]).all()
    for f in files(a):  # the same positions on every run
        assert (np.load(a / f) == np.load(b / f)).all(), f
    assert (np.load(a / "out_low_f0.npy") == arrays["out_low_f0"]).all()


def test_default_limit_holds_for_the_default_workload(tmp_path):
    """8 masks of 1920x1080 RGBA + out / aux logits of three contexts' last frames (265 MB as float32) stay under 64 MB."""
    arrays = {f"mask_f{i}": np.zeros((1080, 1920, 4), np.uint8) for i in range(8)}
    for i in (5, 6, 7):
        arrays[f"out_low_f{i}"] = np.zeros((21, 135, 240), np.float32)
        arrays[f"aux_low_f{i}"] = np.zeros((21, 135, 240), np.float32)
    bench.dump_outputs(str(tmp_path), arrays)
    assert total_bytes(tmp_path) <= bench.DUMP_LIMIT == 64 << 20


def test_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 3 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"
