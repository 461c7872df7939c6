"""A plain `bench.py` run with --dump-outputs: --steps sets the timed steps, the line carries ms_per_step and none of --full's side
objects, and the dumped arrays are what the timed path computed -- logits within 1e-3 relative of the CPU oracle for the frame each
context ran last, and that frame's mask bit-exact given those logits (the check of smoke())."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from infur_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path, oracle_model):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--frames-per-step", "3", "--contexts-per-gpu", "2", "--width", "160", "--height", "120",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0 and j["dtype"] == "f32"
    assert abs(j["value"] - 3 * 1e3 / j["ms_per_step"]) / j["value"] < 1e-3  # frames/s = frames per step / step time
    assert "cpu_baseline" not in j and "side_rates" not in j["config"]
    names = sorted(os.listdir(out))
    assert [n for n in names if n.startswith("mask_")] == ["mask_f0.npy", "mask_f1.npy", "mask_f2.npy"]
    lows = [n for n in names if n.startswith("out_low_")]
    assert len(lows) == 2 and all(f"aux_{n[4:]}" in names for n in lows)  # one per context, aux head on
    for n in lows:
        i = int(n[len("out_low_f"):-len(".npy")])
        fr = W.synth_frame(120, 160, index=i)
        ref = oracle_model.model_forward(oracle_model.pack_normalize(fr), full=False)
        lo = np.load(out / n)
        la = np.load(out / f"aux_low_f{i}.npy")
        for got, want in ((lo, ref["out_low"]), (la, ref["aux_low"])):
            assert got.dtype == np.float32 and got.shape == want.shape
            assert np.abs(got - want).max() / np.abs(want).max() < 1e-3
        mask = np.load(out / f"mask_f{i}.npy")
        assert mask.dtype == np.float32 and mask.shape == (120, 160, 4)
        assert (mask == oracle_model.colorcode(oracle_model.upsample_bilinear(lo, 120, 160))).all()
