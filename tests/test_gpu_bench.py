"""bench.py as the driver runs it: a plain run prints the headline line and nothing of the --full legs, and
--dump-outputs writes what the last timed step computed, the same for the same arguments."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*words):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(words),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_render_line_and_outputs(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    res = run_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(a))
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["dtype"] == "f16"
    assert abs(res["value"] - 800 * 800 * 128 / (res["ms_per_step"] * 1e-3)) <= 1e-6 * res["value"]
    assert "cpu_baseline" not in res and "aux" not in res and set(res["by_dtype"]) == {"f16"}
    assert res["roofline"]["traffic_source"] != "live"
    rgb, disp = np.load(a / "rgb.npy"), np.load(a / "disp.npy")
    assert rgb.shape == (640_000, 3) and disp.shape == (640_000,) and rgb.dtype == disp.dtype == np.float32
    assert np.isfinite(rgb).all() and rgb.min() >= 0 and rgb.max() <= 1 and np.isfinite(disp).all() and rgb.std() > 0
    # the same arguments but another number of steps: every step renders the same seeded image
    run_bench("--steps", "2", "--warmup", "0", "--dump-outputs", str(b))
    assert np.abs(np.load(b / "rgb.npy") - rgb).max() <= 1e-6 and np.abs(np.load(b / "disp.npy") - disp).max() <= 1e-6


def test_plain_train_line_and_outputs(tmp_path, synthetic):
    res = run_bench("--mode", "train", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["by_storage"] is None and res["roofline"] is None
    loss = np.load(tmp_path / "loss.npy")
    assert loss.dtype == np.float32 and np.isfinite(loss) and float(loss) == pytest.approx(res["final_loss"], rel=1e-6)
    init = synthetic.synthetic_state_dict(0, "default")
    files = sorted(glob.glob(str(tmp_path / "param.*.npy")))
    assert len(files) == len(init) == 24
    moved = 0
    for f in files:
        k = os.path.basename(f)[len("param."):-len(".npy")]
        p = np.load(f)
        assert p.dtype == np.float32 and p.shape == tuple(init[k].shape) and np.isfinite(p).all()
        moved += int(not np.array_equal(p, init[k].float().numpy()))
    assert moved == len(files)                       # four Adam steps moved every tensor
