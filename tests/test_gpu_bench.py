"""bench.py end to end on the GPU box (short runs): the contract line of the default configuration and of the redraw loop
(controller update + inverse uniform + render per frame), with the self-check fields of the roofline block."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--cpu-seconds", "0", *args], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_default_line_has_the_contract_fields():
    d = _bench("--steps", "200", "--warmup", "50")
    assert d["metric"] == "Mray/s" and d["n_gpus"] == 1 and d["steps"] == 200 and d["value"] > 0 and d["dtype"] == "f32"
    assert abs(d["value"] - 1920 * 1080 / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 1e-3
    r = d["roofline"]
    assert r["bound"] in ("valu", "hbm") and 0.0 < r["frac"] < 1.5 and r["timed_region_instrumented"] is False
    assert r["csrc_tree"] and "counters_stale" in r and r["hbm"]["algorithmic_bytes_per_step"] == 8 * 1920 * 1080
    if r["valu"]:
        assert r["valu"]["spec_mhz"] == 2400.0 and r["frac"] == r["valu"]["frac_at_2400mhz"]


def test_redraw_loop_line():
    d = _bench("--config", "loop", "--steps", "200", "--warmup", "50")
    lp = d["loop"]
    assert lp["keys"] == "SWDA" and max(abs(v) for v in lp["eye_after"]) <= 0.25   # the scripted keys wobble about the reference pose
    assert 0.0 < lp["host_us_per_frame_update_and_uniform"] < 50.0 and lp["host_us_per_frame_enqueue_total"] > 0.0
    assert d["roofline"]["counters_stale"] in (True, None)                       # counters are the fixed camera's: said so
    assert d["value"] > 0 and d["config"]["frames_in_flight"] == 2


def test_plain_line_and_dumped_frame(rwr, orc, suzanne, tmp_path):
    """A plain run (no --full): the contract fields and nothing measured outside the timed steps; --dump-outputs writes the
    last timed frame, which is the reference frame of configs[1] (depth bit-exact against the oracle, RGBA8 within 1 LSB)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["metric"] == "Mray/s" and d["unit"] == "Mray/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 30 and d["warmup"] == 5 and d["ms_per_step"] > 0
    assert abs(d["value"] - 1920 * 1080 / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 1e-3
    assert "roofline" not in d and "cpu_baseline" not in d and "ms_per_frame_one_in_flight" not in d
    assert sorted(os.listdir(tmp_path)) == ["color.npy", "depth.npy"]
    color, depth = np.load(tmp_path / "color.npy"), np.load(tmp_path / "depth.npy")
    assert color.dtype == np.float32 and color.shape == (1080, 1920, 4) and depth.dtype == np.float32 and depth.shape == (1080, 1920)
    w, h = 1920, 1080
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(aspect=w / h, eye=(0, 0, 0), target=(0, 0, -1)))
    want = orc.render_frame(cam_inv.view(orc.CAMERA_INV_DTYPE), orc.make_screen(w, h), orc.make_spheres(), suzanne)
    assert np.array_equal(depth.view(np.uint32), want["depth"].view(np.uint32))
    d8 = np.abs(color - want["color"].astype(np.float32))
    assert d8.max() <= 1 and (d8 != 0).mean() < 1e-3
