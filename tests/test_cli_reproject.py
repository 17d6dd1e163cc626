"""rwr_render --reproject [--reproject-history N] [--reproject-normal C] [--reproject-depth X]: what the arguments give
(--show-params, without a device), bad values, and - on the GPU - the key script whose every step feeds the next frame's history."""
import os
import subprocess

import pytest


def _exe(rwr):
    return os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")


def _run(rwr, *args):
    return subprocess.run([_exe(rwr), *args], capture_output=True, text=True)


def test_show_params_lists_the_parameters(rwr):
    r = _run(rwr, "--help")
    assert r.returncode == 0 and all(o in r.stdout for o in ("--reproject", "--reproject-history", "--reproject-normal", "--reproject-depth"))
    r = _run(rwr, "--spp", "2", "--show-params")
    assert r.returncode == 0 and "reproject" not in r.stdout and "flags 0x0 " in r.stdout
    r = _run(rwr, "--reproject", "--show-params")
    assert r.returncode == 0 and "reproject 1 history 32 normal 0.95 depth 0.05\n" in r.stdout and f"flags 0x{rwr.FLAG_REPROJECT:x} " in r.stdout
    # a value implies the flag
    r = _run(rwr, "--reproject-history", "8", "--show-params")
    assert r.returncode == 0 and "reproject 1 history 8 normal 0.95 depth 0.05\n" in r.stdout and f"flags 0x{rwr.FLAG_REPROJECT:x} " in r.stdout
    r = _run(rwr, "--bounces", "2", "--reproject-normal", "-0.5", "--reproject-depth", "0.25", "--reproject-history", "1024", "--show-params")
    assert r.returncode == 0 and "reproject 1 history 1024 normal -0.5 depth 0.25\n" in r.stdout
    assert f"flags 0x{rwr.FLAG_REPROJECT | rwr.FLAG_MULTI_BOUNCE:x} " in r.stdout


@pytest.mark.parametrize("opt,bad", [("--reproject-history", "0"), ("--reproject-history", "1025"), ("--reproject-history", "3.5"), ("--reproject-history", "many"),
                                     ("--reproject-normal", "1.5"), ("--reproject-normal", "-2"), ("--reproject-normal", "nan"),
                                     ("--reproject-depth", "-0.1"), ("--reproject-depth", "inf"), ("--reproject-depth", "nan"), ("--reproject-depth", "0.1x")])
def test_bad_values_exit_with_status_2(rwr, opt, bad):
    r = _run(rwr, opt, bad, "--show-params")
    assert r.returncode == 2 and opt in r.stderr, (opt, bad, r.stderr)
    assert _run(rwr, opt).returncode == 2   # a missing value


@pytest.mark.gpu
def test_every_key_step_feeds_the_history(rwr, suzanne, tmp_path):
    """--keys "S*4,D*4" and the one frame after the script: nine frames, `history 9`, and the PNG is the library's ninth frame."""
    w, h = 96, 64
    common = ["--res", rwr.RES_DIR, "--size", f"{w}x{h}", "--keys", "S*4,D*4", "--spp", "2", "--bounces", "1"]
    outs = {k: str(tmp_path / f"{k}.png") for k in ("plain", "reproject", "short")}
    r = _run(rwr, *common, "--out", outs["plain"])
    assert r.returncode == 0 and "history" not in r.stdout, r.stderr
    r = _run(rwr, *common, "--reproject", "--out", outs["reproject"])
    assert r.returncode == 0 and "\nhistory 9\n" in r.stdout, (r.stdout, r.stderr)
    r = _run(rwr, *common, "--reproject-history", "3", "--out", outs["short"])
    assert r.returncode == 0 and "\nhistory 9\n" in r.stdout, (r.stdout, r.stderr)

    def driver_png(name, **params):
        with rwr.Context(0) as ctx:
            ctx.upload_model(suzanne); ctx.set_spheres(rwr.make_spheres()); ctx.resize(w, h)
            if params:
                ctx.set_reproject_params(**params)
            cam = rwr.make_camera(aspect=w / h)
            for keys in [rwr.KEY_BACKWARD] * 4 + [rwr.KEY_RIGHT] * 4 + [0]:
                cam = rwr.circle_controller_update(cam, keys)
                ctx.render(rwr.camera_build_inv_uniform(cam), rwr.make_params(spp=2, max_bounces=1, seed=0, flags=rwr.FLAG_REPROJECT))
            assert ctx.reproject_frames() == 9
            path = str(tmp_path / name)
            rwr.write_png(path, ctx.readback()["color"], flip_vertical=True, encode_srgb=True)
            return open(path, "rb").read()

    read = lambda k: open(outs[k], "rb").read()   # noqa: E731
    assert read("reproject") == driver_png("d0.png")
    assert read("short") == driver_png("d1.png", max_history=3)
    assert read("reproject") != read("plain") and read("short") != read("reproject")
