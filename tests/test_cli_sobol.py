"""rwr_render --sobol (RWR_FLAG_SOBOL): the option sets the flag and implies nothing else; the frame it writes is the library's frame
with the flag.  (--show-params prints what the arguments give, without a device.)"""
import os
import subprocess

import numpy as np
import pytest


def _run(rwr, *args):
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")
    return subprocess.run([exe, *args], capture_output=True, text=True)


def test_cli_sobol_arguments(rwr):
    r = _run(rwr, "--help")
    assert r.returncode == 0 and "--sobol" in r.stdout and "RWR_FLAG_SOBOL" in r.stdout
    r = _run(rwr, "--sobol", "--show-params")                       # it implies nothing
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_SOBOL:x} " in r.stdout
    r = _run(rwr, "--bounces", "2", "--spp", "4", "--sobol", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_SOBOL:x} " in r.stdout and "spp 4 bounces 2 " in r.stdout
    r = _run(rwr, "--bounces", "1", "--spp", "4", "--show-params")  # and nothing implies it
    assert r.returncode == 0 and "flags 0x0 " in r.stdout


@pytest.mark.gpu
def test_cli_sobol_writes_the_librarys_frame(rwr, tmp_path):
    """The reference's scene from the default camera, 96 x 64, 4 spp and a bounce: the PNG rwr_render --sobol writes holds the RGBA8
    frame the library renders with RWR_FLAG_SOBOL (written by the library's own PNG writer, read back by its own decoder), and it is
    not the frame without the option."""
    w, h = 96, 64
    common = ["--res", rwr.RES_DIR, "--size", f"{w}x{h}", "--spp", "4", "--bounces", "1"]

    def run(out, *args):
        path = str(tmp_path / out)
        r = _run(rwr, *common, *args, "--out", path)
        assert r.returncode == 0, (r.stdout, r.stderr)
        return rwr.decode_image_rgba8(open(path, "rb").read())

    plain, sob = run("plain.png"), run("sobol.png", "--sobol")
    assert sob.shape == (h, w, 4) and not np.array_equal(sob, plain)
    model = rwr.load_model_compute("suzanne_lowpoly.obj")
    cam = rwr.circle_controller_update(rwr.make_camera(aspect=w / h), 0)      # the program's one frame: update() with no key held, then render()
    cam_inv = rwr.camera_build_inv_uniform(cam)
    with rwr.Context(0) as c:
        c.upload_model(model)
        c.set_spheres(rwr.make_spheres())
        c.resize(w, h)
        for flags, want, name in ((rwr.FLAG_SOBOL, sob, "lib_sobol.png"), (0, plain, "lib_plain.png")):
            c.render(cam_inv, rwr.make_params(spp=4, max_bounces=1, seed=0, flags=flags))
            path = str(tmp_path / name)
            rwr.write_png(path, c.readback()["color"], flip_vertical=True, encode_srgb=True)     # as the program writes its frame
            assert np.array_equal(rwr.decode_image_rgba8(open(path, "rb").read()), want), name
