"""rwr_render --light-sky (RWR_FLAG_LIGHT_SKY): what the option gives (--show-params, no device), and on the GPU that it renders and
prints the counts under --sky-image and changes nothing without it."""
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _run(rwr, *args):
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")
    return subprocess.run([exe, *args], capture_output=True, text=True)


def _flat_hdr(px) -> bytes:
    """A Radiance picture of the (h, w, 4) RGBE pixels, not run-length encoded."""
    h, w = px.shape[:2]
    return b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode() + px.tobytes()


def test_cli_light_sky_arguments(rwr):
    r = _run(rwr, "--help")
    assert r.returncode == 0 and "--light-sky" in r.stdout and "RWR_FLAG_LIGHT_SKY" in r.stdout and "sky light rays N, reached M" in r.stdout
    # the option implies nothing: its bit alone; with --sky-image beside the bits that option gives
    r = _run(rwr, "--bounces", "2", "--spp", "4", "--light-sky", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_LIGHT_SKY:x} sky 0 " in r.stdout
    r = _run(rwr, "--bounces", "2", "--spp", "4", "--sky-image", "place.hdr", "--light-sky", "--light-mis", "--show-params")
    flags = rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_SKY | rwr.FLAG_SKY_IMAGE | rwr.FLAG_LIGHT_SKY | rwr.FLAG_LIGHT_MIS
    assert r.returncode == 0 and f"flags 0x{flags:x} sky 1 " in r.stdout
    r = _run(rwr, "--bounces", "2", "--spp", "4", "--show-params")            # without it: the line as it was
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE:x} sky 0 " in r.stdout


@pytest.mark.gpu
def test_cli_light_sky_renders_and_counts(rwr, tmp_path):
    """Under a .hdr picture with a bright patch the run prints `sky light rays N, reached M` with 0 < M <= N and the frame differs from
    the one without the option; without --sky-image the option changes nothing: the same PNG, and no ray is counted."""
    px = np.zeros((8, 16, 4), np.uint8)
    px[..., :3] = 128
    px[..., 3] = 124
    px[1:3, 10:12, 3] = 134                             # a small sun, 1 024 times the sky, high up
    (tmp_path / "sun.hdr").write_bytes(_flat_hdr(px))
    common = ["--res", rwr.RES_DIR, "--size", "96x64", "--spp", "4", "--bounces", "2"]

    def run(out, *args):
        path = str(tmp_path / out)
        r = _run(rwr, *common, *args, "--out", path)
        assert r.returncode == 0, (r.stdout, r.stderr)
        return r.stdout, rwr.decode_image_rgba8(open(path, "rb").read())

    image = ["--sky-image", str(tmp_path / "sun.hdr"), "--sky-image-size", "32"]
    text, lit = run("lit.png", *image, "--light-sky", "--light-mis")
    m = re.search(r"^sky light rays (\d+), reached (\d+)$", text, re.M)
    assert m and 0 < int(m.group(2)) <= int(m.group(1)), text
    text, plain = run("plain.png", *image)
    assert "sky light rays" not in text and not np.array_equal(lit, plain)
    text, a = run("a.png", "--sky", "--light-sky", "--light-mis")
    assert re.search(r"^sky light rays 0, reached 0$", text, re.M), text
    text, b = run("b.png", "--sky")
    assert np.array_equal(a, b)
