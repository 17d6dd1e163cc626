"""rwr_render --tonemap [clamp|reinhard|aces], --exposure STOPS, --auto-exposure [KEY], --white W (RWR_FLAG_TONEMAP): each implies
the flag; a run prints the final frame's `exposure E (log-average G over N pixels)` and writes the mapped picture - a lamp that the
plain store cuts off at 255 keeps its shape; a curve that is none of the three is an error exit.
(--show-params prints what the arguments give, without a device.)"""
import os
import re
import subprocess

import pytest


def _run(rwr, *args):
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")
    return subprocess.run([exe, *args], capture_output=True, text=True)


def test_cli_tonemap_arguments(rwr):
    r = _run(rwr, "--help")
    assert r.returncode == 0 and "--tonemap [clamp|reinhard|aces]" in r.stdout and "--auto-exposure [KEY]" in r.stdout
    assert "--exposure STOPS" in r.stdout and "--white W" in r.stdout
    r = _run(rwr, "--show-params")
    assert r.returncode == 0 and "tonemap" not in r.stdout and "flags 0x0 " in r.stdout
    r = _run(rwr, "--tonemap", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_TONEMAP:x} " in r.stdout
    assert "tonemap 1 curve aces auto-exposure 0 exposure 1 key 0.18 white 4\n" in r.stdout
    r = _run(rwr, "--tonemap", "reinhard", "--exposure", "-1", "--auto-exposure", "--white", "8", "--show-params")
    assert r.returncode == 0 and "tonemap 1 curve reinhard auto-exposure 1 exposure 0.5 key 0.18 white 8\n" in r.stdout
    for args in (("--exposure", "2"), ("--auto-exposure", "0.25"), ("--white", "2"), ("--auto-exposure",)):   # each implies --tonemap
        r = _run(rwr, *args, "--show-params")
        assert r.returncode == 0 and f"flags 0x{rwr.FLAG_TONEMAP:x} " in r.stdout, args
    assert "exposure 4 key 0.18" in _run(rwr, "--exposure", "2", "--show-params").stdout             # 2^STOPS
    assert "auto-exposure 1 exposure 1 key 0.25" in _run(rwr, "--auto-exposure", "0.25", "--show-params").stdout
    for bad in (("--tonemap", "bad"), ("--tonemap", "ACES"), ("--exposure", "17"), ("--exposure", "nan"), ("--exposure",), ("--auto-exposure", "0"),
                ("--auto-exposure", "1e9"), ("--white", "0"), ("--white", "x"), ("--white",)):
        r = _run(rwr, *bad, "--show-params")
        assert r.returncode == 2 and bad[0] in r.stderr, (bad, r.stderr)


@pytest.mark.gpu
def test_cli_maps_the_lamp(rwr, tmp_path):
    """The README's lamp: sphere 1 emits (8, 7, 5).  With --tonemap aces --auto-exposure the run prints the exposure line and the
    picture has fewer bytes at 255 than the same frame without the option."""
    common = ["--res", rwr.RES_DIR, "--size", "96x64", "--keys", "S*25,D*75", "--spp", "4", "--bounces", "2", "--frames", "1",   # (the README's keys
              "--emissive-sphere", "1:8,7,5"]                                                          # bring the lamp into view)
    plain_png, mapped_png = str(tmp_path / "plain.png"), str(tmp_path / "mapped.png")
    r = _run(rwr, *common, "--out", plain_png)
    assert r.returncode == 0 and "exposure" not in r.stdout, (r.stdout, r.stderr)
    r = _run(rwr, *common, "--tonemap", "aces", "--auto-exposure", "--out", mapped_png)
    assert r.returncode == 0, (r.stdout, r.stderr)
    m = re.search(r"^exposure (\S+) \(log-average (\S+) over (\d+) pixels\)$", r.stdout, re.M)
    assert m, r.stdout
    E, G, n = float(m.group(1)), float(m.group(2)), int(m.group(3))
    assert 0 < n <= 96 * 64 and G > 0 and E == pytest.approx(0.18 / G, rel=1e-4)

    def saturated(path):
        img = rwr.decode_image_rgba8(open(path, "rb").read())
        return int((img[..., :3] == 255).sum())

    assert saturated(plain_png) > 0 and saturated(mapped_png) < saturated(plain_png)
    # a manual frame measures nothing and says so
    r = _run(rwr, *common, "--tonemap", "reinhard", "--exposure", "-2")
    assert r.returncode == 0 and re.search(r"^exposure 0\.25 \(log-average 0 over 0 pixels\)$", r.stdout, re.M), r.stdout
    r = _run(rwr, *common, "--tonemap", "bad")
    assert r.returncode == 2 and "--tonemap" in r.stderr
