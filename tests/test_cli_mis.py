"""rwr_render --light-mis (RWR_FLAG_LIGHT_MIS): the option sets the flag and implies nothing else; without a light flag in effect it
changes nothing in the written frame, with one it weights hits and changes none of the light stage's counts.  (--show-params prints what
the arguments give, without a device.)"""
import os
import re
import subprocess

import pytest


def _run(rwr, *args):
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")
    return subprocess.run([exe, *args], capture_output=True, text=True)


def test_cli_light_mis_arguments(rwr):
    r = _run(rwr, "--help")
    assert r.returncode == 0 and "--light-mis" in r.stdout and "RWR_FLAG_LIGHT_MIS" in r.stdout and "weighted hits N" in r.stdout
    r = _run(rwr, "--bounces", "2", "--light-mis", "--show-params")     # it implies nothing: no light flag, no RWR_FLAG_EMISSIVE, no bounce
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_LIGHT_MIS:x} " in r.stdout
    r = _run(rwr, "--light-mis", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_LIGHT_MIS:x} " in r.stdout
    r = _run(rwr, "--bounces", "1", "--emissive-part", "0:8,7,5", "--light-parts", "--light-sampling", "--light-mis", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_EMISSIVE | rwr.FLAG_LIGHT_SAMPLING | rwr.FLAG_LIGHT_PARTS | rwr.FLAG_LIGHT_MIS:x} " in r.stdout
    r = _run(rwr, "--bounces", "1", "--emissive-part", "0:8,7,5", "--light-parts", "--show-params")      # and nothing implies it
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_EMISSIVE | rwr.FLAG_LIGHT_PARTS:x} " in r.stdout


@pytest.mark.gpu
def test_cli_light_mis_weights_hits_only_beside_a_light_flag(rwr, tmp_path):
    """The reference's scene with its mesh emitting, seen from behind the mesh (test_cli_part_light.py's walk).  Without a light flag
    the written frame is the frame without the option, byte for byte, and no hit is weighted; beside --light-parts the light rays and
    the reached count stay, the hits it weights are printed, and those of them whose value is not zero are emissive hits again (the
    frame is too small, 38 light rays, for its 8-bit image to have to differ)."""
    common = ["--res", rwr.RES_DIR, "--size", "96x64", "--spp", "2", "--keys", "S*25,D*75", "--bounces", "2", "--emissive-part", "0:1,1,1"]

    def run(out, *args):
        path = str(tmp_path / out)
        r = _run(rwr, *common, *args, "--out", path)
        assert r.returncode == 0, (r.stdout, r.stderr)
        return open(path, "rb").read(), r.stdout

    plain, text = run("plain.png")
    assert "weighted hits" not in text
    alone, text = run("alone.png", "--light-mis")
    assert alone == plain and re.search(r"^weighted hits 0$", text, re.M), text
    parts, text_parts = run("parts.png", "--light-parts")
    mis, text_mis = run("mis.png", "--light-parts", "--light-mis")
    assert parts != plain
    rays = lambda t: re.search(r"^part light rays (\d+), reached (\d+)$", t, re.M).groups()
    hits = lambda t: int(re.search(r"^emissive hits (\d+)$", t, re.M).group(1))
    assert rays(text_mis) == rays(text_parts) and int(rays(text_mis)[1]) > 0
    weighted = int(re.search(r"^weighted hits (\d+)$", text_mis, re.M).group(1))
    assert weighted > 0 and hits(text_parts) < hits(text_mis) <= hits(text_parts) + weighted and "weighted hits" not in text_parts
