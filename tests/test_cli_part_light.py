"""rwr_render --light-parts (RWR_FLAG_LIGHT_PARTS): the option sets the flag and implies nothing else; a run with it prints the final
frame's `part light rays N, reached M`.  (--show-params prints what the arguments give, without a device.)"""
import os
import re
import subprocess

import pytest


def _run(rwr, *args):
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")
    return subprocess.run([exe, *args], capture_output=True, text=True)


def test_cli_light_parts_arguments(rwr):
    r = _run(rwr, "--help")
    assert r.returncode == 0 and "--light-parts" in r.stdout and "part light rays N, reached M" in r.stdout
    r = _run(rwr, "--bounces", "2", "--light-parts", "--show-params")     # it implies nothing: neither RWR_FLAG_EMISSIVE nor a bounce
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_LIGHT_PARTS:x} " in r.stdout
    r = _run(rwr, "--bounces", "1", "--emissive-part", "0:8,7,5", "--light-parts", "--light-sampling", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_EMISSIVE | rwr.FLAG_LIGHT_SAMPLING | rwr.FLAG_LIGHT_PARTS:x} " in r.stdout
    assert "emissive 1 part 0:8,7,5\n" in r.stdout


@pytest.mark.gpu
def test_cli_prints_the_part_light_rays(rwr):
    """The reference's scene with its mesh emitting, seen from behind the mesh (test_cli_light.py's walk): the run prints the light
    rays aimed at the mesh light in its final frame and how many reached their face; the counts repeat; with a lamp and
    --light-sampling beside it the stage's totals hold both; without a bounce, without an emitting part or without the option nothing
    is aimed at a face or printed."""
    common = ["--res", rwr.RES_DIR, "--size", "96x64", "--spp", "2", "--keys", "S*25,D*75"]

    def counts(*args, what="part light rays"):
        r = _run(rwr, *common, *args)
        assert r.returncode == 0, (r.stdout, r.stderr)
        m = re.search(rf"^{what} (\d+), reached (\d+)$", r.stdout, re.M)
        assert m, r.stdout
        return int(m.group(1)), int(m.group(2))

    glow = ("--emissive-part", "0:1,1,1")
    rays, reached = counts("--bounces", "2", "--light-parts", *glow)
    assert rays >= reached > 0 and counts("--bounces", "2", "--light-parts", *glow) == (rays, reached)
    both = ("--bounces", "2", "--light-parts", "--light-sampling", "--emissive-sphere", "1:8,7,5", *glow)
    part, total = counts(*both), counts(*both, what="light rays")
    assert total[0] > part[0] > 0 and total[1] >= part[1]
    assert counts("--bounces", "0", "--light-parts", *glow) == (0, 0)             # no hit sends a ray on
    assert counts("--bounces", "2", "--light-parts") == (0, 0)                    # nothing emits
    assert counts("--bounces", "2", "--light-parts", "--emissive-sphere", "1:8,7,5") == (0, 0)   # an emitting sphere is not this flag's
    r = _run(rwr, *common, "--bounces", "2", *glow)
    assert r.returncode == 0 and "part light rays" not in r.stdout and "emissive hits" in r.stdout
