"""rwr_render --light-sampling (RWR_FLAG_LIGHT_SAMPLING): the option sets the flag and implies nothing else; a run with it prints the
final frame's `light rays N, reached M`.  (--show-params prints what the arguments give, without a device.)"""
import os
import re
import subprocess

import pytest


def _run(rwr, *args):
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")
    return subprocess.run([exe, *args], capture_output=True, text=True)


def test_cli_light_sampling_arguments(rwr):
    r = _run(rwr, "--help")
    assert r.returncode == 0 and "--light-sampling" in r.stdout and "light rays N, reached M" in r.stdout
    r = _run(rwr, "--bounces", "2", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE:x} " in r.stdout
    r = _run(rwr, "--bounces", "2", "--light-sampling", "--show-params")     # it implies nothing: neither RWR_FLAG_EMISSIVE nor a bounce
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_LIGHT_SAMPLING:x} " in r.stdout
    r = _run(rwr, "--bounces", "1", "--emissive-sphere", "1:8,7,5", "--light-sampling", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_EMISSIVE | rwr.FLAG_LIGHT_SAMPLING:x} " in r.stdout
    assert "emissive 1 sphere 1:8,7,5\n" in r.stdout


@pytest.mark.gpu
def test_cli_prints_the_light_rays(rwr):
    """The reference's spheres, one of them a lamp, seen from behind the mesh (the README's walk: from the front the faces the lamp
    lights look away from the camera): the run prints the light rays of its final frame and how many reached the lamp; the counts
    repeat; without a bounce, without an emitter or without the option nothing is traced or printed."""
    common = ["--res", rwr.RES_DIR, "--size", "96x64", "--spp", "2", "--keys", "S*25,D*75"]

    def counts(*args):
        r = _run(rwr, *common, *args)
        assert r.returncode == 0, (r.stdout, r.stderr)
        m = re.search(r"^light rays (\d+), reached (\d+)$", r.stdout, re.M)
        assert m, r.stdout
        return int(m.group(1)), int(m.group(2))

    lamp = ("--emissive-sphere", "1:8,7,5")
    rays, reached = counts("--bounces", "2", "--light-sampling", *lamp)
    assert rays >= reached > 0 and counts("--bounces", "2", "--light-sampling", *lamp) == (rays, reached)
    assert counts("--bounces", "0", "--light-sampling", *lamp) == (0, 0)          # no hit sends a ray on
    assert counts("--bounces", "2", "--light-sampling") == (0, 0)                 # nothing emits
    assert counts("--bounces", "2", "--light-sampling", "--emissive-part", "0:1,1,1") == (0, 0)   # an emitting part is not aimed at
    r = _run(rwr, *common, "--bounces", "2", *lamp)
    assert r.returncode == 0 and "light rays" not in r.stdout and "emissive hits" in r.stdout
