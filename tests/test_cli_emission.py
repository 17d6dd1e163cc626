"""rwr_render --emissive-part / --emissive-sphere (RWR_FLAG_EMISSIVE): the two options imply the flag, are repeatable and take an
index and a radiance; a malformed index or radiance is an error exit that names the option; the emitters are listed on a line of
their own, so that the line every run prints stays what it was; a run prints the final frame's `emissive hits N`.
(--show-params prints what the arguments give, without a device.)"""
import os
import re
import subprocess

import pytest


def _run(rwr, *args):
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")
    return subprocess.run([exe, *args], capture_output=True, text=True)


def test_cli_emission_arguments(rwr):
    def run(*args):
        return _run(rwr, *args)

    r = run("--help")
    assert r.returncode == 0 and "--emissive-part N:r,g,b" in r.stdout and "--emissive-sphere N:r,g,b" in r.stdout
    r = run("--bounces", "2", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE:x} " in r.stdout and " gloss 0 glass 0 mirrors 0" in r.stdout
    assert "emissive" not in r.stdout
    r = run("--bounces", "2", "--emissive-sphere", "1:8,7,5", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_EMISSIVE:x} " in r.stdout
    assert "emissive 1 sphere 1:8,7,5\n" in r.stdout and " gloss 0 glass 0 mirrors 0" in r.stdout
    r = run("--emissive-part", "0:0.5,0,64", "--emissive-sphere", "7:0,0,0", "--emissive-part", "3:1,2,3", "--mirror-part", "0", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_EMISSIVE | rwr.FLAG_MIRRORS:x} " in r.stdout      # (no bounce is needed: an emitter shows at h0)
    assert "emissive 3 part 0:0.5,0,64 sphere 7:0,0,0 part 3:1,2,3\n" in r.stdout and " gloss 0 glass 0 mirrors 1 part 0:1,1,1" in r.stdout
    for opt in ("--emissive-part", "--emissive-sphere"):
        for bad in ("x", "-1", "1", "1:", "1:x", "1:1", "1:1,1", "1:1,1,1,1", "1:1,1,64.001", "1:-0.1,0,0", "1:nan,0,0", "1:0,inf,0", "1;1,1,1", "",
                    "1:1,1,1x", "1:1:1,1,1", ":1,1,1"):
            r = run(opt, bad, "--show-params")
            assert r.returncode == 2 and opt in r.stderr, (opt, bad)
        assert run(opt).returncode == 2      # the value is missing
    r = run("--emissive-sphere", "8:1,1,1", "--show-params")     # RWR_MAX_SPHERES = 8: indices 0 ... 7
    assert r.returncode == 2 and "--emissive-sphere" in r.stderr


@pytest.mark.gpu
def test_cli_prints_the_emissive_hits(rwr):
    """A glowing mesh: the run prints how many shaded hits of its final frame lay on an emitter; the count repeats; bounce rays find
    the emitter too; an emitter that is all zeros, and a run without the option, count nothing; a part the scene lacks is the library's
    refusal."""
    common = ["--res", rwr.RES_DIR, "--size", "96x64", "--spp", "2", "--frames", "1"]

    def hits(*args):
        r = _run(rwr, *common, *args)
        assert r.returncode == 0, (r.stdout, r.stderr)
        m = re.search(r"^emissive hits (\d+)$", r.stdout, re.M)
        assert m, r.stdout
        return int(m.group(1))

    one = hits("--bounces", "0", "--emissive-part", "0:1,2,3")
    assert one > 0 and hits("--bounces", "0", "--emissive-part", "0:1,2,3") == one
    assert hits("--bounces", "2", "--emissive-part", "0:1,2,3") > one       # the hits of the bounce rays on top
    assert hits("--bounces", "2", "--emissive-part", "0:0,0,0") == 0        # nothing emits: the flag does nothing
    r = _run(rwr, *common, "--bounces", "2")
    assert r.returncode == 0 and "emissive hits" not in r.stdout
    r = _run(rwr, *common, "--bounces", "1", "--emissive-part", "99:1,1,1")
    assert r.returncode == 2 and "--emissive-part" in r.stderr
