"""rwr_render --gloss-part / --gloss-sphere (RWR_FLAG_GLOSSY): the two options imply the flag, are repeatable, need a roughness
and default to a reflectance of 1,1,1; a malformed index, roughness or reflectance is an error exit that names the option; they are
applied after the mirror and glass options; a run prints the final frame's `glossy rays N`.
(--show-params prints what the arguments give, without a device.)"""
import os
import re
import subprocess

import pytest


def _run(rwr, *args):
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")
    return subprocess.run([exe, *args], capture_output=True, text=True)


def test_cli_gloss_arguments(rwr):
    def run(*args):
        return _run(rwr, *args)

    r = run("--help")
    assert r.returncode == 0 and "--gloss-part" in r.stdout and "--gloss-sphere" in r.stdout
    r = run("--bounces", "2", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE:x} " in r.stdout and " gloss 0 glass 0 mirrors 0" in r.stdout
    r = run("--bounces", "4", "--sky", "--gloss-sphere", "1:0.25", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_SKY | rwr.FLAG_GLOSSY:x} " in r.stdout
    assert " gloss 1 sphere 1:0.25:1,1,1 glass 0 mirrors 0" in r.stdout
    r = run("--bounces", "1", "--gloss-part", "0:0.5", "--gloss-sphere", "7:0.125:0,0.25,1", "--gloss-part", "3:1", "--mirror-sphere", "2", "--glass-part", "1",
            "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_GLOSSY | rwr.FLAG_GLASS | rwr.FLAG_MIRRORS:x} " in r.stdout
    assert " gloss 3 part 0:0.5:1,1,1 sphere 7:0.125:0,0.25,1 part 3:1:1,1,1 glass 1 part 1:1.5:1,1,1 mirrors 1 sphere 2:1,1,1" in r.stdout
    r = run("--bounces", "1", "--gloss-part", "2:0.0009765625:0.5,0.5,0.5", "--gloss-part", "2:1", "--show-params")      # the ends of the range
    assert r.returncode == 0 and " gloss 2 part 2:0.000976562:0.5,0.5,0.5 part 2:1:1,1,1" in r.stdout
    for opt in ("--gloss-part", "--gloss-sphere"):
        for bad in ("x", "-1", "1", "1:", "1:x", "1:0", "1:0.0009", "1:1.01", "1:nan", "1:inf", "1:-0.5", "1:0.5:", "1:0.5:0.5", "1:0.5:0.5,0.5",
                    "1:0.5:0.5,0.5,0.5,0.5", "1:0.5:0.5,0.5,1.0001", "1:0.5:-0.1,0,0", "1:0.5:nan,0,0", "1:0.5:inf,0,0", "1;0.5", "", "1:0.5:0.5,0.5,0.5x",
                    "1:0.5x", "1:0.5,0.5,0.5"):
            r = run("--bounces", "1", opt, bad, "--show-params")
            assert r.returncode == 2 and opt in r.stderr, (opt, bad)
        assert run("--bounces", "1", opt).returncode == 2      # the value is missing
    r = run("--bounces", "1", "--gloss-sphere", "8:0.5", "--show-params")     # RWR_MAX_SPHERES = 8: indices 0 ... 7
    assert r.returncode == 2 and "--gloss-sphere" in r.stderr


@pytest.mark.gpu
def test_cli_prints_the_glossy_rays(rwr):
    """A satin mesh: the run prints how many rays the glossy hits of its final frame sent on; the count repeats; the gloss option
    wins over a mirror option for the same part (it is applied after it); a part the scene lacks is the library's refusal."""
    common = ["--res", rwr.RES_DIR, "--size", "96x64", "--spp", "2", "--frames", "1"]

    def glossy(*args):
        r = _run(rwr, *common, *args)
        assert r.returncode == 0, (r.stdout, r.stderr)
        m = re.search(r"^glossy rays (\d+)$", r.stdout, re.M)
        assert m, r.stdout
        return int(m.group(1))

    one = glossy("--bounces", "2", "--gloss-part", "0:0.25")
    assert one > 0 and glossy("--bounces", "2", "--gloss-part", "0:0.25") == one
    assert glossy("--bounces", "2", "--gloss-part", "0:0.25", "--mirror-part", "0") == one      # applied after the mirrors: the gloss wins
    assert glossy("--bounces", "0", "--gloss-part", "0:0.25") == 0                            # no bounce: the flag does nothing
    r = _run(rwr, *common, "--bounces", "2")
    assert r.returncode == 0 and "glossy rays" not in r.stdout
    r = _run(rwr, *common, "--bounces", "1", "--gloss-part", "99:0.5")
    assert r.returncode == 2 and "--gloss-part" in r.stderr
