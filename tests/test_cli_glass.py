"""rwr_render --glass-part / --glass-sphere (RWR_FLAG_GLASS): the two options imply the flag, are repeatable, default to an index
of refraction of 1.5 and a tint of 1,1,1; a malformed index, index of refraction or tint is an error exit that names the option.
(--show-params prints what the arguments give, without a device.)"""
import os
import subprocess


def test_cli_glass_arguments(rwr):
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")

    def run(*args):
        return subprocess.run([exe, *args], capture_output=True, text=True)

    r = run("--help")
    assert r.returncode == 0 and "--glass-part" in r.stdout and "--glass-sphere" in r.stdout
    r = run("--bounces", "2", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE:x} " in r.stdout and " glass 0 mirrors 0" in r.stdout
    r = run("--bounces", "4", "--sky", "--glass-sphere", "1", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_SKY | rwr.FLAG_GLASS:x} " in r.stdout
    assert " glass 1 sphere 1:1.5:1,1,1 mirrors 0" in r.stdout
    r = run("--bounces", "1", "--glass-part", "0:1.33", "--glass-sphere", "7:2.4:0,0.25,1", "--glass-part", "3", "--mirror-sphere", "2", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_GLASS | rwr.FLAG_MIRRORS:x} " in r.stdout
    assert " glass 3 part 0:1.33:1,1,1 sphere 7:2.4:0,0.25,1 part 3:1.5:1,1,1 mirrors 1 sphere 2:1,1,1" in r.stdout
    r = run("--bounces", "1", "--glass-part", "2:1:0.5,0.5,0.5", "--glass-part", "2:4", "--show-params")      # the ends of the range
    assert r.returncode == 0 and " glass 2 part 2:1:0.5,0.5,0.5 part 2:4:1,1,1" in r.stdout
    for opt in ("--glass-part", "--glass-sphere"):
        for bad in ("x", "-1", "1:", "1:x", "1:0.99", "1:4.01", "1:nan", "1:inf", "1:-1.5", "1:1.5:", "1:1.5:0.5", "1:1.5:0.5,0.5", "1:1.5:0.5,0.5,0.5,0.5",
                    "1:1.5:0.5,0.5,1.0001", "1:1.5:-0.1,0,0", "1:1.5:nan,0,0", "1:1.5:inf,0,0", "1;1.5", "", "1:1.5:0.5,0.5,0.5x", "1:1.5x", "1:0.5,0.5,0.5"):
            r = run("--bounces", "1", opt, bad, "--show-params")
            assert r.returncode == 2 and opt in r.stderr, (opt, bad)
        assert run("--bounces", "1", opt).returncode == 2      # the value is missing
    r = run("--bounces", "1", "--glass-sphere", "8", "--show-params")     # RWR_MAX_SPHERES = 8: indices 0 ... 7
    assert r.returncode == 2 and "--glass-sphere" in r.stderr
