"""Mirror surfaces (RWR_FLAG_MIRRORS), host side: the public surface, the reflection against float64, the tests' CPU
reference (mirror_ref.c, built on sky_ref.c and through it on shadow_ref.c, path_ref.c and the oracle) against sky_ref where both
define the frame, the definition's consequences, a closed form, the conditions the GPU file's scenes must meet, and the command
line.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import mirror_common
import mirror_ref
import sky_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
DEFAULT = (sky_ref.DEFAULT_ZENITH, sky_ref.DEFAULT_HORIZON)


@pytest.fixture(scope="module")
def mref(tmp_path_factory):
    return mirror_ref.lib(tmp_path_factory)


def test_header_declares_and_library_exports_the_mirrors(rwr):
    text = open(os.path.join(ROOT, "include", "rwr_hip.h")).read()
    m = re.search(r"RWR_FLAG_MIRRORS\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and int(m.group(1)) == 10
    bits = [int(v) for v in re.findall(r"RWR_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", text)]
    assert bits.count(10) == 1                                  # a bit nobody else has
    assert re.search(r"RWR_API int rwr_scene_set_part_mirror\(rwr_context \*ctx, uint32_t part, const float \*reflectance\);", text)
    assert re.search(r"RWR_API int rwr_scene_set_sphere_mirror\(rwr_context \*ctx, uint32_t sphere, const float \*reflectance\);", text)
    assert re.search(r"RWR_API int rwr_scene_get_part_mirror\(rwr_context \*ctx, uint32_t part, int \*is_mirror, float reflectance\[3\]\);", text)
    assert re.search(r"RWR_API int rwr_scene_get_sphere_mirror\(rwr_context \*ctx, uint32_t sphere, int \*is_mirror, float reflectance\[3\]\);", text)
    assert rwr.FLAG_MIRRORS == 1 << 10
    declared = rwr.exported_symbols_declared_in_header()
    lib = rwr.lib()
    for name in ("rwr_scene_set_part_mirror", "rwr_scene_set_sphere_mirror", "rwr_scene_get_part_mirror", "rwr_scene_get_sphere_mirror"):
        assert name in declared and hasattr(lib, name), name
    for name in ("set_part_mirror", "set_sphere_mirror", "get_part_mirror", "get_sphere_mirror"):
        assert hasattr(rwr.Context, name), name


def test_reflection_against_float64(mref):
    """D' = D - (2 dot3(n, D)) n in f32 against the same expression in float64.  For unit n and D the exact reflection has
    |D'| = |D| and D'.n = -D.n.  The f32 evaluation rounds d (3 products, 2 sums), 2 d (exact), three products and three
    differences: every component of D' is off by at most a handful of 2^-24 of quantities of magnitude <= 2, so |D'| is within
    8 ulp of |D| and D'.n + D.n within 1e-6; the inputs' own distance from unit length (2^-24 relative) is inside that."""
    rng = np.random.default_rng(17)
    n = rng.normal(size=(4000, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = rng.normal(size=(4000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n32, d32 = n.astype(np.float32), d.astype(np.float32)
    worst_len = worst_dot = worst_abs = 0.0
    for k in range(len(n32)):
        got = mirror_ref.reflect(mref, n32[k], d32[k]).astype(np.float64)
        N, D = n32[k].astype(np.float64), d32[k].astype(np.float64)
        want = D - 2.0 * N.dot(D) * N
        worst_abs = max(worst_abs, float(np.abs(got - want).max()))
        worst_len = max(worst_len, abs(np.linalg.norm(got) - np.linalg.norm(D)) / np.spacing(np.float32(np.linalg.norm(D))))
        worst_dot = max(worst_dot, abs(got.dot(N) + D.dot(N)))
    print(f"reflection: |D'| within {worst_len:.2f} ulp of |D|, D'.n + D.n up to {worst_dot:.3g}, against float64 up to {worst_abs:.3g}")
    assert worst_len <= 8.0 and worst_dot <= 1e-6 and worst_abs <= 1e-6
    # an axis normal of either sign flips exactly that component's sign and nothing else
    for axis in range(3):
        for sign in (1.0, -1.0):
            nn = np.zeros(3, np.float32)
            nn[axis] = sign
            for k in range(50):
                want = d32[k].copy()
                want[axis] = -want[axis]
                assert mirror_ref.reflect(mref, nn, d32[k]).tobytes() == want.tobytes(), (axis, sign, k)
    # and it is the definition, one f32 operation at a time
    f = np.float32
    for k in range(200):
        a, b = n32[k], d32[k]
        dd = f(f(f(a[0] * b[0]) + f(a[1] * b[1])) + f(a[2] * b[2]))
        two = f(f(2.0) * dd)
        want = np.array([f(b[c] - f(two * a[c])) for c in range(3)], f)
        assert mirror_ref.reflect(mref, a, b).tobytes() == want.tobytes(), k


@pytest.mark.parametrize("name", ["quad_floor", "soup"])
@pytest.mark.parametrize("bounces", [1, 3])
def test_without_mirrors_it_is_sky_ref(mref, rwr, orc, ref_loader, suzanne, cube, name, bounces):
    """No mirror surface: sky_render_path's bytes and counts — with and without a sky, with shadow rays — on the cube over the quad and
    on the soup.  (The comparison runs sky_ref.c's own loop, compiled into the same library.)"""
    s = dict(mirror_common.scene(name, rwr, ref_loader, suzanne, cube), w=40, h=30, spp=3)
    cam = mirror_common.camera(rwr, s).view(orc.CAMERA_INV_DTYPE)
    for sky, shadows in ((None, False), (DEFAULT, False), (DEFAULT, True)):
        kw = dict(instances=None, shadows=shadows, sky=sky)
        args = (mref, orc, cam, orc.make_screen(s["w"], s["h"]), orc.make_params(3, bounces, seed=7), s["spheres"].view(orc.SPHERE_DTYPE), s["model"])
        want = mirror_ref.render_path(*args, use_sky_ref=True, **kw)
        got = mirror_ref.render_path(*args, **kw)
        for k in PLANES:
            assert got[k].tobytes() == want[k].tobytes(), (name, bounces, sky, shadows, k)
        for k in ("rays", "shadow_rays", "occluded", "sky_terms"):
            assert got[k] == want[k], (name, k)
        assert got["gen_mirror"].sum() == 0 and got["gen_rays"].sum() == got["rays"]
        # a table without a mirror in it is no mirror either
        got = mirror_ref.render_path(*args, mirror_parts={}, mirror_spheres={}, **kw)
        assert got["color_f32"].tobytes() == want["color_f32"].tobytes()


def test_a_path_is_a_prefix_of_the_deeper_path(mref, rwr, orc, ref_loader, suzanne, cube):
    s = dict(mirror_common.scene("soup", rwr, ref_loader, suzanne, cube), w=40, h=30, spp=3)
    frames = [mirror_common.reference(mref, rwr, orc, s, 5, sky=DEFAULT, bounces=b, first=True, name=("prefix", b)) for b in range(0, 5)]
    assert frames[0]["rays"] == 0
    for b, (a, d) in enumerate(zip(frames, frames[1:])):
        assert (d["color_f32"] >= a["color_f32"]).all() and d["rays"] >= a["rays"]
        for k in ("depth", "obj_id", "hit_t"):
            assert a[k].tobytes() == d[k].tobytes()
        # the generations the shallower frame traced are the deeper frame's, ray for ray
        assert np.array_equal(a["gen_rays"][:b + 1], d["gen_rays"][:b + 1]) and np.array_equal(a["gen_mirror"][:b + 1], d["gen_mirror"][:b + 1])
        seen = a["first"][..., 7] > 0
        assert np.array_equal(a["first"][seen], d["first"][seen])
    assert frames[4]["gen_mirror"][1] > 0 and frames[4]["gen_mirror"][2:].sum() > 0


@pytest.mark.parametrize("name", mirror_common.GPU_SCENES)
def test_sample_zero_and_first_generation_do_not_depend_on_the_flag(mref, rwr, orc, ref_loader, suzanne, cube, name):
    s = mirror_common.scene(name, rwr, ref_loader, suzanne, cube)
    on = mirror_common.reference(mref, rwr, orc, s, 13, sky=DEFAULT, first=True, name=name)
    off = mirror_common.reference(mref, rwr, orc, s, 13, mirrors=False, sky=DEFAULT, name=name)
    for k in ("depth", "obj_id", "hit_t"):
        assert on[k].tobytes() == off[k].tobytes(), k
    assert np.array_equal(on["color_f32"][..., 3], off["color_f32"][..., 3])
    assert on["gen_rays"][1] == off["gen_rays"][1] > 0
    # h0's shadow rays too: at B = 0 nothing is left of the flag
    a = mirror_common.reference(mref, rwr, orc, s, 13, shadows=True, bounces=0, spp=2, name=name)
    b = mirror_common.reference(mref, rwr, orc, s, 13, mirrors=False, shadows=True, bounces=0, spp=2, name=name)
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["shadow_rays"], a["occluded"]) == (b["shadow_rays"], b["occluded"])


def test_closed_form_of_the_mirror_quad(mref, rwr, orc, ref_loader, suzanne, cube):
    """One upward-facing mirror quad under the default sky, one centre ray per pixel, B = 1: every reflected ray leaves the scene, so
    a pixel is E(h0) + clamp(R * S(D')).  E(h0) is the frame without a bounce (the oracle's local shading); the sky term is
    recomputed here in numpy float32, one operation at a time, from the D' the reference exports; the sum of the two is one f32
    addition: the frame's bits."""
    f = np.float32
    s = mirror_common.scene("quad_alone", rwr, ref_loader, suzanne, cube)
    got = mirror_common.reference(mref, rwr, orc, s, 3, sky=DEFAULT, first=True, name="quad_alone")
    e0 = mirror_common.reference(mref, rwr, orc, s, 3, sky=DEFAULT, bounces=0, name="quad_alone")
    hit = got["obj_id"] >= 0
    assert hit.any() and not hit.all()
    first = got["first"][:, :, 0]
    assert got["gen_mirror"][1] == got["gen_rays"][1] == hit.sum() and (first[hit][:, 6] == 0).all() and (first[hit][:, 7] == 1).all()
    assert got["sky_terms"] == hit.sum()
    d1 = first[..., 0:3]
    assert (d1[hit][:, 1] > 0).all()                                                   # n = +y: the rays go up
    assert np.abs(np.linalg.norm(d1[hit].astype(np.float64), axis=1) - 1.0).max() <= 4 * 2.0 ** -23
    assert np.array_equal(first[hit][:, 3:6], np.tile(np.asarray(mirror_common.QUAD_R, f), (int(hit.sum()), 1)))   # T0 = R
    z, hz = np.asarray(DEFAULT[0], f), np.asarray(DEFAULT[1], f)
    u = np.minimum(np.maximum(f(0.5) * d1[..., 1] + f(0.5), f(0.0)), f(1.0)).astype(f)
    S = (hz + ((z - hz) * u[..., None]).astype(f)).astype(f)
    term = np.clip((np.asarray(mirror_common.QUAD_R, f) * S).astype(f), f(0.0), f(64.0)) * hit[..., None]
    want = (e0["color_f32"][..., :3] + term.astype(f)).astype(f)
    assert got["color_f32"][..., :3].tobytes() == want.tobytes()
    assert np.array_equal(got["color_f32"][~hit], e0["color_f32"][~hit])


@pytest.mark.parametrize("name", mirror_common.GPU_SCENES)
def test_the_gpu_scenes_exercise_the_mirrors(mref, rwr, orc, ref_loader, suzanne, cube, name):
    """What tests/test_gpu_mirror.py relies on, asserted with the reference alone: reflections in the first generation and in the
    second, reflected rays that find a face, a sphere (where there are spheres) and the sky, and a frame that differs from the
    frame without the flag."""
    s = mirror_common.scene(name, rwr, ref_loader, suzanne, cube)
    on = mirror_common.reference(mref, rwr, orc, s, 13, sky=DEFAULT, first=True, name=name)
    off = mirror_common.reference(mref, rwr, orc, s, 13, mirrors=False, sky=DEFAULT, name=name)
    print(f"{name}: bounce rays per generation {on['gen_rays'][1:].tolist()}, of them reflections {on['gen_mirror'][1:].tolist()}")
    assert s["bounces"] >= 2 and on["gen_mirror"][1] > 0 and on["gen_mirror"][2] > 0
    first = on["first"].reshape(-1, 8)
    first = first[first[:, 7] > 0]
    found = set(np.unique(first[:, 6]).tolist())
    assert 1.0 in found and 0.0 in found, found
    if len(s["spheres"]):
        assert 2.0 in found, found
    assert not np.array_equal(on["color_f32"], off["color_f32"]) and not np.array_equal(on["color"], off["color"])


def test_cli_mirror_arguments(rwr):
    """--mirror-part / --mirror-sphere imply the flag, are repeatable and default to reflectance 1,1,1; a malformed index or an
    out-of-range reflectance is an error exit that names the option.  (--show-params prints what the arguments give, without a device.)"""
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")

    def run(*args):
        return subprocess.run([exe, *args], capture_output=True, text=True)

    r = run("--help")
    assert r.returncode == 0 and "--mirror-part" in r.stdout and "--mirror-sphere" in r.stdout
    r = run("--bounces", "2", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE:x} " in r.stdout and r.stdout.rstrip().endswith("mirrors 0")
    r = run("--bounces", "2", "--sky", "--mirror-sphere", "1", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_SKY | rwr.FLAG_MIRRORS:x} " in r.stdout
    assert r.stdout.rstrip().endswith("mirrors 1 sphere 1:1,1,1")
    r = run("--bounces", "1", "--mirror-part", "0:0.5,0.75,1", "--mirror-sphere", "7:0,0.25,1", "--mirror-part", "3", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MIRRORS:x} " in r.stdout
    assert r.stdout.rstrip().endswith("mirrors 3 part 0:0.5,0.75,1 sphere 7:0,0.25,1 part 3:1,1,1")
    for opt in ("--mirror-part", "--mirror-sphere"):
        for bad in ("x", "-1", "1:", "1:0.5", "1:0.5,0.5", "1:0.5,0.5,0.5,0.5", "1:0.5,0.5,1.0001", "1:-0.1,0,0", "1:nan,0,0", "1:inf,0,0",
                    "1;0,0,0", "", "1:0.5,0.5,0.5x"):
            r = run("--bounces", "1", opt, bad, "--show-params")
            assert r.returncode == 2 and opt in r.stderr, (opt, bad)
        assert run("--bounces", "1", opt).returncode == 2      # the value is missing
    r = run("--bounces", "1", "--mirror-sphere", "8", "--show-params")     # RWR_MAX_SPHERES = 8: indices 0 ... 7
    assert r.returncode == 2 and "--mirror-sphere" in r.stderr
