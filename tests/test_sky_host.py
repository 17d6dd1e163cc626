"""Sky light (RWR_FLAG_SKY), host side: the public surface, the tests' CPU reference (sky_ref.c, built on shadow_ref.c,
path_ref.c and the oracle) against path_ref where both define the frame, the definition's consequences, and the command line.
No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import path_ref
import sky_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
DEFAULT = (sky_ref.DEFAULT_ZENITH, sky_ref.DEFAULT_HORIZON)
BLACK = ((0, 0, 0), (0, 0, 0))
TINTED = ((0.25, 2.0, 0.0), (3.5, 0.5, 0.125))   # zenith below and above horizon, a zero, components above 1


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return sky_ref.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return path_ref.lib(tmp_path_factory)


def _scene(name, rwr, orc, suzanne, cube):
    """(model, spheres, instances, eye, target)"""
    none = np.zeros(0, orc.SPHERE_DTYPE)
    if name == "cube_alone":
        return cube, none, None, (2.2, 1.7, 3.1), (0, 0, 0)
    if name == "cube":
        return cube, orc.make_spheres([((1.6, 1.2, 1.4), 0.5)]), None, (2.2, 1.7, 3.1), (0, 0, 0)
    if name == "grid":
        return suzanne, orc.make_spheres(), rwr.make_instance_grid(2, 3.0).view(orc.INSTANCE_DTYPE), (1.5, -1.5, 7.0), (1.5, -1.5, 0)
    raise KeyError(name)


def _render(L, rwr, orc, scene, w, h, spp, bounces, sky, seed=7, shadows=False, misses=False):
    model, spheres, inst, eye, target = scene
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=eye, target=target, aspect=w / h)).view(orc.CAMERA_INV_DTYPE)
    return sky_ref.render_path(L, orc, cam_inv, orc.make_screen(w, h), orc.make_params(spp, bounces, seed=seed), spheres, model,
                               instances=inst, shadows=shadows, sky=sky, misses=misses)


def test_header_declares_and_library_exports_the_sky(rwr):
    text = open(os.path.join(ROOT, "include", "rwr_hip.h")).read()
    m = re.search(r"RWR_FLAG_SKY\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and int(m.group(1)) == 9
    bits = [int(v) for v in re.findall(r"RWR_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", text)]
    assert bits.count(9) == 1                                  # a bit nobody else has
    assert re.search(r"typedef struct rwr_sky_params\s*\{\s*float zenith\[3\];\s*float horizon\[3\];\s*\}\s*rwr_sky_params;", text)
    assert re.search(r"RWR_API int rwr_sky_set_params\(rwr_context \*ctx, const rwr_sky_params \*params\);", text)
    assert re.search(r"RWR_API int rwr_sky_get_params\(rwr_context \*ctx, rwr_sky_params \*out\);", text)
    assert rwr.FLAG_SKY == 1 << 9
    assert rwr.SKY_PARAMS_DTYPE.itemsize == 24 and rwr.SKY_PARAMS_DTYPE.names == ("zenith", "horizon")
    declared = rwr.exported_symbols_declared_in_header()
    assert "rwr_sky_set_params" in declared and "rwr_sky_get_params" in declared
    lib = rwr.lib()
    assert hasattr(lib, "rwr_sky_set_params") and hasattr(lib, "rwr_sky_get_params")
    assert hasattr(rwr.Context, "sky_set_params") and hasattr(rwr.Context, "sky_get_params")


def test_sky_radiance_is_the_definition(sref):
    """S(D) by the reference's routine against the definition written out in numpy float32 (IEEE, one operation at a time)."""
    f = np.float32
    rng = np.random.default_rng(5)
    dirs = rng.normal(size=(2000, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True).astype(np.float32)
    dirs[:6] = [[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 1.5, 0], [0, -1.5, 0], [0, np.nan, 0]]   # the ends, beyond them, NaN (u = 0)
    for sky in (DEFAULT, TINTED):
        z, hz = np.asarray(sky[0], f), np.asarray(sky[1], f)
        for d in dirs:
            u = f(0.5) * d[1] + f(0.5)
            u = f(0.0) if np.isnan(u) else min(max(u, f(0.0)), f(1.0))
            want = hz + (z - hz) * f(u)
            assert sky_ref.radiance(sref, sky, d).tobytes() == want.astype(f).tobytes(), (sky, d)
    assert sky_ref.radiance(sref, DEFAULT, (0, 1, 0)).tolist() == [0.5, pytest.approx(0.7), 1.0]
    assert sky_ref.radiance(sref, DEFAULT, (0, -1, 0)).tolist() == [1.0, 1.0, 1.0]


@pytest.mark.parametrize("bounces", [1, 2, 8])
def test_black_sky_and_no_sky_are_path_ref(sref, pref, rwr, orc, suzanne, cube, bounces):
    for name in ("cube", "grid"):
        scene = _scene(name, rwr, orc, suzanne, cube)
        model, spheres, inst, eye, target = scene
        w, h, spp = 40, 30, 3
        cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=eye, target=target, aspect=w / h)).view(orc.CAMERA_INV_DTYPE)
        want = path_ref.render_path(pref, orc, cam_inv, orc.make_screen(w, h), orc.make_params(spp, bounces, seed=7), spheres, model, instances=inst)
        for sky in (BLACK, None):
            got = _render(sref, rwr, orc, scene, w, h, spp, bounces, sky)
            for k in PLANES:
                assert got[k].tobytes() == want[k].tobytes(), (name, bounces, sky, k)
            assert got["rays"] == want["rays"]
        assert _render(sref, rwr, orc, scene, w, h, spp, bounces, BLACK)["sky_terms"] > 0     # (the terms were there, and were zero)


@pytest.mark.parametrize("sky", [DEFAULT, TINTED], ids=["default", "tinted"])
def test_lone_cube_gets_the_mean_of_its_sky_terms(sref, rwr, orc, suzanne, cube, sky):
    """A lone convex mesh: every bounce ray misses (asserted from the reference's counts), so a pixel is the pixel without the sky
    plus (sum over samples of clamp(albedo * S(D1), 0, 64)) / spp, recomputed here from the directions and throughputs the
    reference exports.
    Bound: both frames sum non-negative f32 terms in order and divide by spp.  The frame with the sky makes 2 spp additions and
    one division, the one without spp and one: at most 3 spp + 2 roundings, each at most 2^-24 of a partial sum, and no partial
    sum exceeds the sky frame's total - so after the division the two differ from exact arithmetic by at most
    (3 spp + 2) 2^-24 x (the sky frame's pixel value, rounded up by one more 2^-24).  The terms themselves are recomputed in
    float32 operation by operation (the same bits) and summed in float64 (error below 2^-50, ignored)."""
    f = np.float32
    w, h, spp = 16, 12, 4
    scene = _scene("cube_alone", rwr, orc, suzanne, cube)
    on = _render(sref, rwr, orc, scene, w, h, spp, 1, sky, misses=True)
    off = _render(sref, rwr, orc, scene, w, h, spp, 1, None)
    hit = off["color_f32"][..., 3] > 0
    assert hit.any() and not hit.all()
    assert on["rays"] > 0 and on["sky_terms"] == on["rays"] == off["rays"]             # every bounce ray missed
    assert not np.array_equal(off["color_f32"], on["color_f32"])
    m = on["misses"]
    assert int(m[..., 7].sum()) == on["sky_terms"] and set(np.unique(m[..., 6])) <= {0.0, 1.0}
    z, hz = np.asarray(sky[0], f), np.asarray(sky[1], f)
    u = np.minimum(np.maximum(f(0.5) * m[..., 1] + f(0.5), f(0.0)), f(1.0)).astype(f)
    S = (hz + ((z - hz) * u[..., None]).astype(f)).astype(f)                             # (h, w, spp, 3)
    term = np.clip((m[..., 3:6] * S).astype(f), f(0.0), f(64.0)) * m[..., 7:8]
    want = off["color_f32"][..., :3].astype(np.float64) + term.astype(np.float64).sum(axis=2) / spp
    bound = (3 * spp + 2) * 2.0 ** -24 * on["color_f32"][..., :3].astype(np.float64) * (1 + 2.0 ** -24)
    err = np.abs(on["color_f32"][..., :3].astype(np.float64) - want)
    print(f"lone cube: largest error {err.max():.3g}, bound there {bound.flat[err.argmax()]:.3g}")
    assert (err <= bound).all()
    # background pixels: untouched
    assert np.array_equal(on["color_f32"][~hit], off["color_f32"][~hit]) and (on["obj_id"][~hit] == -1).all()
    assert np.array_equal(on["color_f32"][..., 3], off["color_f32"][..., 3])


@pytest.mark.parametrize("name", ["cube", "grid"])
def test_sky_only_adds_light_and_leaves_sample_zero_alone(sref, rwr, orc, suzanne, cube, name):
    scene = _scene(name, rwr, orc, suzanne, cube)
    for bounces, shadows in ((1, False), (3, False), (3, True)):
        off = _render(sref, rwr, orc, scene, 40, 30, 3, bounces, None, shadows=shadows)
        on = _render(sref, rwr, orc, scene, 40, 30, 3, bounces, DEFAULT, shadows=shadows)
        assert (on["color_f32"] >= off["color_f32"]).all() and (on["color"] >= off["color"]).all()
        assert (on["color_f32"][..., :3] > off["color_f32"][..., :3]).any()
        for k in ("depth", "obj_id", "hit_t"):
            assert on[k].tobytes() == off[k].tobytes(), k
        assert np.array_equal(on["color_f32"][..., 3], off["color_f32"][..., 3])
        # the rays are the same rays, and a sky term casts no shadow ray
        assert (on["rays"], on["shadow_rays"], on["occluded"]) == (off["rays"], off["shadow_rays"], off["occluded"])
        assert 0 < on["sky_terms"] <= on["rays"]


def test_a_path_is_a_prefix_of_the_deeper_path(sref, rwr, orc, suzanne, cube):
    scene = _scene("grid", rwr, orc, suzanne, cube)
    frames = [_render(sref, rwr, orc, scene, 40, 30, 3, b, TINTED, misses=True) for b in range(0, 5)]
    assert frames[0]["sky_terms"] == 0
    for b, (a, d) in enumerate(zip(frames, frames[1:])):
        assert (d["color_f32"] >= a["color_f32"]).all() and d["rays"] >= a["rays"] and d["sky_terms"] >= a["sky_terms"]
        for k in ("depth", "obj_id", "hit_t"):
            assert a[k].tobytes() == d[k].tobytes()
        # a sample whose path ended in the sky within b bounces ends there, with the same ray and throughput, in the deeper frame
        ended = a["misses"][..., 7] == 1
        assert np.array_equal(a["misses"][ended], d["misses"][ended])
        later = (d["misses"][..., 7] == 1) & ~ended
        assert (d["misses"][later][:, 6] == b + 1).all()
    assert frames[4]["sky_terms"] > frames[1]["sky_terms"]     # some paths reach the sky at their second bounce or later


def test_cli_sky_arguments(rwr):
    """--sky-zenith / --sky-horizon imply --sky; a malformed or out-of-range colour is an error exit.  (--show-params prints what the
    arguments give and needs no device.)"""
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")

    def run(*args):
        return subprocess.run([exe, *args], capture_output=True, text=True)

    r = run("--help")
    assert r.returncode == 0 and "--sky-zenith" in r.stdout and "--sky-horizon" in r.stdout
    r = run("--bounces", "1", "--show-params")
    assert r.returncode == 0 and "flags 0x0 sky 0 zenith 0.5,0.7,1 horizon 1,1,1" in r.stdout
    r = run("--bounces", "1", "--sky", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_SKY:x} sky 1 zenith 0.5,0.7,1 horizon 1,1,1" in r.stdout
    r = run("--bounces", "2", "--sky-zenith", "0.25,0.5,2", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_SKY | rwr.FLAG_MULTI_BOUNCE:x} sky 1 zenith 0.25,0.5,2 horizon 1,1,1" in r.stdout
    r = run("--bounces", "1", "--sky-horizon", "0,16,0.5", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_SKY:x} sky 1 zenith 0.5,0.7,1 horizon 0,16,0.5" in r.stdout
    for bad in ("0.1,0.2", "0.1,0.2,x", "1,2,3,4", "1,2,3x", "", "1,2,nan", "1,2,inf", "-0.5,0,0", "0,0,16.5"):
        for opt in ("--sky-zenith", "--sky-horizon"):
            r = run("--bounces", "1", opt, bad, "--show-params")
            assert r.returncode == 2 and opt in r.stderr, (opt, bad)
    assert run("--bounces", "1", "--sky-zenith").returncode == 2      # the value is missing
