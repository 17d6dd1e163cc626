"""Soft shadows (RWR_FLAG_SOFT_SHADOWS), host side: the tests' CPU reference (soft_shadow_ref.c) against the stack
below it with the lights' size off, the rule for single inputs, the coverage condition of the parity scenes (enough shadow rays
whose answer the lights' size changes, in both directions), a penumbra on the floor-and-blocker scene, the public constants
and the command line's parsing.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gloss_ref
import shadow_common as sc
import shadow_ref
import soft_shadow_ref as ssr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
W, H = sc.W, sc.H
COVERAGE_SCENES = ("cube", "suzanne_side", "two_parts")
RADIUS = 0.2   # the parity tests' radius: at the default 0.05 only about 1 % of these scenes' shadow rays change their answer


@pytest.fixture(scope="module")
def soft(tmp_path_factory):
    return ssr.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return shadow_ref.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def coverage_frames(soft, rwr, orc, suzanne, cube):
    """name -> (soft reference frame at the coverage condition's size, the hard frame of the same call)."""
    out = {}
    for name in COVERAGE_SCENES:
        s = sc.scene(name, rwr, orc, suzanne, cube)
        cam_inv = sc.camera(rwr, orc, s)
        out[name] = (ssr.reference(soft, orc, s, cam_inv, W, H, 5, 2, radii=(RADIUS, RADIUS)), ssr.reference(soft, orc, s, cam_inv, W, H, 5, 2))
    return out


@pytest.mark.parametrize("name", ["cube", "suzanne_side", "grid", "two_parts", "cube_nmap"])
def test_radii_zero_is_the_shadow_reference(soft, sref, rwr, orc, suzanne, cube, name):
    """Radii 0 - S = L + 0 * (...) = L - and no radii at all both give shadow_ref.c's planes and counts, byte for byte."""
    s = sc.scene(name, rwr, orc, suzanne, cube)
    cam_inv = sc.camera(rwr, orc, s, 48, 32)
    for bounces, spp in ((0, 1), (1, 3), (3, 2)):
        want = sc.reference(shadow_ref, sref, orc, s, cam_inv, 48, 32, spp, bounces)
        for radii in ((0.0, 0.0), None):
            got = ssr.reference(soft, orc, s, cam_inv, 48, 32, spp, bounces, radii=radii)
            for k in PLANES:
                assert got[k].tobytes() == want[k].tobytes(), (name, bounces, spp, radii, k)
            assert (got["rays"], got["shadow_rays"], got["occluded"]) == (want["rays"], want["shadow_rays"], want["occluded"])
            assert got["changed_to_lit"] == 0 and got["changed_to_dark"] == 0
    # one radius 0: hits lit by that light keep the hard answer - the spheres' own rays when the sphere light is a point
    mesh_only = ssr.reference(soft, orc, s, cam_inv, 48, 32, 1, 0, radii=(0.3, 0.0))
    hard = ssr.reference(soft, orc, s, cam_inv, 48, 32, 1, 0)
    on_sphere = hard["obj_id"] <= -2
    assert np.array_equal(mesh_only["occluded0"][on_sphere], hard["occluded0"][on_sphere]), name


def test_the_rule_for_single_inputs(soft, orc):
    """S = L + r (a b1 + b b2) with bounce_direction's disk point and basis: L at r = 0, within r of L, |S| >= 1 up to rounding,
    dimensions 130 + 16 k (a bounce direction of the same dimensions shares the disk point), another point per pixel, sample, k, seed."""
    lights = [-np.array(v, np.float32) / np.float32(np.sqrt(np.float32(27.0))) for v in ((1, -1, -5), (1, -5, 1))]
    for light in lights:
        assert np.array_equal(ssr.direction(soft, light, 0.0, pixel=5, sample=3, k=2, seed=9), light)
        seen = set()
        for pixel, sample, k, seed in ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (2, 0, 0, 1), (77, 5, 8, 123)):   # (the hash starts from seed ^ pixel: pixel 0 seed 1 IS pixel 1 seed 0)
            S = ssr.direction(soft, light, 0.25, pixel, sample, k, seed)
            d = (S - light).astype(np.float64)
            assert np.linalg.norm(d) <= 0.25 * (1 + 1e-5) and abs(d @ light.astype(np.float64)) < 1e-6   # in the plane across L
            assert np.linalg.norm(S.astype(np.float64)) >= 1.0 - 1e-6
            # the disk point is pr_bounce_direction_dim's of dimension block 130 + 16 k: that direction is (a b1 + b b2 + dz L) normalised
            X = gloss_ref.bounce_direction(soft, light, pixel, sample, 130 + 16 * k, seed).astype(np.float64)
            flat = X - (X @ light.astype(np.float64)) * light.astype(np.float64)
            assert np.allclose(flat * 0.25, d, atol=2e-6), (pixel, sample, k, seed)
            seen.add(S.tobytes())
        assert len(seen) == 6


@pytest.mark.parametrize("name", COVERAGE_SCENES)
def test_coverage_condition(coverage_frames, name):
    """The lights' size changes the answer of at least 1 % of the shadow rays (and at least 20), at least 5 in either direction,
    and the scene stays mixed: a GPU that ignored the radii, or made every ray lit or dark, cannot pass parity on these scenes."""
    on, hard = coverage_frames[name]
    rays, lit, dark = on["shadow_rays"], on["changed_to_lit"], on["changed_to_dark"]
    print(f"{name}: {lit} shadow rays changed to lit, {dark} to dark, of {rays} ({100.0 * (lit + dark) / rays:.2f} %); occluded {on['occluded']}")
    assert lit + dark >= max(20, 0.01 * rays), (name, lit, dark, rays)
    assert lit >= 5 and dark >= 5, (name, lit, dark)
    assert 0.1 <= on["occluded"] / rays <= 0.9, (name, on["occluded"], rays)
    assert on["occluded"] == hard["occluded"] - lit + dark


@pytest.mark.parametrize("name", COVERAGE_SCENES)
def test_only_visibility_changes(coverage_frames, name):
    """Sample-0 planes, alpha, the bounce rays and the number of shadow rays are the hard frame's; the colour is not."""
    on, hard = coverage_frames[name]
    for k in ("depth", "obj_id", "hit_t"):
        assert on[k].tobytes() == hard[k].tobytes(), (name, k)
    assert on["color_f32"][..., 3].tobytes() == hard["color_f32"][..., 3].tobytes()
    assert on["rays"] == hard["rays"] and on["shadow_rays"] == hard["shadow_rays"] and np.array_equal(on["gen_rays"], hard["gen_rays"])
    assert on["color_f32"].tobytes() != hard["color_f32"].tobytes()


def test_shadow_ray_count_is_the_hard_frames(soft, sref, rwr, orc, suzanne, cube):
    for name in ("cube", "suzanne_side", "grid", "two_parts", "cube_nmap"):
        s = sc.scene(name, rwr, orc, suzanne, cube)
        cam_inv = sc.camera(rwr, orc, s, 48, 32)
        for bounces, spp in ((0, 1), (1, 3), (4, 2)):
            hard = sc.reference(shadow_ref, sref, orc, s, cam_inv, 48, 32, spp, bounces)
            for radii in ((RADIUS, RADIUS), (0.3, 0.0), (1.0, 1.0)):
                on = ssr.reference(soft, orc, s, cam_inv, 48, 32, spp, bounces, radii=radii)
                assert (on["shadow_rays"], on["rays"]) == (hard["shadow_rays"], hard["rays"]), (name, bounces, spp, radii)


def _blocker_scene(ref_loader, orc, suzanne):
    return (sc.triangle_model(ref_loader, [sc.FLOOR, sc.BLOCKER], suzanne["texture"]), np.zeros(0, orc.SPHERE_DTYPE), None, (3.0, -3.0, 6.0), (0, 0, 0), 0)


def test_penumbra_on_the_floor(soft, rwr, orc, ref_loader, suzanne):
    """The floor-and-blocker triangles of shadow_common.py, 64 samples of the light per pixel: along the row through the middle of
    the blocker's shadow the lit share of the primary hits takes at least three distinct values strictly between 0 and 1; with
    radius 0 it takes none.
    A frame of 64 spp jitters its primary rays, so a pixel ON the hard shadow's edge has a share between 0 and 1 at radius 0 too
    (some of its samples land inside the shadow, some outside).  The statement is therefore checked twice: on 64 frames of one
    sample (seeds 0 ... 63: the primary ray goes through the pixel's centre every time, only the light's point differs), where it
    holds as written; and on one frame of 64 spp over the pixels whose hard-shadow share is 0 or 1, i.e. off the hard edge."""
    s = _blocker_scene(ref_loader, orc, suzanne)
    cam_inv = sc.camera(rwr, orc, s, W, H)

    def shares(radii, spp, seeds):
        total = np.zeros((H, W, 2), np.int64)
        for seed in seeds:
            total += ssr.reference(soft, orc, s, cam_inv, W, H, spp, 0, seed=seed, radii=radii)["primary"]
        return total

    hard1 = shares((0.0, 0.0), 1, range(64))
    soft1 = shares((RADIUS, RADIUS), 1, range(64))
    assert np.array_equal(hard1[..., 0], soft1[..., 0])
    dark_px = (hard1[..., 0] == 64) & (hard1[..., 1] == 0)
    row = int(np.argmax(dark_px.sum(axis=1)))
    assert dark_px[row].sum() >= 4, "the row crosses the shadow"
    hit = hard1[row, :, 0] == 64
    share_hard = hard1[row, hit, 1] / 64.0
    share_soft = soft1[row, hit, 1] / 64.0
    between = lambda v: sorted(set(float(x) for x in v if 0.0 < x < 1.0))
    print(f"row {row}: hard shares {sorted(set(share_hard))}; soft shares strictly between 0 and 1: {between(share_soft)}")
    assert between(share_hard) == []
    assert len(between(share_soft)) >= 3
    assert (share_soft == 0.0).any() and (share_soft == 1.0).any()   # an umbra and full light remain on the row

    hard64 = shares((0.0, 0.0), 64, [5])
    soft64 = shares((RADIUS, RADIUS), 64, [5])
    assert np.array_equal(hard64[..., 0], soft64[..., 0])
    off_edge = (hard64[row, :, 0] > 0) & ((hard64[row, :, 1] == 0) | (hard64[row, :, 1] == hard64[row, :, 0]))
    v = soft64[row, off_edge, 1] / soft64[row, off_edge, 0]
    print(f"row {row}, one frame of 64 spp, pixels off the hard edge: soft shares strictly between 0 and 1: {between(v)}")
    assert len(between(v)) >= 3


def test_header_driver_and_library_agree(rwr):
    text = open(os.path.join(ROOT, "include", "rwr_hip.h")).read()
    m = re.search(r"RWR_FLAG_SOFT_SHADOWS\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and int(m.group(1)) == 14
    assert rwr.FLAG_SOFT_SHADOWS == 1 << 14
    bits = [int(v) for v in re.findall(r"RWR_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", text)]
    assert bits.count(14) == 1 and len(set(bits)) == len(bits)
    assert re.search(r"typedef struct rwr_shadow_params\s*\{\s*float\s+mesh_light_radius\s*,\s*sphere_light_radius\s*;\s*\}\s*rwr_shadow_params;", text)
    assert re.search(r"RWR_API\s+int\s+rwr_shadow_set_params\s*\(\s*rwr_context\s*\*\s*\w*,\s*const\s+rwr_shadow_params\s*\*\s*\w*\)", text)
    assert re.search(r"RWR_API\s+int\s+rwr_shadow_get_params\s*\(\s*rwr_context\s*\*\s*\w*,\s*rwr_shadow_params\s*\*\s*\w*\)", text)
    assert re.search(r"#define\s+RWR_SHADOW_DEFAULTS\s+\{0\.05f,\s*0\.05f\}", text)
    assert rwr.SHADOW_PARAMS_DTYPE.itemsize == 8 and rwr.SHADOW_PARAMS_DTYPE.names == ("mesh_light_radius", "sphere_light_radius")
    lib = C.CDLL(rwr.LIB_PATH)
    assert hasattr(lib, "rwr_shadow_set_params") and hasattr(lib, "rwr_shadow_get_params")
    assert hasattr(rwr.Context, "shadow_set_params") and hasattr(rwr.Context, "shadow_get_params")
    # a NULL context is refused without a device
    L = rwr.lib()
    p = np.zeros(1, rwr.SHADOW_PARAMS_DTYPE)
    assert L.rwr_shadow_set_params(None, p.ctypes.data_as(C.c_void_p)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_shadow_get_params(None, p.ctypes.data_as(C.c_void_p)) == rwr.ERR_INVALID_ARGUMENT


def test_cli_soft_shadow_arguments(rwr):
    """--soft-shadows R[,R2] implies --shadows; one value sets both lights; a malformed or out-of-range radius is an error exit.
    (--show-params prints what the arguments give, without a device.)"""
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")

    def run(*args):
        return subprocess.run([exe] + list(args), capture_output=True, text=True)

    r = run("--help")
    assert r.returncode == 0 and "--soft-shadows" in r.stdout
    r = run("--shadows", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_SHADOWS:x} " in r.stdout and "soft-shadows" not in r.stdout
    r = run("--soft-shadows", "0.2", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_SHADOWS | rwr.FLAG_SOFT_SHADOWS:x} " in r.stdout and "soft-shadows 1 radii 0.2,0.2\n" in r.stdout
    r = run("--bounces", "3", "--soft-shadows", "0.3,0", "--show-params")
    assert r.returncode == 0 and f"flags 0x{rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_SHADOWS | rwr.FLAG_SOFT_SHADOWS:x} " in r.stdout
    assert "soft-shadows 1 radii 0.3,0\n" in r.stdout
    r = run("--soft-shadows", "0,1", "--show-params")       # the ends of the range
    assert r.returncode == 0 and "soft-shadows 1 radii 0,1\n" in r.stdout
    for bad in ("", "x", "0.2,", ",0.2", "0.2,0.2,0.2", "-0.1", "1.5", "0.2,2", "nan", "inf", "0.2,nan", "0.2x"):
        r = run("--soft-shadows", bad, "--show-params")
        assert r.returncode == 2 and "--soft-shadows" in r.stderr, bad
