"""Glossy surfaces (RWR_FLAG_GLOSSY), host side: the public surface, the rule for single inputs, the tests' CPU
reference (gloss_ref.c, built on glass_ref.c and through it on the oracle) against glass_ref where both define the frame, and the
conditions the GPU file's scenes must meet - asserted here, not assumed.  No GPU."""
import os
import re

import numpy as np
import pytest

import gloss_common
import gloss_ref
import path_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
DEFAULT = (gloss_ref.glass_ref.DEFAULT_ZENITH, gloss_ref.glass_ref.DEFAULT_HORIZON)
COUNTS = ("rays", "shadow_rays", "occluded", "sky_terms", "events", "multi", "deep")


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return gloss_ref.lib(tmp_path_factory)


def test_header_declares_and_library_exports_the_gloss(rwr):
    text = open(os.path.join(ROOT, "include", "rwr_hip.h")).read()
    m = re.search(r"RWR_FLAG_GLOSSY\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and int(m.group(1)) == 13
    bits = [int(v) for v in re.findall(r"RWR_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", text)]
    assert bits.count(13) == 1                                  # a bit nobody else has
    assert re.search(r"RWR_API int rwr_scene_set_part_gloss\(rwr_context \*ctx, uint32_t part, const float \*reflectance, float roughness\);", text)
    assert re.search(r"RWR_API int rwr_scene_set_sphere_gloss\(rwr_context \*ctx, uint32_t sphere, const float \*reflectance, float roughness\);", text)
    assert re.search(r"RWR_API int rwr_scene_get_part_gloss\(rwr_context \*ctx, uint32_t part, int \*is_glossy, float reflectance\[3\], float \*roughness\);", text)
    assert re.search(r"RWR_API int rwr_scene_get_sphere_gloss\(rwr_context \*ctx, uint32_t sphere, int \*is_glossy, float reflectance\[3\], float \*roughness\);", text)
    assert re.search(r"RWR_API int rwr_last_gloss_stats\(rwr_context \*ctx, uint64_t \*glossy_rays\);", text)
    assert rwr.FLAG_GLOSSY == 1 << 13
    declared = rwr.exported_symbols_declared_in_header()
    lib = rwr.lib()
    for name in ("rwr_scene_set_part_gloss", "rwr_scene_set_sphere_gloss", "rwr_scene_get_part_gloss", "rwr_scene_get_sphere_gloss", "rwr_last_gloss_stats"):
        assert name in declared and hasattr(lib, name), name
    for name in ("set_part_gloss", "set_sphere_gloss", "get_part_gloss", "get_sphere_gloss", "last_gloss_stats"):
        assert hasattr(rwr.Context, name), name


def _face_hits(rng, count):
    """Seeded random face hits: a unit normal flipped towards the ray, a direction of any length."""
    for k in range(count):
        n = rng.normal(size=3)
        n = (n / np.linalg.norm(n)).astype(np.float32)
        d = (rng.normal(size=3) * rng.uniform(0.2, 3.0)).astype(np.float32)
        if float(n.astype(np.float64) @ d.astype(np.float64)) > 0:
            n = -n
        yield k, n, d


def test_the_rule_for_single_inputs(sref):
    """gloss_scatter against the definition written out one f32 operation at a time; at rho = 1 it is bounce_direction's
    components exactly; for a face hit S stays on n's side (dot(S, n) in float64 >= -1e-6); the mean angle between S and Rf grows
    with the roughness."""
    f = np.float32
    rng = np.random.default_rng(31)
    angles = {rho: [] for rho in (0.05, 0.25, 1.0)}
    lowest = 0.0
    for k, n, d in _face_hits(rng, 3000):
        pixel, sample, dim, seed = k * 7, k % 5, 2 + 16 * (k % 3), 99
        X = gloss_ref.bounce_direction(sref, n, pixel, sample, dim, seed)
        ln = np.sqrt(f(f(f(d[0] * d[0]) + f(d[1] * d[1])) + f(d[2] * d[2])))
        dh = np.array([d[0] / ln, d[1] / ln, d[2] / ln], f)
        two_d = f(f(2.0) * f(f(f(n[0] * dh[0]) + f(n[1] * dh[1])) + f(n[2] * dh[2])))
        rf = np.array([f(dh[i] - f(two_d * n[i])) for i in range(3)], f)
        for rough in gloss_common.ROUGHNESSES:
            rho = gloss_ref.roughness_of(rough)
            S, got_rf = gloss_ref.scatter(sref, n, d, rho, pixel, sample, dim, seed)
            assert got_rf.tobytes() == rf.tobytes(), k
            om = f(f(1.0) - rho)
            want = np.array([f(f(om * rf[i]) + f(rho * X[i])) for i in range(3)], f)
            if not f(f(f(want[0] * want[0]) + f(want[1] * want[1])) + f(want[2] * want[2])) > 0:
                want = rf
            assert S.tobytes() == want.tobytes(), (k, rough)
            if rough == 1.0:
                assert all(S[i] == X[i] for i in range(3)), k      # 0 * Rf is a zero: X's components (a zero of either sign is a zero)
            lowest = min(lowest, float(S.astype(np.float64) @ n.astype(np.float64)))
            if rough in angles:
                a, b = S.astype(np.float64), rf.astype(np.float64)
                angles[rough].append(np.arccos(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1.0, 1.0)))
    means = [float(np.mean(angles[r])) for r in (0.05, 0.25, 1.0)]
    print(f"gloss rule: lowest dot(S, n) {lowest:.3g}; mean angle to the reflection at rho 0.05 / 0.25 / 1: {means}")
    assert lowest >= -1e-6
    assert means[0] < means[1] < means[2]
    # the roughness the table keeps is a multiple of 2^-23 in [2^-10, 1]
    for rough in gloss_common.ROUGHNESSES + (0.3, 0.7):
        rho = float(gloss_ref.roughness_of(rough))
        assert rho * 2.0 ** 23 == int(rho * 2.0 ** 23) and abs(rho - rough) <= 2.0 ** -24 and 2.0 ** -10 <= rho <= 1.0


def test_a_vanishing_sum_gives_the_reflection(sref):
    """Step 5: NaN in, or S = 0, gives Rf.  (Rf = -X at rho = 0.5 cannot be met with a real hit; NaN can, from a NaN direction.)"""
    n = np.array([0.0, 0.0, 1.0], np.float32)
    d = np.array([np.nan, 0.0, -1.0], np.float32)
    S, rf = gloss_ref.scatter(sref, n, d, 0.25)
    assert np.isnan(rf).any() and S.tobytes() == rf.tobytes()


CASES = (3, 17, 29, 58)   # four cases of tests/path_cases.py: with mirrors, with shadows and sky, on instances


@pytest.mark.parametrize("i", CASES)
def test_without_gloss_it_is_the_glass_reference(sref, orc, ref_loader, cube, suzanne, i):
    """gloss_render_path with the case's table (no glossy record) equals glass_render_path byte for byte: every plane, every count."""
    c = path_cases.case(i, ref_loader, orc, cube, suzanne)
    kw = dict(instances=c["instances"], shadows=c["shadows"], sky=c["sky_colors"] if c["sky"] else None,
              mirror_parts=c["mirror_parts"] if c["mirrors"] else None, mirror_spheres=c["mirror_spheres"] if c["mirrors"] else None)
    args = (sref, orc, c["cam_inv"].view(orc.CAMERA_INV_DTYPE), orc.make_screen(c["w"], c["h"]),
            orc.make_params(c["spp"], c["bounces"], seed=c["seed"], flags=c["extra"] & path_cases.FLAG_NORMAL_MAP), c["spheres"].view(orc.SPHERE_DTYPE), c["model"])
    for rounded in (False, True):        # thr_unorm16 is passed through
        want = gloss_ref.render_path(*args, use_glass_ref=True, thr_unorm16=rounded, **kw)
        got = gloss_ref.render_path(*args, thr_unorm16=rounded, **kw)
        for k in PLANES:
            assert got[k].tobytes() == want[k].tobytes(), (i, k)
        for k in COUNTS:
            assert got[k] == want[k], (i, k)
        for k in ("gen_rays", "gen_mirror", "gen_glass"):
            assert np.array_equal(got[k], want[k]), (i, k)
        assert got["glossy"] == 0


@pytest.mark.parametrize("name", gloss_common.GPU_SCENES)
def test_the_scenes_exercise_the_gloss(rwr, orc, sref, ref_loader, suzanne, cube, name):
    """What tests/test_gpu_gloss.py relies on: every scene has glossy rays; from generation 2 on its ray count differs from the same
    scene with the glossy surfaces set as mirrors, so the comparison sees the rule (at B = 3 for every scene, the B = 1 one too);
    sample-0 planes and generation 1's ray count do not depend on the model."""
    s = gloss_common.scene(name, rwr, ref_loader, suzanne, cube)
    spp = 33 if name == "tiny" else 2
    on = gloss_common.reference(sref, rwr, orc, s, 13, spp, sky=DEFAULT, bounces=3, name=name)
    mir = gloss_common.reference(sref, rwr, orc, gloss_common.as_mirrors(s), 13, spp, sky=DEFAULT, bounces=3, name=name + " as mirrors")
    print(f"gloss scene {name}: glossy rays per generation {on['gen_gloss'][1:].tolist()}, rays {on['gen_rays'][1:].tolist()}, "
          f"as mirrors {mir['gen_rays'][1:].tolist()}")
    assert on["glossy"] > 0 and on["gen_gloss"][1] > 0 and mir["glossy"] == 0
    assert gloss_common.reference(sref, rwr, orc, s, 13, spp, sky=DEFAULT, name=name)["glossy"] > 0      # at the scene's own B
    for k in ("depth", "obj_id", "hit_t"):
        assert on[k].tobytes() == mir[k].tobytes(), (name, k)
    assert on["gen_rays"][1] == mir["gen_rays"][1]
    assert (on["gen_rays"][2:] != mir["gen_rays"][2:]).any(), name
    assert not np.array_equal(on["color_f32"], mir["color_f32"])
    assert s["w"] % 64 != 0 or s["h"] % 8 != 0      # no multiple of the 64 x 8 tile
    if name == "all_three":
        assert on["gen_mirror"].sum() > 0 and sum(on["events"]) > 0      # all three record kinds are met


def test_the_scenes_cover_the_roughnesses_and_depths(rwr, ref_loader, suzanne, cube):
    scenes = [gloss_common.scene(n, rwr, ref_loader, suzanne, cube) for n in gloss_common.GPU_SCENES]
    used = {r for s in scenes for items in (s["gloss_parts"], s["gloss_spheres"]) for r, _ in items.values()}
    assert used == set(gloss_common.ROUGHNESSES)
    assert {s["bounces"] for s in scenes} == {1, 3}
    assert (5, 3) in {(s["w"], s["h"]) for s in scenes} and (37, 29) in {(s["w"], s["h"]) for s in scenes} and (80, 56) in {(s["w"], s["h"]) for s in scenes}
