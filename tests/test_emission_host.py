"""Emissive surfaces (RWR_FLAG_EMISSIVE), host side: the public surface, the tests' CPU reference (emission_ref.c,
built on soft_shadow_ref.c and through it on the oracle) against soft_shadow_ref where both define the frame, and the conditions the
GPU file's scenes must meet - asserted here, not assumed.  No GPU."""
import os
import re

import numpy as np
import pytest

import emission_common
import emission_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
COUNTS = ("rays", "shadow_rays", "occluded", "sky_terms", "events", "glossy")
SPP = 3


@pytest.fixture(scope="module")
def eref(tmp_path_factory):
    return emission_ref.lib(tmp_path_factory)


def _ref(eref, rwr, orc, ref_loader, suzanne, cube, name, spp=SPP, **kw):
    s = emission_common.scene(name, rwr, ref_loader, suzanne, cube)
    return s, emission_common.reference(eref, rwr, orc, s, 13, spp, name, **kw)


def test_header_declares_and_library_exports_the_emission(rwr):
    text = open(os.path.join(ROOT, "include", "rwr_hip.h")).read()
    m = re.search(r"RWR_FLAG_EMISSIVE\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and int(m.group(1)) == 15
    bits = [int(v) for v in re.findall(r"RWR_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", text)]
    assert bits.count(15) == 1                                  # a bit nobody else has
    assert re.search(r"#define RWR_MAX_EMISSION 64\.0f", text)
    assert re.search(r"RWR_API int rwr_scene_set_part_emission\(rwr_context \*ctx, uint32_t part, const float \*radiance\);", text)
    assert re.search(r"RWR_API int rwr_scene_set_sphere_emission\(rwr_context \*ctx, uint32_t sphere, const float \*radiance\);", text)
    assert re.search(r"RWR_API int rwr_scene_get_part_emission\(rwr_context \*ctx, uint32_t part, int \*emits, float radiance\[3\]\);", text)
    assert re.search(r"RWR_API int rwr_scene_get_sphere_emission\(rwr_context \*ctx, uint32_t sphere, int \*emits, float radiance\[3\]\);", text)
    assert re.search(r"RWR_API int rwr_last_emission_stats\(rwr_context \*ctx, uint64_t \*emissive_hits\);", text)
    assert rwr.FLAG_EMISSIVE == 1 << 15 and rwr.MAX_EMISSION == 64.0
    declared = rwr.exported_symbols_declared_in_header()
    lib = rwr.lib()
    for name in ("rwr_scene_set_part_emission", "rwr_scene_set_sphere_emission", "rwr_scene_get_part_emission", "rwr_scene_get_sphere_emission",
                 "rwr_last_emission_stats"):
        assert name in declared and hasattr(lib, name), name
    for name in ("set_part_emission", "set_sphere_emission", "get_part_emission", "get_sphere_emission", "last_emission_stats"):
        assert hasattr(rwr.Context, name), name


@pytest.mark.parametrize("name", ("tiny", "two_parts", "spheres", "inside_sphere", "instances", "clamped"))
def test_emitters_are_seen_directly(rwr, orc, eref, ref_loader, suzanne, cube, name):
    s, r = _ref(eref, rwr, orc, ref_loader, suzanne, cube, name)
    assert r["gen_glow"][0] > 0, (name, r["gen_glow"].tolist())
    # h0's emitting hits at sample 0 are the id plane's pixels on an emitting surface
    one = emission_common.reference(eref, rwr, orc, s, 13, 1, name)
    n_parts = emission_common.n_parts(s)
    table = emission_ref.emission_table(n_parts, s["emissive_parts"], s["emissive_spheres"])
    emits = table[:, :3].any(axis=1)
    scene = orc.concat_parts(list(s["model"]) if isinstance(s["model"], (list, tuple)) else [s["model"]])
    fmat = np.asarray(scene["face_material"], np.int64)
    ids = one["obj_id"].astype(np.int64)
    rec = np.where(ids >= 0, fmat[np.clip(ids, 0, None) % len(fmat)], n_parts + (-2 - ids))
    assert one["gen_glow"][0] == int((emits[np.clip(rec, 0, len(emits) - 1)] & (ids != -1)).sum()), name


@pytest.mark.parametrize("name", ("room", "with_models", "instances", "clamped"))
def test_emitters_are_found_by_bounce_rays(rwr, orc, eref, ref_loader, suzanne, cube, name):
    _, r = _ref(eref, rwr, orc, ref_loader, suzanne, cube, name)
    assert r["gen_glow"][1:].sum() > 0, (name, r["gen_glow"].tolist())
    assert r["emissive_hits"] == r["gen_glow"].sum() == r["glow_by_surface"].sum()


def test_the_room_is_lit_by_its_lamp(rwr, orc, eref, ref_loader, suzanne, cube):
    """Pixels whose h0 does not emit are brighter in the mean than in the frame without the flag: the light came by bounce hits."""
    s, on = _ref(eref, rwr, orc, ref_loader, suzanne, cube, "room", spp=33)
    off = emission_common.reference(eref, rwr, orc, s, 13, 33, "room", emissive=False)
    elsewhere = (on["obj_id"] != -2) & (on["obj_id"] != -1)          # (sphere 0 is the lamp; the planes are the same in both frames)
    assert elsewhere.sum() > 100
    a, b = float(on["color_f32"][elsewhere][:, :3].mean()), float(off["color_f32"][elsewhere][:, :3].mean())
    print(f"room: mean radiance away from the lamp {b:.4f} -> {a:.4f}")
    assert a > b
    # no pixel got darker: Le >= 0 and nothing else moved
    assert (on["color_f32"] >= off["color_f32"]).all()


def test_an_emitter_in_shadow_keeps_its_light(rwr, orc, eref, ref_loader, suzanne, cube):
    s, r = _ref(eref, rwr, orc, ref_loader, suzanne, cube, "shadowed")
    assert s["shadows"] and r["glow_occluded"] > 0 and r["glow_occluded"] < r["emissive_hits"], (r["glow_occluded"], r["emissive_hits"])
    # an occluded h0 on the emitter shows ambient + Le: at one sample, exactly that
    one = emission_common.reference(eref, rwr, orc, s, 13, 1, "shadowed", bounces=0)
    scene = orc.concat_parts(list(s["model"]))
    fmat = np.asarray(scene["face_material"], np.int64)
    ids = one["obj_id"].astype(np.int64)
    dark = (one["occluded0"] != 0) & (ids >= 0)
    dark &= fmat[np.clip(ids, 0, None) % len(fmat)] == 1
    assert dark.sum() > 0
    amb = np.asarray(scene["materials"]["ambient"][1], np.float32)[:3]
    want = amb + np.asarray(s["emissive_parts"][1], np.float32)
    assert np.array_equal(one["color_f32"][dark][:, :3], np.broadcast_to(want, (int(dark.sum()), 3)))


@pytest.mark.parametrize("name", emission_common.SCENES)
def test_terms_reach_their_cap_in_the_clamped_scene_alone(rwr, orc, eref, ref_loader, suzanne, cube, name):
    _, r = _ref(eref, rwr, orc, ref_loader, suzanne, cube, name)
    if name == "clamped":
        assert r["capped"][0] > 0 and r["capped"][1] > 0, r["capped"]
        assert float(r["color_f32"][..., :3].max()) <= 16.0 + 64.0 * 2     # E0 <= 16, two later terms <= 64 each
    else:
        assert r["capped"] == (0, 0), (name, r["capped"])


def test_emission_stands_beside_every_model(rwr, orc, eref, ref_loader, suzanne, cube):
    """with_models: hits on the mirror part and on the glass sphere emit, and the rays those surfaces send on are the ones they sent."""
    s, r = _ref(eref, rwr, orc, ref_loader, suzanne, cube, "with_models")
    n_parts = emission_common.n_parts(s)
    assert s["mirror_parts"].keys() & s["emissive_parts"].keys() and s["glass_spheres"].keys() & s["emissive_spheres"].keys()
    assert r["glow_by_surface"][0] > 0 and r["glow_by_surface"][n_parts + 0] > 0, r["glow_by_surface"].tolist()
    off = emission_common.reference(eref, rwr, orc, s, 13, SPP, "with_models", emissive=False)
    for k in COUNTS + ("gen_rays", "gen_mirror", "gen_glass", "gen_gloss"):
        assert np.array_equal(r[k], off[k]), k
    assert r["gen_mirror"].sum() > 0 and r["gen_glass"].sum() > 0 and r["gen_gloss"].sum() > 0


@pytest.mark.parametrize("name", emission_common.SCENES)
def test_nothing_but_the_sums_moves(rwr, orc, eref, ref_loader, suzanne, cube, name):
    """The frame with emitters has the planes, rays and counts of the frame without; a zero table, and no table, give soft_render_path's
    bytes."""
    s, on = _ref(eref, rwr, orc, ref_loader, suzanne, cube, name)
    soft = emission_common.reference(eref, rwr, orc, s, 13, SPP, name, emissive=False, entry="soft")
    for k in ("depth", "obj_id", "hit_t", "occluded0", "primary"):
        assert on[k].tobytes() == soft[k].tobytes(), (name, k)
    for k in COUNTS + ("gen_rays", "gen_mirror", "gen_glass", "gen_gloss"):
        assert np.array_equal(on[k], soft[k]), (name, k)
    assert on["color_f32"].tobytes() != soft["color_f32"].tobytes(), name
    zero = emission_ref.emission_table(emission_common.n_parts(s))
    for what, kw in (("zero table", dict(table=zero)), ("no table", dict(emissive=False))):
        r = emission_common.reference(eref, rwr, orc, s, 13, SPP, name, **kw)
        for k in PLANES + ("occluded0", "primary"):
            assert r[k].tobytes() == soft[k].tobytes(), (name, what, k)
        for k in COUNTS + ("gen_rays",):
            assert np.array_equal(r[k], soft[k]), (name, what, k)
        assert r["emissive_hits"] == 0 and r["capped"] == (0, 0) and r["glow_occluded"] == 0, (name, what)


def test_a_sphere_that_is_not_in_use_lights_nothing(rwr, orc, eref, ref_loader, suzanne, cube):
    """An emission kept for a sphere index beyond the scene's count: the frame is the frame without the flag, also at spp 1 without a
    bounce (the unclamped reference frame)."""
    s = emission_common.scene("two_parts", rwr, ref_loader, suzanne, cube)
    table = emission_ref.emission_table(emission_common.n_parts(s), None, {3: (8.0, 8.0, 8.0)})
    for spp, bounces in ((1, 0), (2, 1)):
        r = emission_common.reference(eref, rwr, orc, s, 13, spp, "two_parts", bounces=bounces, table=table)
        soft = emission_common.reference(eref, rwr, orc, s, 13, spp, "two_parts", bounces=bounces, emissive=False, entry="soft")
        for k in PLANES:
            assert r[k].tobytes() == soft[k].tobytes(), (spp, k)
        assert r["emissive_hits"] == 0


def test_a_frame_with_an_emitter_is_the_integrators_at_one_sample(rwr, orc, eref, ref_loader, suzanne, cube):
    """tiny at spp 1, no bounce: E(h0) + Le, clamped to [0, 16] - the integrator's form, not the reference frame's."""
    s = emission_common.scene("tiny", rwr, ref_loader, suzanne, cube)
    on = emission_common.reference(eref, rwr, orc, s, 13, 1, "tiny")
    off = emission_common.reference(eref, rwr, orc, s, 13, 1, "tiny", emissive=False)
    hit = on["obj_id"] >= 0
    assert hit.any() and on["gen_glow"].tolist() == [int(hit.sum())]
    le = np.asarray(s["emissive_parts"][0], np.float32)
    want = np.clip(off["color_f32"][hit][:, :3] + le, 0.0, 16.0).astype(np.float32)
    assert np.array_equal(on["color_f32"][hit][:, :3], want)
