"""Light sampling (RWR_FLAG_LIGHT_SAMPLING), host side: the public surface, the tests' CPU reference (light_ref.c,
built on emission_ref.c and through it on the oracle) against emission_ref where both define the frame, the conditions the GPU
file's scenes must meet - asserted here, not assumed - and the estimator itself: unbiased, and less noisy.  No GPU."""
import os
import re

import numpy as np
import pytest

import emission_common as ec
import light_common as lc
import light_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
COUNTS = ("rays", "shadow_rays", "occluded", "sky_terms", "events", "glossy")
SPP = 3


@pytest.fixture(scope="module")
def lref(tmp_path_factory):
    return light_ref.lib(tmp_path_factory)


def _ref(lref, rwr, orc, ref_loader, suzanne, cube, name, spp=SPP, seed=13, **kw):
    s = lc.scene(name, rwr, ref_loader, suzanne, cube)
    return s, lc.reference(lref, rwr, orc, s, seed, spp, name, **kw)


def test_header_declares_and_library_exports_the_flag(rwr):
    text = open(os.path.join(ROOT, "include", "rwr_hip.h")).read()
    m = re.search(r"RWR_FLAG_LIGHT_SAMPLING\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and int(m.group(1)) == 16
    bits = [int(v) for v in re.findall(r"RWR_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", text)]
    assert bits.count(16) == 1                                  # a bit nobody else has
    assert re.search(r"RWR_API int rwr_last_light_stats\(rwr_context \*ctx, uint64_t \*light_rays, uint64_t \*reached, uint64_t \*suppressed_hits\);", text)
    assert "no next-event estimation" not in text
    assert rwr.FLAG_LIGHT_SAMPLING == 1 << 16
    assert "rwr_last_light_stats" in rwr.exported_symbols_declared_in_header() and hasattr(rwr.lib(), "rwr_last_light_stats")
    assert hasattr(rwr.Context, "last_light_stats")


# what each scene of the GPU parity test is there for: (light rays, reached, unreached, suppressed hits) that must not be zero
# (inside_sphere: every h0 lies on the lamp's inside and faces away from it; with_models: no surface is diffuse - the flag is in effect
# and traces nothing)
CLAIMS = {"room": (1, 1, 1, 1), "hidden": (1, 1, 1, 0), "two_lamps": (1, 1, 1, 1), "eight_lamps": (1, 1, 1, 1), "tiny": (1, 1, 0, 0),
          "far": (1, 1, 0, 0), "spheres": (1, 1, 0, 0), "inside_sphere": (0, 0, 0, 0), "lamp_around": (1, 1, 0, 0), "mirror_lamp": (1, 1, 1, 0),
          "with_models": (0, 0, 0, 0), "combo": (1, 1, 1, 1), "grid": (1, 1, 1, 1)}


@pytest.mark.parametrize("name", lc.SCENES)
def test_each_scene_shows_what_its_gpu_test_relies_on(rwr, orc, lref, ref_loader, suzanne, cube, name):
    s, r = _ref(lref, rwr, orc, ref_loader, suzanne, cube, name, spp=33 if name == "tiny" else SPP)
    got = (r["light_rays"], r["reached"], r["light_rays"] - r["reached"], r["suppressed"])
    print(f"light {name}: M {lc.n_lights(s)}, rays / reached / unreached / suppressed {got}, per generation {r['light_gen'].tolist()}, "
          f"emissive hits {r['gen_glow'].tolist()}")
    assert lc.n_lights(s) >= 1 and r["reached"] <= r["light_rays"]
    for claim, n in zip(CLAIMS[name], got):
        assert not claim or n > 0, (name, got)
    assert r["light_gen"][s["bounces"]][:2].tolist() == [0, 0] and r["light_gen"][0][2] == 0     # the last hit sends nothing on; h0 is no ray's hit


def test_the_hidden_lamp_is_hidden_from_part_of_the_floor(rwr, orc, lref, ref_loader, suzanne, cube):
    """hidden, one sample: h0's light rays are the samples with g > 0, fewer reach than are traced, and a pixel whose ray did not
    reach is no brighter than in the frame without the flag."""
    s, on = _ref(lref, rwr, orc, ref_loader, suzanne, cube, "hidden", spp=1, bounces=1, samples=True)
    off = lc.reference(lref, rwr, orc, s, 13, 1, "hidden", bounces=1, light=False)
    traced = on["light_samples"][:, :, 0, 0, 3] > 0.0
    assert on["light_gen"][0][0] == int(traced.sum()) > on["light_gen"][0][1] > 0
    lit = (on["color_f32"] > off["color_f32"]).any(axis=-1)      # (a silenced bounce hit makes a pixel darker, only a light term brighter)
    assert 0 < int(lit.sum()) <= on["light_gen"][0][1] and not (lit & ~traced).any()


def test_lanes_choose_their_own_sphere(rwr, orc, lref, ref_loader, suzanne, cube):
    """two_lamps, eight_lamps: g = 2 M kc (n . w) carries M, and among the pixels of one ballot word - 64 consecutive slots of a tile:
    a 32 x 2 block of pixels... here simply 32 neighbours of one row - the rays run towards different spheres."""
    for name, M in (("two_lamps", 2), ("eight_lamps", 8)):
        s, r = _ref(lref, rwr, orc, ref_loader, suzanne, cube, name, spp=1, bounces=1, samples=True)
        assert lc.n_lights(s) == M
        smp = r["light_samples"][:, :, 0, 0, :]
        centres = np.asarray([c["center"][:3] for c in s["spheres"]], np.float64)
        lamps = sorted(s["emissive_spheres"])
        mixed = 0
        for y in range(s["h"]):
            for x0 in range(0, s["w"] - 31, 32):
                row = smp[y, x0:x0 + 32]
                row = row[row[:, 3] > 0.0]
                if len(row) < 8:
                    continue
                # the sphere a ray runs towards: the emitter whose centre makes the smallest angle with it, seen from the scene's middle
                d = row[:, :3].astype(np.float64)
                d /= np.linalg.norm(d, axis=1)[:, None]
                c = centres[lamps] / np.linalg.norm(centres[lamps], axis=1)[:, None]
                mixed += len(set(np.argmax(d @ c.T, axis=1).tolist())) > 1
        assert mixed > 0, name


def test_a_hit_inside_an_emitting_sphere_takes_no_sample(rwr, orc, lref, ref_loader, suzanne, cube):
    """lamp_around: the eye and the cube's near corner lie inside the lamp.  There are mesh h0 whose ray origin O = P0 + 1e-4 n lies
    inside the sphere (|O - C| < R, from the reference's own O and the scene's C and R) and whose normal faces the centre
    (n . (C - O) > 0: the cosine test would have let a ray towards it through), and every such hit takes no sample: g == 0, no ray.
    Whatever did trace a ray started outside the sphere."""
    s, r = _ref(lref, rwr, orc, ref_loader, suzanne, cube, "lamp_around", spp=1, samples=True)
    c, R = np.asarray(s["spheres"][0]["center"][:3], np.float64), float(s["spheres"][0]["radius"])
    assert float(np.linalg.norm(np.asarray(s["eye"], np.float64) - c)) < R
    hits, g = r["light_hits"][:, :, 0, 0, :].astype(np.float64), r["light_samples"][:, :, 0, 0, 3]
    eligible = hits[..., 6] > 0
    mesh = (r["obj_id"] >= 0) & eligible
    O, n = hits[..., 0:3], hits[..., 3:6]
    dist = np.linalg.norm(O - c, axis=-1)
    facing = ((c - O) * n).sum(axis=-1) > 0.0
    inside = mesh & (dist < R * (1.0 - 1e-4)) & facing           # (a margin: the reference's own test is f32)
    later = r["light_hits"][:, :, 0, :, :].astype(np.float64).reshape(-1, 8)      # every generation's eligible hits
    g_all = r["light_samples"][:, :, 0, :, 3].reshape(-1)
    traced = later[:, 6] == 3.0
    dist_all = np.linalg.norm(later[:, 0:3] - c, axis=-1)
    print(f"lamp_around: {int(mesh.sum())} eligible mesh h0, {int(inside.sum())} inside the lamp and facing its centre; {int(traced.sum())} hits traced a ray")
    assert inside.sum() > 20
    assert (hits[..., 6][inside] == 1.0).all() and (g[inside] == 0.0).all()
    assert traced.any() and (dist_all[traced] > R).all() and (g_all[traced] > 0.0).all() and not (g_all[~traced] != 0.0).any()
    assert r["light_rays"] == int(traced.sum())


def test_a_mirror_rays_hit_on_the_lamp_keeps_le(rwr, orc, lref, ref_loader, suzanne, cube):
    """room has no mirror and its lamp is seen from outside only: every later hit on it is a diffuse ray's and is silenced.  In
    mirror_lamp the cube reflects: later hits on the lamp remain, the reflected rays', and silenced + kept hits are the frame's
    emissive hits without the flag."""
    for name in ("room", "mirror_lamp"):
        s, on = _ref(lref, rwr, orc, ref_loader, suzanne, cube, name, spp=33)
        off = _ref(lref, rwr, orc, ref_loader, suzanne, cube, name, spp=33, light=False)[1]
        print(f"{name}: emissive hits per generation with the flag {on['gen_glow'].tolist()}, without {off['gen_glow'].tolist()}, silenced {on['light_gen'][:, 2].tolist()}")
        assert np.array_equal(on["gen_glow"] + on["light_gen"][:, 2], off["gen_glow"]) and on["suppressed"] > 0
        assert on["gen_glow"][0] == off["gen_glow"][0]
        if name == "room":
            assert on["gen_glow"][1:].sum() == 0
        else:
            assert on["gen_mirror"].sum() > 0 and on["gen_glow"][1:].sum() > 0


@pytest.mark.parametrize("name", ("room", "two_lamps", "with_models", "mirror_lamp"))
def test_off_conditions_give_the_emission_frames_bytes(rwr, orc, lref, ref_loader, suzanne, cube, name):
    """Without the flag, without an emitting sphere in use, or at max_bounces 0: emission_render_path's bytes and counts."""
    s = lc.scene(name, rwr, ref_loader, suzanne, cube)
    cases = [("no flag", s, dict(light=False)), ("no bounce", s, dict(bounces=0)),
             ("no emitting sphere", dict(s, emissive_spheres={}, emissive_parts={0: (1.0, 2.0, 3.0)}), {}),
             ("an emitting sphere not in use", dict(s, emissive_spheres={7: (8.0, 8.0, 8.0)} if len(s["spheres"]) < 8 else {}, emissive_parts={0: (1.0, 2.0, 3.0)}), {})]
    for what, sc, kw in cases:
        got = lc.reference(lref, rwr, orc, sc, 13, SPP, f"{name} {what}", **kw)
        want = lc.reference(lref, rwr, orc, sc, 13, SPP, f"{name} {what}", entry="emission", **{k: v for k, v in kw.items() if k != "light"})
        for k in PLANES + ("occluded0", "primary"):
            assert got[k].tobytes() == want[k].tobytes(), (name, what, k)
        for k in COUNTS + ("gen_rays", "gen_glow", "emissive_hits"):
            assert np.array_equal(got[k], want[k]), (name, what, k)
        assert (got["light_rays"], got["reached"], got["suppressed"]) == (0, 0, 0), (name, what)


@pytest.mark.parametrize("name", lc.SCENES)
def test_no_existing_random_number_moves(rwr, orc, lref, ref_loader, suzanne, cube, name):
    """The id, depth and t planes, ray counts and shadow stats are the frame's without the flag - with soft shadows on, whose RNG
    blocks end where the light samples' begin."""
    s = lc.scene(name, rwr, ref_loader, suzanne, cube)
    kw = dict(shadows=True, radii=(0.05, 0.1))
    on = lc.reference(lref, rwr, orc, s, 13, SPP, name, **kw)
    off = lc.reference(lref, rwr, orc, s, 13, SPP, name, light=False, **kw)
    for k in ("depth", "obj_id", "hit_t", "occluded0", "primary"):
        assert on[k].tobytes() == off[k].tobytes(), (name, k)
    for k in COUNTS + ("gen_rays", "gen_mirror", "gen_glass", "gen_gloss"):
        assert np.array_equal(on[k], off[k]), (name, k)
    assert on["shadow_rays"] > 0 and (on["color_f32"].tobytes() != off["color_f32"].tobytes()) == (on["light_rays"] > 0)


def _mean(frames):
    return np.asarray([f["color_f32"][..., :3].reshape(-1, 3).mean(axis=0, dtype=np.float64) for f in frames])


def test_the_estimator_is_unbiased(rwr, orc, lref, ref_loader, suzanne, cube):
    """room: the frame mean per channel over 8 seeds with the flag against 8 seeds without it (disjoint seeds: independent frames).
    The two means differ by less than 4 standard errors of their difference, estimated from the 16 frames themselves."""
    s = lc.scene("room", rwr, ref_loader, suzanne, cube)
    spp = 48
    on = _mean([lc.reference(lref, rwr, orc, s, 100 + k, spp, "room") for k in range(8)])
    off = _mean([lc.reference(lref, rwr, orc, s, 200 + k, spp, "room", light=False) for k in range(8)])
    diff = on.mean(axis=0) - off.mean(axis=0)
    se = np.sqrt(on.var(axis=0, ddof=1) / 8.0 + off.var(axis=0, ddof=1) / 8.0)
    print(f"unbiased: mean with {on.mean(axis=0)}, without {off.mean(axis=0)}, difference {diff}, standard error {se}, ratio {np.abs(diff) / se}")
    assert (se > 0.0).all() and (np.abs(diff) < 4.0 * se).all(), (diff, se)


def test_the_frame_is_less_noisy(rwr, orc, lref, ref_loader, suzanne, cube):
    """room at 4 spp: the mean squared error against a many-sample frame made WITHOUT the flag, over the pixels of the floor and
    the cube, is lower with the flag than without it."""
    s = lc.scene("room", rwr, ref_loader, suzanne, cube)
    truth = lc.reference(lref, rwr, orc, s, 7, 2048, "room", light=False)
    on = lc.reference(lref, rwr, orc, s, 31, 4, "room")
    off = lc.reference(lref, rwr, orc, s, 31, 4, "room", light=False)
    mesh = truth["obj_id"] >= 0
    assert mesh.sum() > 500

    def mse(f):
        return float(((f["color_f32"][mesh][:, :3].astype(np.float64) - truth["color_f32"][mesh][:, :3].astype(np.float64)) ** 2).mean())

    a, b = mse(on), mse(off)
    print(f"less noise: MSE at 4 spp with the flag {a:.5g}, without {b:.5g}, ratio {a / b:.4f}")
    assert a < b
