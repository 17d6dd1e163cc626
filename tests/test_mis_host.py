"""Multiple importance sampling for the light rays (RWR_FLAG_LIGHT_MIS), host side: the public surface, the weight at
its ends, the tests' CPU reference (mis_ref.c, built on part_light_ref.c) against part_light_ref where both define the frame, the
conditions the GPU file's scenes must meet - asserted here, not assumed - and the estimator itself: unbiased where the light flags
alone are not, and less noisy.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import mis_common as mc
import mis_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
COUNTS = ("rays", "shadow_rays", "occluded", "sky_terms", "events", "glossy")
SPP = 3


@pytest.fixture(scope="module")
def mref(tmp_path_factory):
    return mis_ref.lib(tmp_path_factory)


def test_header_declares_the_flag(rwr):
    text = open(os.path.join(ROOT, "include", "rwr_hip.h")).read()
    m = re.search(r"RWR_FLAG_LIGHT_MIS\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and int(m.group(1)) == 22
    bits = [int(v) for v in re.findall(r"RWR_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", text)]
    assert bits.count(22) == 1 and not set(bits) & {17, 18, 19, 20}           # a bit nobody else has, and no internal one
    public = re.search(r"#define RWR_FLAGS_PUBLIC \((.*)\)\s*$", text, re.M).group(1)
    assert eval(public.replace("u", "")) & (1 << 22) and not eval(public.replace("u", "")) & (0xf << 17)
    assert "There is no multiple importance sampling" not in text
    for doc in ("README.md", "DESIGN.md"):
        assert "RWR_FLAG_LIGHT_MIS" in open(os.path.join(ROOT, doc)).read(), doc
    assert rwr.FLAG_LIGHT_MIS == 1 << 22 and rwr.FLAG_LIGHT_PARTS == 1 << 21 and rwr.FLAG_DEBUG_COUNTS == 1 << 20


def test_the_weight_at_its_ends(mref):
    """m(g) = g / (1 + g) in the form 1 / (1 + 1 / g): 0 for g <= 0 and NaN, 0 for a denormal g, exactly 1 for g = inf, and the f32
    operations of the header in between."""
    w = lambda g: mis_ref.weight(mref, g)
    assert w(0.0) == 0.0 and w(-0.0) == 0.0 and w(-3.0) == 0.0 and w(-math.inf) == 0.0
    assert w(math.nan) == 0.0
    assert w(1e-45) == 0.0 and w(1e-39) == 0.0          # denormals: 1 / g overflows to inf, 1 / inf is 0
    assert w(math.inf) == 1.0
    assert w(1.0) == 0.5 and w(3.0) == 0.75
    f = np.float32
    for g in (1e-30, 1e-7, 0.3, 0.9999, 7.0, 123.456, 1e9, 3e38):
        want = f(1.0) / (f(1.0) + f(1.0) / f(g))
        assert w(g) == float(want) and 0.0 <= w(g) <= 1.0, g
    assert w(3e38) == 1.0 and 0.0 < w(1e-30) < 1e-29


@pytest.mark.parametrize("name", mc.SCENES)
def test_without_the_flag_it_is_part_light_refs_frame(rwr, orc, mref, ref_loader, suzanne, cube, name):
    """mis_render_path without the new flag is part_light_render_path: planes and counts."""
    s = mc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    spp = 1 if name in ("grid", "large") else SPP
    got = mc.reference(mref, rwr, orc, s, 13, spp, name, mis=False)
    want = mc.reference(mref, rwr, orc, s, 13, spp, name, entry="parts")
    for k in PLANES + ("occluded0", "primary"):
        assert got[k].tobytes() == want[k].tobytes(), (name, k)
    for k in COUNTS + ("gen_rays", "gen_glow", "emissive_hits", "light_gen", "part_gen", "light_capped", "light_rays", "reached", "suppressed"):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert got["mis"][0] == got["mis"][1] == got["mis"][3] == 0


def _spp(name):
    return 33 if name == "tiny" else mc.spps(name)[-1] if name in ("grid", "large") else SPP


@pytest.mark.parametrize("name", mc.SCENES)
def test_each_scene_shows_what_its_gpu_test_relies_on(rwr, orc, mref, ref_loader, suzanne, cube, name):
    """Weighted hits occur in every scene; the rays, reached and suppressed counts, the planes and the ray counts are those of the
    frame without the flag; no light term is at the cap under the flag."""
    s = mc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    spp = _spp(name)
    r = mc.reference(mref, rwr, orc, s, 13, spp, name)
    off = mc.reference(mref, rwr, orc, s, 13, spp, name, mis=False)
    w_sphere, w_face, inside, nonzero = r["mis"]
    print(f"mis {name}: weighted sphere / face hits {w_sphere} / {w_face} ({nonzero} not zero), from inside {inside}, light rays, reached, suppressed "
          f"{(r['light_rays'], r['reached'], r['suppressed'])}, capped light terms {r['light_capped']} (without the flag {off['light_capped']}), "
          f"emissive hits {r['gen_glow'].tolist()} (without {off['gen_glow'].tolist()})")
    assert w_sphere + w_face > 0 and nonzero > 0, name
    assert w_sphere + w_face == r["suppressed"] and w_face == r["part_light"][2]
    assert r["light_capped"] == 0, name
    for k in ("depth", "obj_id", "hit_t"):
        assert r[k].tobytes() == off[k].tobytes(), (name, k)
    for k in COUNTS + ("gen_rays", "light_gen", "part_gen", "light_rays", "reached", "suppressed", "part_light"):
        assert np.array_equal(r[k], off[k]), (name, k)
    assert r["emissive_hits"] == off["emissive_hits"] + nonzero
    assert r["color_f32"].tobytes() != off["color_f32"].tobytes()
    if name == "panel_and_lamp":
        assert w_sphere > 0 and w_face > 0
    if name == "inside":
        assert inside > 0
    if name == "parts_only":        # the sphere is not sampled: its hits keep Le and no sphere weight occurs
        assert w_sphere == 0 and r["glow_by_surface"][mc.n_parts(s)] > 0
    if name == "crease":            # the case the parts flag alone darkens: terms at the cap without the weight
        assert off["light_capped"] > 0


def test_off_conditions_give_the_frame_without_the_flag(rwr, orc, mref, ref_loader, suzanne, cube):
    """Neither light flag, no bounce, or nothing that emits: part_light_render_path's bytes and counts."""
    s = mc.scene("panel_and_lamp", rwr, ref_loader, suzanne, cube, orc)
    cases = [("neither light flag", s, dict(parts=False, light=False)), ("no bounce", s, dict(bounces=0)),
             ("no emitter", dict(s, emissive_parts={}, emissive_spheres={}), {})]
    for what, sc, kw in cases:
        got = mc.reference(mref, rwr, orc, sc, 13, SPP, f"off {what}", **kw)
        want = mc.reference(mref, rwr, orc, sc, 13, SPP, f"off {what}", entry="parts", **kw)
        for k in PLANES:
            assert got[k].tobytes() == want[k].tobytes(), (what, k)
        for k in COUNTS + ("gen_rays", "gen_glow", "emissive_hits", "light_gen", "part_gen"):
            assert np.array_equal(got[k], want[k]), (what, k)
        assert got["mis"][:2] == (0, 0) and got["mis"][3] == 0, what


def _mean(frames):
    return np.asarray([f["color_f32"][..., :3].reshape(-1, 3).mean(axis=0, dtype=np.float64) for f in frames])


@pytest.mark.parametrize("name", ("panel", "crease", "big_lamp"))
def test_the_estimator_is_unbiased(rwr, orc, mref, ref_loader, suzanne, cube, name):
    """The frame mean per channel over 8 seeds with the flag against 8 seeds of plain RWR_FLAG_EMISSIVE frames (disjoint seeds:
    independent frames): the two means differ by less than 4 standard errors of their difference, estimated from the 16 frames
    themselves - test_light_host.py's bar.  No precondition on capped terms: under the flag there are none, `crease` included."""
    s = mc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    spp = 48
    frames = [mc.reference(mref, rwr, orc, s, 100 + k, spp, name) for k in range(8)]
    assert sum(f["light_capped"] for f in frames) == 0 and all(f["reached"] > 0 and f["mis"][3] > 0 for f in frames)
    on = _mean(frames)
    off = _mean([mc.reference(mref, rwr, orc, s, 200 + k, spp, name, mis=False, parts=False, light=False) for k in range(8)])
    diff = on.mean(axis=0) - off.mean(axis=0)
    se = np.sqrt(on.var(axis=0, ddof=1) / 8.0 + off.var(axis=0, ddof=1) / 8.0)
    print(f"unbiased {name}: mean with {on.mean(axis=0)}, plain {off.mean(axis=0)}, difference {diff}, standard error {se}, ratio {np.abs(diff) / se}")
    assert (se > 0.0).all() and (np.abs(diff) < 4.0 * se).all(), (diff, se)


def _mses(rwr, orc, mref, ref_loader, suzanne, cube, name):
    """MSE at 4 spp against a 2 048-sample plain frame over the pixels that show a face of a part that does not emit - the receivers:
    (with the flag, the light flags alone, plain)."""
    s = mc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    truth = mc.reference(mref, rwr, orc, s, 7, 2048, name, mis=False, parts=False, light=False)
    parts = s["model"] if isinstance(s["model"], (list, tuple)) else [s["model"]]
    ends = np.cumsum([len(p["faces"]) for p in parts])
    mesh = np.zeros(truth["obj_id"].shape, bool)
    for k, end in enumerate(ends):
        if k not in s["emissive_parts"]:
            mesh |= (truth["obj_id"] >= end - len(parts[k]["faces"])) & (truth["obj_id"] < end)
    assert mesh.sum() > 500

    def mse(f):
        return float(((f["color_f32"][mesh][:, :3].astype(np.float64) - truth["color_f32"][mesh][:, :3].astype(np.float64)) ** 2).mean())

    return (mse(mc.reference(mref, rwr, orc, s, 31, 4, name)), mse(mc.reference(mref, rwr, orc, s, 31, 4, name, mis=False)),
            mse(mc.reference(mref, rwr, orc, s, 31, 4, name, mis=False, parts=False, light=False)))


@pytest.mark.parametrize("name", ("glow_cube", "crease"))
def test_less_noisy_than_the_light_flags_alone(rwr, orc, mref, ref_loader, suzanne, cube, name):
    a, b, c = _mses(rwr, orc, mref, ref_loader, suzanne, cube, name)
    print(f"less noise {name}: MSE at 4 spp with the flag {a:.5g}, the light flags alone {b:.5g}, plain {c:.5g}; ratio to the light flags alone {a / b:.4f}")
    assert a < b


@pytest.mark.parametrize("name", ("panel", "big_lamp"))
def test_less_noisy_than_the_plain_frame(rwr, orc, mref, ref_loader, suzanne, cube, name):
    a, b, c = _mses(rwr, orc, mref, ref_loader, suzanne, cube, name)
    print(f"less noise {name}: MSE at 4 spp with the flag {a:.5g}, the light flags alone {b:.5g}, plain {c:.5g}; ratio to the plain frame {a / c:.4f}")
    assert a < c
