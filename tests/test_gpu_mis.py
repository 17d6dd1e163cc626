"""Multiple importance sampling for the light rays (RWR_FLAG_LIGHT_MIS) on the GPU: k_wf_light's weighted terms and
add_glow's weighted hits against the tests' CPU reference (mis_ref.c):
  * sample-0 planes (object id, distance, depth) bit-exact and equal to the frame's without the flag; ray, shadow, glass and gloss
    counts equal to the reference's; the light stage's three counts, the mesh light's share of each and the emissive hits equal;
    RGBA8 within one code; colour within the bar tests/test_gpu_multi_bounce.py holds deeper paths to (COLOR_TOL there, read from
    that file) times max(1, the scene's largest Le component) - the largest value a term can take under the flag;
  * 32-bit traversal stacks beside nodelets in LDS; every schedule, accumulation, strips, row bands, frames in flight and the
    loopback gather: the same bytes;
  * frames the flag does nothing to, the keys, the refusals.
The scenes are tests/mis_common.py's; tests/test_mis_host.py asserts with the reference alone that they exercise the rule."""
import os
import re

import numpy as np
import pytest

import mis_common as mc
import mis_ref
import path_cases
import refusals_common

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# the colour bar of the deeper paths: not a tolerance of this file's own
COLOR_TOL = float(re.search(r"^COLOR_TOL\s*=\s*([0-9.eE+-]+)", open(os.path.join(HERE, "test_gpu_multi_bounce.py")).read(), re.M).group(1))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
COUNTS = ("stats", "shadow", "glass", "glossy")
MAX_SPHERES = mis_ref.MAX_SPHERES


@pytest.fixture(scope="module")
def mref(tmp_path_factory):
    return mis_ref.lib(tmp_path_factory)


def _plain_spheres(c):
    for i in range(MAX_SPHERES):
        c.set_sphere_gloss(i, 0.5, None)     # (any of the three model setters with None makes the surface diffuse)
        c.set_sphere_emission(i, None)


@pytest.fixture()
def ctx(gpu_ctx):
    """The shared context, left as it was found (test_gpu_part_light.py's fixture)."""
    gpu_ctx.sky_set_params()
    _plain_spheres(gpu_ctx)
    yield gpu_ctx
    gpu_ctx.sky_set_params()
    gpu_ctx.shadow_set_params(0.0, 0.0)
    _plain_spheres(gpu_ctx)
    gpu_ctx.set_instances(None)
    gpu_ctx.set_frames_in_flight(1)
    gpu_ctx.accum_reset()


def _upload(c, s, emitters=True):
    if isinstance(s["model"], (list, tuple)):
        c.upload_parts(s["model"])
    else:
        c.upload_model(s["model"])
    c.set_instances(s["instances"])
    c.set_spheres(s["spheres"])
    c.resize(s["w"], s["h"])
    _plain_spheres(c)
    for k, r in s["mirror_parts"].items():
        c.set_part_mirror(k, r)
    for k, (ior, tint) in s["glass_spheres"].items():
        c.set_sphere_glass(k, ior, tint)
    if emitters:
        for k, le in s["emissive_parts"].items():
            c.set_part_emission(k, le)
        for k, le in s["emissive_spheres"].items():
            c.set_sphere_emission(k, le)


def _frame(c, cam_inv, params, **kw):
    c.render(cam_inv, params, **kw)
    out = c.readback(aux=True)
    out["stats"] = c.last_render_stats()
    out["shadow"] = c.last_shadow_stats()
    out["glass"] = c.last_glass_stats()
    out["glossy"] = c.last_gloss_stats()
    out["emissive"] = c.last_emission_stats()
    out["light"] = c.last_light_stats()
    out["part"] = c.last_part_light_stats()
    out["plan"] = c.last_traversal_plan()
    return out


def _same(a, b, what=""):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _same_counts(a, b, what="", light=True):
    for k in COUNTS + (("emissive", "light", "part") if light else ()):
        assert a[k] == b[k], (what, k, a[k], b[k])


def _check(got, want, what, bar):
    """Planes bit for bit, colour within the bar, RGBA8 within one code; the counts exactly."""
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"mis colour error {what}: {err:.3g} (bar {bar:.3g}); light rays, reached, suppressed {got['light']} "
          f"(reference {(want['light_rays'], want['reached'], want['suppressed'])}), the mesh light's {got['part']} ({want['part_light']}), "
          f"emissive hits {got['emissive']} ({want['emissive_hits']})")
    assert got["light"] == (want["light_rays"], want["reached"], want["suppressed"]), (what, want["light_gen"].tolist())
    assert got["part"] == want["part_light"], (what, want["part_gen"].tolist())
    assert got["emissive"] == want["emissive_hits"], (what, want["gen_glow"].tolist())
    assert err <= bar, (what, err)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, what
    return err


def _params(rwr, s, spp, seed=13, mis=True, parts=None, light=None, emissive=True, bounces=None, extra=0):
    bounces = s["bounces"] if bounces is None else bounces
    return rwr.make_params(spp=spp, max_bounces=bounces, seed=seed,
                           flags=mc.flags(rwr, s, bounces=bounces, mis=mis, parts=parts, light=light, emissive=emissive, extra=extra))


@pytest.mark.parametrize("name,spp", [(n, k) for n in mc.SCENES for k in mc.spps(n)])
def test_matches_the_reference(rwr, orc, mref, ctx, ref_loader, suzanne, cube, name, spp):
    s = mc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    cam_inv = mc.camera(rwr, s)
    _upload(ctx, s)
    got = _frame(ctx, cam_inv, _params(rwr, s, spp))
    want = mc.reference(mref, rwr, orc, s, 13, spp, name)
    assert got["stats"] == (s["w"] * s["h"] * spp, want["rays"]), (name, spp, want["gen_rays"].tolist())
    assert got["glass"] == want["events"] and got["glossy"] == want["glossy"], (name, spp)
    assert got["shadow"] == (want["shadow_rays"], want["occluded"]), (name, spp)
    _check(got, want, f"{name} spp={spp}", COLOR_TOL * mc.bar_factor(s))
    # nothing but the sums moves: the same context's frame without the flag has the planes, the counts and the traversal plan
    off = _frame(ctx, cam_inv, _params(rwr, s, spp, mis=False))
    for k in ("obj_id", "hit_t", "depth"):
        assert got[k].tobytes() == off[k].tobytes(), (name, k)
    _same_counts(got, off, (name, spp), light=False)
    assert got["plan"] == off["plan"] and off["light"] == got["light"] and off["part"] == got["part"]
    assert off["emissive"] + want["mis"][3] == got["emissive"]
    assert (got["color_f32"].tobytes() != off["color_f32"].tobytes()) == (got["light"][0] + got["light"][2] > 0)
    if name == "grid":          # nodelets out of LDS
        assert got["plan"]["trace"]["launches"] > 0 and got["plan"]["trace"]["nodes_in_lds"] == 0 and got["plan"]["trace"]["stack16"] == 1, got["plan"]
    if name == "large":         # above 4 095 world faces: 32-bit stacks chosen by the plan
        assert got["plan"]["trace"]["launches"] > 0 and got["plan"]["trace"]["stack16"] == 0, got["plan"]


def _with_env(rwr, env, s, cam_inv, params):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with rwr.Context(0) as c:        # the tunables are read when the context is created
            _upload(c, s)
            return _frame(c, cam_inv, params)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("name", ("bare_panel", "bare_lamp"))
def test_32_bit_stacks_beside_nodelets_in_lds(rwr, orc, mref, ctx, ref_loader, suzanne, cube, name):
    """k_wf_light's form with nodelets in LDS and 32-bit stacks, for both values of PARTS, and the trace kernels' beside it, under the
    flag: a context created under RWR_WF_STACK16=0 gives the 16-bit run's bytes and counts, which the reference vouches for."""
    s = mc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    params = _params(rwr, s, 33)
    want = mc.reference(mref, rwr, orc, s, 13, 33, name)
    assert want["light_rays"] > want["reached"] > 0 and want["suppressed"] > 0 and want["mis"][3] > 0
    cam_inv = mc.camera(rwr, s)
    _upload(ctx, s)
    got = _frame(ctx, cam_inv, params)
    _check(got, want, f"{name} 16-bit stacks", COLOR_TOL * mc.bar_factor(s))
    assert got["light"][1] > 0 and (got["part"][0] > 0) == s["parts"]
    assert got["plan"]["trace"]["launches"] > 0 and got["plan"]["trace"]["nodes_in_lds"] == 1 and got["plan"]["trace"]["stack16"] == 1, got["plan"]
    wide = _with_env(rwr, {"RWR_WF_STACK16": "0", "RWR_WF_WIDE_LANE": "0"}, s, cam_inv, params)
    assert wide["plan"]["trace"]["launches"] > 0 and wide["plan"]["trace"]["nodes_in_lds"] == 1 and wide["plan"]["trace"]["stack16"] == 0, wide["plan"]
    assert wide["plan"]["trace"]["wide"] == 0
    _same(wide, got, "32-bit stacks")
    _same_counts(wide, got, "32-bit stacks")


def test_the_cleared_flag_gives_the_frame_without_it(rwr, ctx, ref_loader, suzanne, cube, orc):
    """The flag with neither light flag effective - not asked for, at max_bounces 0, without RWR_FLAG_EMISSIVE, without an emitter:
    the bytes, the counts and the traversal plan of the frame without it."""
    for name in ("panel", "panel_and_lamp"):
        s = mc.scene(name, rwr, ref_loader, suzanne, cube, orc)
        cam_inv = mc.camera(rwr, s)
        _upload(ctx, s)
        lit = _frame(ctx, cam_inv, _params(rwr, s, 2, seed=5))
        plain = _frame(ctx, cam_inv, _params(rwr, s, 2, seed=5, mis=False))
        assert lit["light"][0] > 0 and lit["color_f32"].tobytes() != plain["color_f32"].tobytes()

        def nothing(what, **kw):
            for spp, b, x in ((33, None, 0), (2, 1, rwr.FLAG_SHADOWS)) if "bounces" not in kw else ((2, 0, 0), (1, 0, rwr.FLAG_SHADOWS)):
                args = dict(dict(bounces=b, extra=x), **{k: v for k, v in kw.items() if k != "bounces"})
                want = _frame(ctx, cam_inv, _params(rwr, s, spp, seed=5, mis=False, **args))
                got = _frame(ctx, cam_inv, _params(rwr, s, spp, seed=5, **args))
                _same(got, want, (name, what, spp, b, x))
                _same_counts(got, want, (name, what, spp, b, x))
                assert got["plan"] == want["plan"]
                if what != "no emitter left to aim at":
                    assert got["light"] == (0, 0, 0)

        nothing("neither light flag", parts=False, light=False)
        nothing("no bounce", bounces=0)
        nothing("no RWR_FLAG_EMISSIVE", emissive=False)
        for k in s["emissive_parts"]:
            ctx.set_part_emission(k, None)
        for k in s["emissive_spheres"]:
            ctx.set_sphere_emission(k, None)
        nothing("no emitter")
        ctx.set_part_emission(0, (1.0, 2.0, 3.0))         # the room emits, but only RWR_FLAG_LIGHT_SAMPLING is asked for: no sphere to aim at
        nothing("no emitter left to aim at", parts=False, light=True)
        ctx.set_part_emission(0, None)
        for k, le in s["emissive_parts"].items():
            ctx.set_part_emission(k, le)
        for k, le in s["emissive_spheres"].items():
            ctx.set_sphere_emission(k, le)
        again = _frame(ctx, cam_inv, _params(rwr, s, 2, seed=5))
        _same(again, lit, "the emission set again")
        _same_counts(again, lit, "the emission set again")


_STATS = re.compile(r"rwr wavefront pools: packets (\d+) pools / (\d+) rays, per-lane (\d+) pools / (\d+) rays.*\n"
                    r"rwr wavefront launches: packet (\d+), per-lane (\d+), per-lane wide (\d+)")
_LANE = {"RWR_WF_GROUP": "5", "RWR_WF_PACKET_RAYS": "0", "RWR_WF_MIN_PACKET_POOLS": "100000"}
SCHEDULES = {"packets": dict(path_cases.FORCED_SCHEDULE, RWR_WF_WIDE_LANE="0"),
             "per lane": dict(_LANE, RWR_WF_WIDE_LANE="0"),
             "wide lane": dict(_LANE, RWR_WF_WIDE_LANE="1"),
             "live list": {"RWR_WF_ZSPLIT": "2"}}


def test_schedules_give_the_same_frame(rwr, orc, mref, ctx, ref_loader, suzanne, cube, capfd):
    """Forced packets, the per-lane kernel alone, its wide form and the live-tile list on panel_and_lamp (all three flags, shadow rays
    on): the default schedule's bytes and counts - add_glow's weighted branch in both trace kernels."""
    name = "panel_and_lamp"
    s = mc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    cam_inv = mc.camera(rwr, s)
    spp = 33
    params = _params(rwr, s, spp, extra=rwr.FLAG_SHADOWS)
    _upload(ctx, s)
    default = _frame(ctx, cam_inv, params)
    want = mc.reference(mref, rwr, orc, s, 13, spp, name, shadows=True)
    _check(default, want, f"schedule {name} default", COLOR_TOL * mc.bar_factor(s))
    assert default["stats"][1] == want["rays"] and default["light"][0] > default["part"][0] > default["part"][1] > 0
    assert default["light"][2] > default["part"][2] > 0 and want["mis"][0] > 0 and want["mis"][1] > 0
    assert default["shadow"] == (want["shadow_rays"], want["occluded"])
    keys = sorted({k for env in SCHEDULES.values() for k in env} | {"RWR_WF_STATS"})
    for what, env in SCHEDULES.items():
        full = {k: "" for k in keys}
        full.update(env, RWR_WF_STATS="1")
        capfd.readouterr()
        saved = {k: os.environ.get(k) for k in keys}
        try:
            for k in keys:
                os.environ.pop(k, None)
            os.environ.update({k: v for k, v in full.items() if v != ""})
            with rwr.Context(0) as c:
                _upload(c, s)
                got = _frame(c, cam_inv, params)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        _same(got, default, (name, what))
        _same_counts(got, default, (name, what))
        m = _STATS.search(capfd.readouterr().err)
        assert m, (name, what)
        p_pools, p_rays, l_pools, l_rays, n_packet, n_lane, n_wide = map(int, m.groups())
        assert p_rays + l_rays == got["stats"][1], (name, what)     # every bounce ray went through a pool
        if what == "packets":
            assert n_packet > 0 and p_pools > 0, (name, what)
        elif what in ("per lane", "wide lane"):
            assert p_pools == 0 and n_lane + n_wide > 0 and (n_lane == 0 or n_wide == 0), (name, what)


@pytest.mark.parametrize("name", ("panel", "panel_two_lamps", "big_lamp", "tiny"))
def test_accumulated_frames_are_one_frame_of_all_samples(rwr, ctx, ref_loader, suzanne, cube, orc, name):
    s = mc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    cam_inv = mc.camera(rwr, s)
    _upload(ctx, s)
    want = _frame(ctx, cam_inv, _params(rwr, s, 2, seed=11))
    ctx.accum_reset()
    acc = _params(rwr, s, 1, seed=11, extra=rwr.FLAG_ACCUMULATE)      # (an accumulating frame's samples are placed by the RNG at spp 1 too)
    counts, share, hits = np.zeros(3, np.int64), np.zeros(3, np.int64), 0
    for k in range(1, 3):
        ctx.render(cam_inv, acc)
        assert ctx.accum_samples() == k
        counts += np.asarray(ctx.last_light_stats())      # (an accumulating frame counts its own samples)
        share += np.asarray(ctx.last_part_light_stats())
        hits += ctx.last_emission_stats()
    _same(ctx.readback(aux=True), want, "2 x 1 spp")
    assert tuple(counts.tolist()) == want["light"] and tuple(share.tolist()) == want["part"] and want["light"][0] > 0 and hits == want["emissive"]


@pytest.mark.parametrize("name", ("panel", "panel_and_lamp"))
def test_strips_bands_and_frames_in_flight(rwr, ctx, ref_loader, suzanne, cube, orc, name):
    """Strips of two ranks (the loopback gather for N = 2) and two row bands assemble the frame (planes, counts); 1 to 3 frames in
    flight give its bytes."""
    s = mc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    h = s["h"]
    cam_inv = mc.camera(rwr, s)
    params = _params(rwr, s, 2, seed=2, extra=rwr.FLAG_SHADOWS)
    _upload(ctx, s)
    full = _frame(ctx, cam_inv, params)
    assert full["part"][0] > 0 and full["light"][2] > 0
    asm = {k: np.zeros_like(full[k]) for k in PLANES}
    rays, light, share, hits = 0, np.zeros(3, np.int64), np.zeros(3, np.int64), 0
    for r in range(2):
        part = _frame(ctx, cam_inv, params, strips=(r, 2))
        rows = [y for y in range(h) if (y // 8) % 2 == r]
        rays += part["stats"][1]
        light += np.asarray(part["light"])
        share += np.asarray(part["part"])
        hits += part["emissive"]
        for k in PLANES:
            asm[k][rows] = part[k][rows]
        ctx.dist_loopback_deposit(r, 2, True)
    ctx.dist_loopback_finish(2, True)
    _same(asm, full, (name, "strips"))
    assert rays == full["stats"][1] and tuple(light.tolist()) == full["light"] and tuple(share.tolist()) == full["part"] and hits == full["emissive"]
    assert np.array_equal(ctx.dist_readback(), full["color"]), name
    asm = {k: np.zeros_like(full[k]) for k in PLANES}
    light = np.zeros(3, np.int64)
    for band in ((0, 16), (16, h)):
        part = _frame(ctx, cam_inv, params, rows=band)
        light += np.asarray(part["light"])
        for k in PLANES:
            asm[k][band[0]:band[1]] = part[k][band[0]:band[1]]
    _same(asm, full, (name, "bands"))
    assert tuple(light.tolist()) == full["light"]
    for n in (1, 2, 3):
        ctx.set_frames_in_flight(n)
        for i in range(n + 1):
            got = _frame(ctx, cam_inv, params)
            _same(got, full, (name, n, i))
            _same_counts(got, full, (name, n, i))


def test_the_flag_is_part_of_both_keys(rwr, ctx, ref_loader, suzanne, cube, orc):
    s = mc.scene("two_parts", rwr, ref_loader, suzanne, cube, orc)
    cam_inv = mc.camera(rwr, s)
    _upload(ctx, s)
    acc = _params(rwr, s, 2, seed=11, extra=rwr.FLAG_ACCUMULATE)
    off = _params(rwr, s, 2, seed=11, mis=False, extra=rwr.FLAG_ACCUMULATE)
    rep, rep_off = _params(rwr, s, 2, seed=11, extra=rwr.FLAG_REPROJECT), _params(rwr, s, 2, seed=11, mis=False, extra=rwr.FLAG_REPROJECT)

    def step(params=acc):
        ctx.render(cam_inv, params)
        return ctx.accum_samples()

    def history(params=rep):
        ctx.render(cam_inv, params)
        return ctx.reproject_frames()

    ctx.accum_reset()
    assert step() == 2 and step() == 4
    assert step(off) == 2 and step(off) == 4                    # the flag toggled: its bit is part of the key ...
    assert step() == 2 and step() == 4                          # ... and back
    ctx.set_part_emission(2, None)                              # a part's emission changed: the list, W and every inv_pdf with it
    assert step() == 2 and ctx.last_light_stats()[2] > 0 and step() == 4
    ctx.set_part_emission(2, (1.0, 1.0, 1.0))
    assert step() == 2 and step() == 4
    assert history() == 1 and history() == 2
    assert history(rep_off) == 1 and history(rep_off) == 2
    assert history() == 1 and history() == 2
    # the flag the frame clears is not part of a key: with neither light flag, or at max_bounces 0, the accumulation goes on across it
    for kw in (dict(parts=False, light=False), dict(bounces=0)):
        flat, flat_off = _params(rwr, s, 2, seed=11, extra=rwr.FLAG_ACCUMULATE, **kw), _params(rwr, s, 2, seed=11, mis=False, extra=rwr.FLAG_ACCUMULATE, **kw)
        ctx.accum_reset()
        assert step(flat) == 2 and step(flat_off) == 4 and step(flat) == 6


def test_a_changed_mesh_light_changes_the_weights(rwr, orc, mref, ctx, ref_loader, suzanne, cube):
    """two_parts, then part 2's emission removed and set again: every inv_pdf changes with W, and the frame is the reference's of the
    scene as it then is - the emission table's copy of inv_pdf follows the list."""
    s = mc.scene("two_parts", rwr, ref_loader, suzanne, cube, orc)
    cam_inv = mc.camera(rwr, s)
    _upload(ctx, s)
    first = _frame(ctx, cam_inv, _params(rwr, s, 2))
    ctx.set_part_emission(2, None)
    one = dict(s, emissive_parts={1: s["emissive_parts"][1]})
    got = _frame(ctx, cam_inv, _params(rwr, s, 2))
    _check(got, mc.reference(mref, rwr, orc, one, 13, 2, "two_parts, one left"), "two_parts, one left", COLOR_TOL * mc.bar_factor(one))
    ctx.set_part_emission(2, s["emissive_parts"][2])
    again = _frame(ctx, cam_inv, _params(rwr, s, 2))
    _same(again, first, "set again")
    _same_counts(again, first, "set again")


def test_refusals(rwr, ctx, ref_loader, suzanne, cube, orc):
    """RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes refuse the flag - the code and the message - whatever
    max_bounces is and whether or not anything emits."""
    s = mc.scene("panel", rwr, ref_loader, suzanne, cube, orc)
    cam_inv = mc.camera(rwr, s)
    _upload(ctx, s)
    text = refusals_common.OFF_REFERENCE % "LIGHT_MIS"
    for emitters in (True, False):
        if not emitters:
            ctx.set_part_emission(1, None)
        for params in (rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_LIGHT_MIS | rwr.FLAG_ORTHO_RAYS),
                       rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_LIGHT_MIS | rwr.FLAG_USE_BVH),
                       rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_LIGHT_MIS | rwr.FLAG_ORTHO_RAYS)):
            with pytest.raises(rwr.RwrError) as ei:
                ctx.render(cam_inv, params)
            assert ei.value.code == rwr.ERR_UNSUPPORTED and text in str(ei.value), (params, str(ei.value))
        ctx.set_triangles(rwr.make_triangles([((0.0, 0.0, -2.0), (1.0, 0.0, -2.0), (0.0, 1.0, -2.0))]))
        try:
            for bounces in (0, 1):
                with pytest.raises(rwr.RwrError) as ei:
                    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=bounces, flags=rwr.FLAG_LIGHT_MIS))
                assert ei.value.code == rwr.ERR_UNSUPPORTED and text in str(ei.value), str(ei.value)
        finally:
            ctx.set_triangles(rwr.make_triangles())
    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=1, flags=rwr.FLAG_LIGHT_MIS | rwr.FLAG_EMISSIVE))   # the context is still usable
