"""Light sampling towards emitting mesh parts (RWR_FLAG_LIGHT_PARTS) on the GPU: k_wf_light's PARTS forms, the table the
library builds and uploads, and add_glow's silenced faces, against the tests' CPU reference (part_light_ref.c):
  * sample-0 planes (object id, distance, depth) bit-exact and equal to the frame's without the flag; ray, shadow, glass and gloss
    counts equal to the reference's; the light stage's three counts, the mesh light's share of each and the emissive hits equal;
    RGBA8 within one code; colour within the bar tests/test_gpu_multi_bounce.py holds deeper paths to (COLOR_TOL there, read from
    that file) times 64 - a frame with the mesh light: g is bounded by the term's cap alone;
  * 32-bit traversal stacks beside nodelets in LDS, for both values of PARTS; every schedule, accumulation, strips, row bands, frames
    in flight and the loopback gather: the same bytes;
  * frames the flag does nothing to, RWR_FLAG_LIGHT_SAMPLING without it, the keys, the refusals.
The scenes are tests/part_light_common.py's; tests/test_part_light_host.py asserts with the reference alone that they exercise the rule."""
import os
import re

import numpy as np
import pytest

import part_light_common as pc
import part_light_ref
import path_cases
import refusals_common

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# the colour bar of the deeper paths: not a tolerance of this file's own
COLOR_TOL = float(re.search(r"^COLOR_TOL\s*=\s*([0-9.eE+-]+)", open(os.path.join(HERE, "test_gpu_multi_bounce.py")).read(), re.M).group(1))
BAR = COLOR_TOL * pc.BAR_FACTOR
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
COUNTS = ("stats", "shadow", "glass", "glossy")
MAX_SPHERES = part_light_ref.MAX_SPHERES


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return part_light_ref.lib(tmp_path_factory)


def _plain_spheres(c):
    for i in range(MAX_SPHERES):
        c.set_sphere_gloss(i, 0.5, None)     # (any of the three model setters with None makes the surface diffuse)
        c.set_sphere_emission(i, None)


@pytest.fixture()
def ctx(gpu_ctx):
    """The shared context, left as it was found (test_gpu_light_sampling.py's fixture)."""
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


def _check(got, want, what):
    """Planes bit for bit, colour within the bar, RGBA8 within one code; the counts exactly."""
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"part light colour error {what}: {err:.3g} (bar {BAR:.3g}); light rays, reached, suppressed {got['light']} "
          f"(reference {(want['light_rays'], want['reached'], want['suppressed'])}), the mesh light's {got['part']} ({want['part_light']}), "
          f"emissive hits {got['emissive']} ({want['emissive_hits']})")
    assert got["light"] == (want["light_rays"], want["reached"], want["suppressed"]), (what, want["light_gen"].tolist())
    assert got["part"] == want["part_light"], (what, want["part_gen"].tolist())
    assert got["emissive"] == want["emissive_hits"], (what, want["gen_glow"].tolist())
    assert err <= BAR, (what, err)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, what
    return err


def _params(rwr, s, spp, seed=13, parts=True, light=None, emissive=True, bounces=None, extra=0):
    bounces = s["bounces"] if bounces is None else bounces
    return rwr.make_params(spp=spp, max_bounces=bounces, seed=seed,
                           flags=pc.flags(rwr, s, bounces=bounces, parts=parts, light=light, emissive=emissive, extra=extra))


@pytest.mark.parametrize("name,spp", [(n, k) for n in pc.SCENES for k in pc.spps(n)])
def test_matches_the_reference(rwr, orc, pref, ctx, ref_loader, suzanne, cube, name, spp):
    s = pc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    cam_inv = pc.camera(rwr, s)
    _upload(ctx, s)
    got = _frame(ctx, cam_inv, _params(rwr, s, spp))
    want = pc.reference(pref, rwr, orc, s, 13, spp, name)
    assert got["stats"] == (s["w"] * s["h"] * spp, want["rays"]), (name, spp, want["gen_rays"].tolist())
    assert got["glass"] == want["events"] and got["glossy"] == want["glossy"], (name, spp)
    _check(got, want, f"{name} spp={spp}")
    # nothing but the sums moves: the same context's frame without the flag has the planes, the counts and the traversal plan
    off = _frame(ctx, cam_inv, _params(rwr, s, spp, parts=False))
    for k in ("obj_id", "hit_t", "depth"):
        assert got[k].tobytes() == off[k].tobytes(), (name, k)
    _same_counts(got, off, (name, spp), light=False)
    assert got["plan"] == off["plan"] and off["part"] == (0, 0, 0)
    assert off["emissive"] + off["light"][2] == got["emissive"] + got["light"][2]
    assert (got["color_f32"].tobytes() != off["color_f32"].tobytes()) == (got["part"][0] + got["part"][2] > 0)
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
def test_32_bit_stacks_beside_nodelets_in_lds(rwr, orc, pref, ctx, ref_loader, suzanne, cube, name):
    """k_wf_light's form with nodelets in LDS and 32-bit stacks, for both values of PARTS: `bare_panel` with the new flag, `bare_lamp`
    with RWR_FLAG_LIGHT_SAMPLING alone - scenes of four and two faces, whose nodelets fit LDS beside stacks of twice the size - in a
    context created under RWR_WF_STACK16=0.  The traversal plan of the trace stage shows the form - k_wf_light picks its own by the
    same rule from the same arguments (lane_lds_plan without the wide form) - and the bytes and counts are the 16-bit run's, which the
    reference vouches for."""
    s = pc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    parts = name == "bare_panel"
    params = _params(rwr, s, 33, parts=parts)
    want = pc.reference(pref, rwr, orc, s, 13, 33, name, parts=parts)
    assert want["light_rays"] > want["reached"] > 0 and want["suppressed"] > 0
    cam_inv = pc.camera(rwr, s)
    _upload(ctx, s)
    got = _frame(ctx, cam_inv, params)
    _check(got, want, f"{name} 16-bit stacks")
    assert got["light"][1] > 0 and (got["part"][0] > 0) == parts
    assert got["plan"]["trace"]["launches"] > 0 and got["plan"]["trace"]["nodes_in_lds"] == 1 and got["plan"]["trace"]["stack16"] == 1, got["plan"]
    wide = _with_env(rwr, {"RWR_WF_STACK16": "0", "RWR_WF_WIDE_LANE": "0"}, s, cam_inv, params)
    assert wide["plan"]["trace"]["launches"] > 0 and wide["plan"]["trace"]["nodes_in_lds"] == 1 and wide["plan"]["trace"]["stack16"] == 0, wide["plan"]
    assert wide["plan"]["trace"]["wide"] == 0
    _same(wide, got, "32-bit stacks")
    _same_counts(wide, got, "32-bit stacks")


def test_the_cleared_flag_gives_the_frame_without_it(rwr, ctx, ref_loader, suzanne, cube, orc):
    """The flag without an emitting part, at max_bounces 0, or without RWR_FLAG_EMISSIVE: the bytes, the counts and the traversal
    plan of the frame without it, and no ray towards a face."""
    for name in ("panel", "panel_and_lamp"):
        s = pc.scene(name, rwr, ref_loader, suzanne, cube, orc)
        cam_inv = pc.camera(rwr, s)
        _upload(ctx, s)
        lit = _frame(ctx, cam_inv, _params(rwr, s, 2, seed=5))
        assert lit["part"][0] > 0

        def nothing(what, **kw):
            for spp, b, x in ((33, None, 0), (2, 1, rwr.FLAG_SHADOWS)) if "bounces" not in kw else ((2, 0, 0), (1, 0, rwr.FLAG_SHADOWS)):
                args = dict(dict(bounces=b, extra=x), **{k: v for k, v in kw.items() if k != "bounces"})
                want = _frame(ctx, cam_inv, _params(rwr, s, spp, seed=5, parts=False, **args))
                got = _frame(ctx, cam_inv, _params(rwr, s, spp, seed=5, **args))
                _same(got, want, (name, what, spp, b, x))
                _same_counts(got, want, (name, what, spp, b, x))
                assert got["part"] == (0, 0, 0) and got["plan"] == want["plan"]

        nothing("no bounce", bounces=0)
        nothing("no RWR_FLAG_EMISSIVE", emissive=False)
        for k in s["emissive_parts"]:
            ctx.set_part_emission(k, None)
        ctx.set_sphere_emission(0, (1.0, 2.0, 3.0))       # (something still emits: RWR_FLAG_EMISSIVE stays effective)
        nothing("no emitting part")
        ctx.set_part_emission(1, pc.PANEL_LE)             # the list is rebuilt: the frame is the lit one again
        if name == "panel":
            ctx.set_sphere_emission(0, None)
            again = _frame(ctx, cam_inv, _params(rwr, s, 2, seed=5))
            _same(again, lit, "the emission set again")
            _same_counts(again, lit, "the emission set again")


def test_light_sampling_without_the_new_flag_is_what_it_was(rwr, orc, pref, ctx, ref_loader, suzanne, cube):
    """panel_and_lamp with RWR_FLAG_LIGHT_SAMPLING but not the new flag: light_ref.c's frame and counts - the panel is found by chance,
    its Le is not suppressed, and the mesh light's share of the stats is zero."""
    s = pc.scene("panel_and_lamp", rwr, ref_loader, suzanne, cube, orc)
    cam_inv = pc.camera(rwr, s)
    _upload(ctx, s)
    for spp in (2, 33):
        got = _frame(ctx, cam_inv, _params(rwr, s, spp, parts=False))
        want = pc.reference(pref, rwr, orc, s, 13, spp, "panel_and_lamp", entry="light")
        _check(got, dict(want, part_light=(0, 0, 0)), f"RWR_FLAG_LIGHT_SAMPLING alone spp={spp}")
        assert got["stats"][1] == want["rays"] and got["light"][0] > 0 and got["part"] == (0, 0, 0)
        assert want["glow_by_surface"][1] > 0          # hits on the panel kept their Le


_STATS = re.compile(r"rwr wavefront pools: packets (\d+) pools / (\d+) rays, per-lane (\d+) pools / (\d+) rays.*\n"
                    r"rwr wavefront launches: packet (\d+), per-lane (\d+), per-lane wide (\d+)")
_LANE = {"RWR_WF_GROUP": "5", "RWR_WF_PACKET_RAYS": "0", "RWR_WF_MIN_PACKET_POOLS": "100000"}
SCHEDULES = {"packets": dict(path_cases.FORCED_SCHEDULE, RWR_WF_WIDE_LANE="0"),
             "per lane": dict(_LANE, RWR_WF_WIDE_LANE="0"),
             "wide lane": dict(_LANE, RWR_WF_WIDE_LANE="1"),
             "live list": {"RWR_WF_ZSPLIT": "2"}}


def test_schedules_give_the_same_frame(rwr, orc, pref, ctx, ref_loader, suzanne, cube, capfd):
    """Forced packets, the per-lane kernel alone, its wide form and the live-tile list on panel_and_lamp (both flags, shadow rays on):
    the default schedule's bytes and counts."""
    name = "panel_and_lamp"
    s = pc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    cam_inv = pc.camera(rwr, s)
    spp = 33
    params = _params(rwr, s, spp, extra=rwr.FLAG_SHADOWS)
    _upload(ctx, s)
    default = _frame(ctx, cam_inv, params)
    want = pc.reference(pref, rwr, orc, s, 13, spp, name, shadows=True)
    _check(default, want, f"schedule {name} default")
    assert default["stats"][1] == want["rays"] and default["light"][0] > default["part"][0] > default["part"][1] > 0 and default["part"][2] > 0
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


@pytest.mark.parametrize("name", ("panel", "panel_two_lamps", "tiny"))
def test_accumulated_frames_are_one_frame_of_all_samples(rwr, ctx, ref_loader, suzanne, cube, orc, name):
    s = pc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    cam_inv = pc.camera(rwr, s)
    _upload(ctx, s)
    want = _frame(ctx, cam_inv, _params(rwr, s, 2, seed=11))
    ctx.accum_reset()
    acc = _params(rwr, s, 1, seed=11, extra=rwr.FLAG_ACCUMULATE)      # (an accumulating frame's samples are placed by the RNG at spp 1 too)
    counts, share = np.zeros(3, np.int64), np.zeros(3, np.int64)
    for k in range(1, 3):
        ctx.render(cam_inv, acc)
        assert ctx.accum_samples() == k
        counts += np.asarray(ctx.last_light_stats())      # (an accumulating frame counts its own samples)
        share += np.asarray(ctx.last_part_light_stats())
    _same(ctx.readback(aux=True), want, "2 x 1 spp")
    assert tuple(counts.tolist()) == want["light"] and tuple(share.tolist()) == want["part"] and want["part"][0] > 0


@pytest.mark.parametrize("name", ("panel", "panel_and_lamp"))
def test_strips_bands_and_frames_in_flight(rwr, ctx, ref_loader, suzanne, cube, orc, name):
    """Strips of two ranks (the loopback gather for N = 2) and two row bands assemble the frame (planes, counts); 1 to 3 frames in
    flight give its bytes."""
    s = pc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    h = s["h"]
    cam_inv = pc.camera(rwr, s)
    params = _params(rwr, s, 2, seed=2, extra=rwr.FLAG_SHADOWS)
    _upload(ctx, s)
    full = _frame(ctx, cam_inv, params)
    assert full["part"][0] > 0
    asm = {k: np.zeros_like(full[k]) for k in PLANES}
    rays, light, share = 0, np.zeros(3, np.int64), np.zeros(3, np.int64)
    for r in range(2):
        part = _frame(ctx, cam_inv, params, strips=(r, 2))
        rows = [y for y in range(h) if (y // 8) % 2 == r]
        rays += part["stats"][1]
        light += np.asarray(part["light"])
        share += np.asarray(part["part"])
        for k in PLANES:
            asm[k][rows] = part[k][rows]
        ctx.dist_loopback_deposit(r, 2, True)
    ctx.dist_loopback_finish(2, True)
    _same(asm, full, (name, "strips"))
    assert rays == full["stats"][1] and tuple(light.tolist()) == full["light"] and tuple(share.tolist()) == full["part"]
    assert np.array_equal(ctx.dist_readback(), full["color"]), name
    asm = {k: np.zeros_like(full[k]) for k in PLANES}
    share = np.zeros(3, np.int64)
    for band in ((0, 16), (16, h)):
        part = _frame(ctx, cam_inv, params, rows=band)
        share += np.asarray(part["part"])
        for k in PLANES:
            asm[k][band[0]:band[1]] = part[k][band[0]:band[1]]
    _same(asm, full, (name, "bands"))
    assert tuple(share.tolist()) == full["part"]
    for n in (1, 2, 3):
        ctx.set_frames_in_flight(n)
        for i in range(n + 1):
            got = _frame(ctx, cam_inv, params)
            _same(got, full, (name, n, i))
            _same_counts(got, full, (name, n, i))


def test_the_flag_and_the_parts_emission_are_part_of_both_keys(rwr, ctx, ref_loader, suzanne, cube, orc):
    s = pc.scene("two_parts", rwr, ref_loader, suzanne, cube, orc)
    cam_inv = pc.camera(rwr, s)
    _upload(ctx, s)
    acc = _params(rwr, s, 2, seed=11, extra=rwr.FLAG_ACCUMULATE)
    off = _params(rwr, s, 2, seed=11, parts=False, extra=rwr.FLAG_ACCUMULATE)
    rep, rep_off = _params(rwr, s, 2, seed=11, extra=rwr.FLAG_REPROJECT), _params(rwr, s, 2, seed=11, parts=False, extra=rwr.FLAG_REPROJECT)

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
    before = ctx.last_part_light_stats()
    ctx.set_part_emission(2, None)                              # a part's emission changed: the list is shorter
    assert step() == 2 and ctx.last_part_light_stats()[0] > 0 and ctx.last_part_light_stats() != before and step() == 4
    ctx.set_part_emission(2, (1.0, 1.0, 1.0))                   # ... and changed again
    assert step() == 2 and step() == 4
    assert history() == 1 and history() == 2
    assert history(rep_off) == 1 and history(rep_off) == 2
    assert history() == 1 and history() == 2
    ctx.set_part_emission(2, (2.0, 1.0, 1.0))
    assert history() == 1 and history() == 2
    # the flag the frame clears is not part of a key: at max_bounces 0 the accumulation goes on across it
    flat, flat_off = _params(rwr, s, 2, seed=11, bounces=0, extra=rwr.FLAG_ACCUMULATE), _params(rwr, s, 2, seed=11, bounces=0, parts=False, extra=rwr.FLAG_ACCUMULATE)
    ctx.accum_reset()
    assert step(flat) == 2 and step(flat_off) == 4 and step(flat) == 6
    assert rwr.lib().rwr_last_part_light_stats(ctx._h, None, None, None) == rwr.ERR_INVALID_ARGUMENT
    assert rwr.lib().rwr_last_part_light_stats(None, None, None, None) == rwr.ERR_INVALID_ARGUMENT


def test_refusals(rwr, ctx, ref_loader, suzanne, cube, orc):
    """RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes refuse the flag - the code and the message - whatever
    max_bounces is and whether or not anything emits."""
    s = pc.scene("panel", rwr, ref_loader, suzanne, cube, orc)
    cam_inv = pc.camera(rwr, s)
    _upload(ctx, s)
    text = refusals_common.OFF_REFERENCE % "LIGHT_PARTS"
    for emitters in (True, False):
        if not emitters:
            ctx.set_part_emission(1, None)
        for params in (rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_LIGHT_PARTS | rwr.FLAG_ORTHO_RAYS),
                       rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_LIGHT_PARTS | rwr.FLAG_USE_BVH),
                       rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_LIGHT_PARTS | rwr.FLAG_ORTHO_RAYS)):
            with pytest.raises(rwr.RwrError) as ei:
                ctx.render(cam_inv, params)
            assert ei.value.code == rwr.ERR_UNSUPPORTED and text in str(ei.value), (params, str(ei.value))
        ctx.set_triangles(rwr.make_triangles([((0.0, 0.0, -2.0), (1.0, 0.0, -2.0), (0.0, 1.0, -2.0))]))
        try:
            for bounces in (0, 1):
                with pytest.raises(rwr.RwrError) as ei:
                    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=bounces, flags=rwr.FLAG_LIGHT_PARTS))
                assert ei.value.code == rwr.ERR_UNSUPPORTED and text in str(ei.value), str(ei.value)
        finally:
            ctx.set_triangles(rwr.make_triangles())
    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=1, flags=rwr.FLAG_LIGHT_PARTS | rwr.FLAG_EMISSIVE))   # the context is still usable
