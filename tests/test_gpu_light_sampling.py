"""Light sampling (RWR_FLAG_LIGHT_SAMPLING) on the GPU: k_wf_light, the marks and records the GLOW forms of the primary
kernel and of the two trace kernels leave for it, and add_glow's silenced hits, against the tests' CPU reference (light_ref.c):
  * sample-0 planes (object id, distance, depth) bit-exact; ray, shadow, glass and gloss counts equal to the reference's AND to the
    same context's frame without the flag; the three light counts and the emissive hits equal; RGBA8 within one code; colour within
    the bar tests/test_gpu_multi_bounce.py holds deeper paths to (COLOR_TOL there, read from that file) times
    max(1, min(64, 2 M the scene's largest Le)) - the largest value a light term can take, as tests/test_gpu_emission.py scales its
    bar by the largest Le;
  * every schedule, accumulation, strips, row bands, frames in flight and the loopback gather: the same bytes;
  * frames the flag does nothing to, the keys, the refusals, the two post-processes behind it.
The scenes are tests/light_common.py's; tests/test_light_host.py asserts with the reference alone that they exercise the rule."""
import os
import re

import numpy as np
import pytest

import denoise_ref
import light_common as lc
import light_ref
import path_cases
import refusals_common
import reproject_ref as rr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# the colour bar of the deeper paths: not a tolerance of this file's own
COLOR_TOL = float(re.search(r"^COLOR_TOL\s*=\s*([0-9.eE+-]+)", open(os.path.join(HERE, "test_gpu_multi_bounce.py")).read(), re.M).group(1))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
COUNTS = ("stats", "shadow", "glass", "glossy")
MAX_SPHERES = light_ref.MAX_SPHERES
SOFT = (0.05, 0.1)     # the combination's light radii


@pytest.fixture(scope="module")
def lref(tmp_path_factory):
    return light_ref.lib(tmp_path_factory)


def _plain_spheres(c):
    for i in range(MAX_SPHERES):
        c.set_sphere_gloss(i, 0.5, None)     # (any of the three model setters with None makes the surface diffuse)
        c.set_sphere_emission(i, None)


@pytest.fixture()
def ctx(gpu_ctx):
    """The shared context, left as it was found: default sky, point lights, plain dark spheres (the part attributes go with the next
    upload), no instances, no accumulation, one frame in flight."""
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
    for k, (rough, refl) in s["gloss_parts"].items():
        c.set_part_gloss(k, rough, refl)
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
    out["plan"] = c.last_traversal_plan()
    return out


def _same(a, b, what=""):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _same_counts(a, b, what="", light=True):
    for k in COUNTS + (("emissive", "light") if light else ()):
        assert a[k] == b[k], (what, k, a[k], b[k])


def _bar(s) -> float:
    return COLOR_TOL * lc.bar_factor(s)


def _check(got, want, what, bar):
    """tests/test_gpu_gloss.py's rule: planes bit for bit, colour within the bar, RGBA8 within one code; the counts exactly."""
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"light sampling colour error {what}: {err:.3g} (bar {bar:.3g}); light rays, reached, suppressed {got['light']} "
          f"(reference {(want['light_rays'], want['reached'], want['suppressed'])}), emissive hits {got['emissive']} ({want['emissive_hits']})")
    assert got["light"] == (want["light_rays"], want["reached"], want["suppressed"]), (what, want["light_gen"].tolist())
    assert got["emissive"] == want["emissive_hits"], (what, want["gen_glow"].tolist())
    assert err <= bar, (what, err)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, what
    return err


def _params(rwr, s, spp, seed=13, light=True, emissive=True, bounces=None, extra=0):
    bounces = s["bounces"] if bounces is None else bounces
    return rwr.make_params(spp=spp, max_bounces=bounces, seed=seed, flags=lc.flags(rwr, s, bounces=bounces, light=light, emissive=emissive, extra=extra))


@pytest.mark.parametrize("spp", lc.SPPS)
@pytest.mark.parametrize("name", lc.SCENES)
def test_matches_the_reference(rwr, orc, lref, ctx, ref_loader, suzanne, cube, name, spp):
    s = lc.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = lc.camera(rwr, s)
    _upload(ctx, s)
    got = _frame(ctx, cam_inv, _params(rwr, s, spp))
    want = lc.reference(lref, rwr, orc, s, 13, spp, name)
    assert got["stats"] == (s["w"] * s["h"] * spp, want["rays"]), (name, spp, want["gen_rays"].tolist())
    assert got["shadow"] == ((want["shadow_rays"], want["occluded"]) if s["shadows"] else (0, 0))
    assert got["glass"] == want["events"] and got["glossy"] == want["glossy"], (name, spp)
    _check(got, want, f"{name} spp={spp}", _bar(s))
    # nothing but the sums moves: the same context's frame with RWR_FLAG_EMISSIVE alone has the planes, the counts and the traversal plan
    off = _frame(ctx, cam_inv, _params(rwr, s, spp, light=False))
    for k in ("obj_id", "hit_t", "depth"):
        assert got[k].tobytes() == off[k].tobytes(), (name, k)
    _same_counts(got, off, (name, spp), light=False)
    assert got["plan"] == off["plan"] and off["light"] == (0, 0, 0)
    assert off["emissive"] == got["emissive"] + got["light"][2]
    assert (got["color_f32"].tobytes() != off["color_f32"].tobytes()) == (got["light"][0] + got["light"][2] > 0)


_STATS = re.compile(r"rwr wavefront pools: packets (\d+) pools / (\d+) rays, per-lane (\d+) pools / (\d+) rays.*\n"
                    r"rwr wavefront launches: packet (\d+), per-lane (\d+), per-lane wide (\d+)")
# tests/path_cases.py FORCED_SCHEDULE's packets, the per-lane kernel alone, its wide form asked for, a forced split of the tiles'
# samples (with it the live-tile list) and 32-bit traversal stacks
_LANE = {"RWR_WF_GROUP": "5", "RWR_WF_PACKET_RAYS": "0", "RWR_WF_MIN_PACKET_POOLS": "100000"}
SCHEDULES = {"packets": dict(path_cases.FORCED_SCHEDULE, RWR_WF_WIDE_LANE="0"),
             "per lane": dict(_LANE, RWR_WF_WIDE_LANE="0"),
             "wide lane": dict(_LANE, RWR_WF_WIDE_LANE="1"),
             "live list": {"RWR_WF_ZSPLIT": "2"},
             "stack32": {"RWR_WF_STACK16": "0"}}


@pytest.mark.parametrize("name", ("room", "two_lamps"))
def test_schedules_give_the_same_frame(rwr, orc, lref, ctx, ref_loader, suzanne, cube, capfd, name):
    """Forced packets, the per-lane kernel alone, its wide form, the live-tile list and 32-bit stacks: the default schedule's bytes and counts.
    Which kernels did run is read from the context's own account (RWR_WF_STATS=1, printed when it is destroyed)."""
    s = lc.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = lc.camera(rwr, s)
    spp = 33
    params = _params(rwr, s, spp, extra=rwr.FLAG_SHADOWS)
    _upload(ctx, s)
    default = _frame(ctx, cam_inv, params)
    want = lc.reference(lref, rwr, orc, s, 13, spp, name, shadows=True)
    _check(default, want, f"schedule {name} default", _bar(s))
    assert default["stats"][1] == want["rays"] and default["light"][0] > default["light"][1] > 0 and default["light"][2] > 0
    assert default["shadow"] == (want["shadow_rays"], want["occluded"])
    keys = sorted({k for env in SCHEDULES.values() for k in env} | {"RWR_WF_STATS"})
    saved = {k: os.environ.get(k) for k in keys}
    try:
        for what, env in SCHEDULES.items():
            for k in keys:
                os.environ.pop(k, None)
            os.environ.update(env)
            os.environ["RWR_WF_STATS"] = "1"
            capfd.readouterr()
            with rwr.Context(0) as c:        # the tunables are read when the context is created
                _upload(c, s)
                got = _frame(c, cam_inv, params)
            _same(got, default, (name, what))
            _same_counts(got, default, (name, what))
            m = _STATS.search(capfd.readouterr().err)
            assert m, (name, what)
            p_pools, p_rays, l_pools, l_rays, n_packet, n_lane, n_wide = map(int, m.groups())
            with capfd.disabled():
                print(f"light sampling schedule {name} {what}: packet pools {p_pools} ({p_rays} rays), per-lane pools {l_pools} ({l_rays} rays), "
                      f"launches packet {n_packet} / per-lane {n_lane} / wide {n_wide}, plan {got['plan']}")
            assert p_rays + l_rays == got["stats"][1], (name, what)     # every bounce ray went through a pool
            if what == "packets":
                assert n_packet > 0 and p_pools > 0, (name, what)
            elif what in ("per lane", "wide lane"):
                assert p_pools == 0 and n_lane + n_wide > 0 and (n_lane == 0 or n_wide == 0), (name, what)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("spp", (2, 33))
def test_a_bvh_that_leaves_lds(rwr, orc, lref, ctx, ref_loader, suzanne, cube, spp):
    """grid: sixteen instances of suzanne, whose nodelets do not fit LDS - k_wf_light's forms that walk them in memory.  With shadow
    rays on, so that the frame's traversal plan shows the shadow stage's form: k_wf_light picks its form by the same rule from the same
    arguments (lane_lds_plan without the wide form).  16-bit stacks first, then a context with RWR_WF_STACK16=0: the CPU reference's
    frame and counts, and the same bytes from both."""
    s = lc.scene("grid", rwr, ref_loader, suzanne, cube)
    cam_inv = lc.camera(rwr, s)
    params = _params(rwr, s, spp, extra=rwr.FLAG_SHADOWS)
    want = lc.reference(lref, rwr, orc, s, 13, spp, "grid", shadows=True)
    assert want["light_rays"] > want["reached"] > 0 and want["suppressed"] > 0
    _upload(ctx, s)
    got = _frame(ctx, cam_inv, params)
    assert got["stats"][1] == want["rays"] and got["shadow"] == (want["shadow_rays"], want["occluded"])
    _check(got, want, f"grid spp={spp} 16-bit stacks", _bar(s))
    for stage in ("trace", "shadow"):
        assert got["plan"][stage]["launches"] > 0 and got["plan"][stage]["nodes_in_lds"] == 0 and got["plan"][stage]["stack16"] == 1, got["plan"]
    saved = os.environ.get("RWR_WF_STACK16")
    os.environ["RWR_WF_STACK16"] = "0"
    try:
        with rwr.Context(0) as c:        # the switch is read when the context is created
            _upload(c, s)
            wide = _frame(c, cam_inv, params)
    finally:
        if saved is None:
            os.environ.pop("RWR_WF_STACK16", None)
        else:
            os.environ["RWR_WF_STACK16"] = saved
    for stage in ("trace", "shadow"):
        assert wide["plan"][stage]["nodes_in_lds"] == 0 and wide["plan"][stage]["stack16"] == 0, wide["plan"]
    _same(wide, got, "32-bit stacks")
    _same_counts(wide, got, "32-bit stacks")


@pytest.mark.parametrize("name", ("room", "eight_lamps", "tiny", "combo"))
def test_accumulated_frames_are_one_frame_of_all_samples(rwr, ctx, ref_loader, suzanne, cube, name):
    s = lc.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = lc.camera(rwr, s)
    _upload(ctx, s)
    want = _frame(ctx, cam_inv, _params(rwr, s, 2, seed=11))
    ctx.accum_reset()
    acc = _params(rwr, s, 1, seed=11, extra=rwr.FLAG_ACCUMULATE)      # (an accumulating frame's samples are placed by the RNG at spp 1 too)
    counts = np.zeros(3, np.int64)
    for k in range(1, 3):
        ctx.render(cam_inv, acc)
        assert ctx.accum_samples() == k
        counts += np.asarray(ctx.last_light_stats())      # (an accumulating frame counts its own samples)
    _same(ctx.readback(aux=True), want, "2 x 1 spp")
    assert tuple(counts.tolist()) == want["light"] and want["light"][0] > 0


@pytest.mark.parametrize("name", ("room", "two_lamps", "hidden", "combo"))
def test_strips_bands_and_frames_in_flight(rwr, ctx, ref_loader, suzanne, cube, name):
    """Strips of two ranks (the loopback gather for N = 2) and two row bands assemble the frame (planes, counts); 1 to 3 frames in
    flight give its bytes."""
    s = lc.scene(name, rwr, ref_loader, suzanne, cube)
    h = s["h"]
    cam_inv = lc.camera(rwr, s)
    params = _params(rwr, s, 2, seed=2, extra=rwr.FLAG_SHADOWS)
    _upload(ctx, s)
    full = _frame(ctx, cam_inv, params)
    assert full["light"][0] > 0
    asm = {k: np.zeros_like(full[k]) for k in PLANES}
    rays, shadow, light = 0, np.zeros(2, np.int64), np.zeros(3, np.int64)
    for r in range(2):
        part = _frame(ctx, cam_inv, params, strips=(r, 2))
        rows = [y for y in range(h) if (y // 8) % 2 == r]
        rays += part["stats"][1]
        shadow += np.asarray(part["shadow"])
        light += np.asarray(part["light"])
        for k in PLANES:
            asm[k][rows] = part[k][rows]
        ctx.dist_loopback_deposit(r, 2, True)
    ctx.dist_loopback_finish(2, True)
    _same(asm, full, (name, "strips"))
    assert rays == full["stats"][1] and tuple(shadow.tolist()) == full["shadow"] and tuple(light.tolist()) == full["light"]
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


def test_the_cleared_flag_gives_the_frame_without_it(rwr, ctx, ref_loader, suzanne, cube):
    """The flag without RWR_FLAG_EMISSIVE, without an emitting sphere in use (an emitting part alone; a sphere index the scene lacks),
    or at max_bounces 0: the bytes, the counts and the traversal plan of the frame without it, and no light ray."""
    for name in ("room", "mirror_lamp"):
        s = lc.scene(name, rwr, ref_loader, suzanne, cube)
        cam_inv = lc.camera(rwr, s)
        _upload(ctx, s)
        lit = _frame(ctx, cam_inv, _params(rwr, s, 2, seed=5))
        assert lit["light"][0] > 0

        def nothing(what, **kw):
            for spp, b, x in ((33, None, 0), (1, 0, 0), (2, 1, rwr.FLAG_SHADOWS)) if "bounces" not in kw else ((2, 0, 0), (1, 0, rwr.FLAG_SHADOWS)):
                args = dict(dict(bounces=b, extra=x), **{k: v for k, v in kw.items() if k != "bounces"})
                want = _frame(ctx, cam_inv, _params(rwr, s, spp, seed=5, light=False, **args))
                got = _frame(ctx, cam_inv, _params(rwr, s, spp, seed=5, **args))
                _same(got, want, (name, what, spp, b, x))
                _same_counts(got, want, (name, what, spp, b, x))
                assert got["light"] == (0, 0, 0) and got["plan"] == want["plan"]

        nothing("no bounce", bounces=0)
        nothing("no RWR_FLAG_EMISSIVE", emissive=False)
        for k in s["emissive_spheres"]:
            ctx.set_sphere_emission(k, None)
        ctx.set_part_emission(0, (1.0, 2.0, 3.0))
        nothing("an emitting part alone")
        ctx.set_sphere_emission(MAX_SPHERES - 1, (8.0, 8.0, 8.0))
        nothing("a sphere that is not there")
        ctx.set_sphere_emission(MAX_SPHERES - 1, None)


def test_the_flag_and_the_emitters_are_part_of_both_keys(rwr, ctx, ref_loader, suzanne, cube):
    s = lc.scene("two_lamps", rwr, ref_loader, suzanne, cube)
    cam_inv = lc.camera(rwr, s)
    _upload(ctx, s)
    acc = _params(rwr, s, 2, seed=11, extra=rwr.FLAG_ACCUMULATE)
    off = _params(rwr, s, 2, seed=11, light=False, extra=rwr.FLAG_ACCUMULATE)
    rep, rep_off = _params(rwr, s, 2, seed=11, extra=rwr.FLAG_REPROJECT), _params(rwr, s, 2, seed=11, light=False, extra=rwr.FLAG_REPROJECT)

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
    ctx.set_sphere_emission(2, None)                            # the list of emitting spheres changed: one lamp fewer
    assert step() == 2 and ctx.last_light_stats()[0] > 0 and step() == 4
    ctx.set_sphere_emission(1, (1.0, 1.0, 1.0))                 # ... one more
    assert step() == 2 and step() == 4
    ctx.set_spheres(s["spheres"][:1])                           # ... the spheres in use
    assert step() == 2 and step() == 4
    ctx.set_spheres(s["spheres"])
    assert history() == 1 and history() == 2
    assert history(rep_off) == 1 and history(rep_off) == 2
    assert history() == 1 and history() == 2
    ctx.set_sphere_emission(1, None)
    assert history() == 1 and history() == 2
    # the flag the frame clears is not part of a key: at max_bounces 0 the accumulation goes on across it
    flat, flat_off = _params(rwr, s, 2, seed=11, bounces=0, extra=rwr.FLAG_ACCUMULATE), _params(rwr, s, 2, seed=11, bounces=0, light=False, extra=rwr.FLAG_ACCUMULATE)
    ctx.accum_reset()
    assert step(flat) == 2 and step(flat_off) == 4 and step(flat) == 6
    assert rwr.lib().rwr_last_light_stats(ctx._h, None, None, None) == rwr.ERR_INVALID_ARGUMENT
    assert rwr.lib().rwr_last_light_stats(None, None, None, None) == rwr.ERR_INVALID_ARGUMENT


def test_the_combination_matches_the_reference(rwr, orc, lref, ctx, ref_loader, suzanne, cube):
    """combo: RWR_FLAG_SHADOWS + soft shadows + sky + a mirror part + a glass sphere + the flag in one frame."""
    s = lc.scene("combo", rwr, ref_loader, suzanne, cube)
    cam_inv = lc.camera(rwr, s)
    _upload(ctx, s)
    sky = (light_ref.glass_ref.DEFAULT_ZENITH, light_ref.glass_ref.DEFAULT_HORIZON)
    ctx.shadow_set_params(*SOFT)
    extra = rwr.FLAG_SKY | rwr.FLAG_SOFT_SHADOWS
    for spp in (2, 33):
        got = _frame(ctx, cam_inv, _params(rwr, s, spp, extra=extra))
        want = lc.reference(lref, rwr, orc, s, 13, spp, "combo soft sky", radii=SOFT, sky=sky)
        assert got["stats"][1] == want["rays"] and got["shadow"] == (want["shadow_rays"], want["occluded"]) and got["glass"] == want["events"]
        assert got["light"][0] > got["light"][1] > 0 and got["light"][2] > 0 and want["sky_terms"] > 0 and want["gen_mirror"].sum() > 0
        _check(got, want, f"combo spp={spp}", COLOR_TOL * max(lc.bar_factor(s), max(max(sky[0]), max(sky[1]))))


def test_refusals(rwr, ctx, ref_loader, suzanne, cube):
    """RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes refuse the flag - the code and the message - whatever
    max_bounces is and whether or not anything emits."""
    s = lc.scene("room", rwr, ref_loader, suzanne, cube)
    cam_inv = lc.camera(rwr, s)
    _upload(ctx, s)
    text = refusals_common.OFF_REFERENCE % "LIGHT_SAMPLING"
    for emitters in (True, False):
        if not emitters:
            ctx.set_sphere_emission(0, None)
        for params in (rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_LIGHT_SAMPLING | rwr.FLAG_ORTHO_RAYS),
                       rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_LIGHT_SAMPLING | rwr.FLAG_USE_BVH),
                       rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_LIGHT_SAMPLING | rwr.FLAG_ORTHO_RAYS)):
            with pytest.raises(rwr.RwrError) as ei:
                ctx.render(cam_inv, params)
            assert ei.value.code == rwr.ERR_UNSUPPORTED and text in str(ei.value), (params, str(ei.value))
        ctx.set_triangles(rwr.make_triangles([((0.0, 0.0, -2.0), (1.0, 0.0, -2.0), (0.0, 1.0, -2.0))]))
        try:
            for bounces in (0, 1):
                with pytest.raises(rwr.RwrError) as ei:
                    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=bounces, flags=rwr.FLAG_LIGHT_SAMPLING))
                assert ei.value.code == rwr.ERR_UNSUPPORTED and text in str(ei.value), str(ei.value)
        finally:
            ctx.set_triangles(rwr.make_triangles())
    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=1, flags=rwr.FLAG_LIGHT_SAMPLING | rwr.FLAG_EMISSIVE))   # the context is still usable


def test_the_denoiser_filters_the_light_sampled_frame(rwr, orc, lref, ctx, ref_loader, suzanne, cube, tmp_path_factory):
    """With RWR_FLAG_DENOISE the frame of `room` is denoise_ref.c applied to the light reference's planes, within the colour bar: the
    filter runs behind the resolve and leaves the traced sums alone."""
    dref = denoise_ref.lib(tmp_path_factory)
    s = lc.scene("room", rwr, ref_loader, suzanne, cube)
    cam_inv = lc.camera(rwr, s)
    _upload(ctx, s)
    ref = lc.reference(lref, rwr, orc, s, 9, 2, "room")
    nhat = denoise_ref.face_normals(dref, orc, s["model"], None)
    want = denoise_ref.denoise(dref, ref["color_f32"], ref["obj_id"], ref["hit_t"], nhat, **denoise_ref.DEFAULTS)
    ctx.set_denoise_params()
    plain = _frame(ctx, cam_inv, _params(rwr, s, 2, seed=9))
    got = _frame(ctx, cam_inv, _params(rwr, s, 2, seed=9, extra=rwr.FLAG_DENOISE))
    assert got["light"] == plain["light"] and plain["light"][0] > 0
    _check(got, dict(ref, color_f32=want["color_f32"], color=want["color"]), "room denoised", _bar(s))
    assert got["color_f32"].tobytes() != plain["color_f32"].tobytes()              # the filter ran


def test_reprojection_blends_the_light_sampled_frames(rwr, orc, lref, ref_loader, suzanne, cube, tmp_path_factory):
    """Two reprojecting frames of `room` are the frames of seed and seed + 1 (each against the CPU reference) blended by reproject_ref.c."""
    s = lc.scene("room", rwr, ref_loader, suzanne, cube)
    cam_inv = lc.camera(rwr, s)
    cam = cam_inv.view(rwr.CAMERA_INV_DTYPE)
    seed, spp = 21, 2
    L = rr.lib(tmp_path_factory)
    nhat = denoise_ref.face_normals(denoise_ref.lib(tmp_path_factory), orc, s["model"], None)
    with rwr.Context(0) as B:
        _upload(B, s)
        plains = [_frame(B, cam_inv, _params(rwr, s, spp, seed=seed + k)) for k in range(2)]
    for k, f in enumerate(plains):
        _check(f, lc.reference(lref, rwr, orc, s, seed + k, spp, "room"), f"reproject plain {k}", _bar(s))
    chain = rr.chain(L, plains, nhat, [cam, cam])
    with rwr.Context(0) as A:
        _upload(A, s)
        params = _params(rwr, s, spp, seed=seed, extra=rwr.FLAG_REPROJECT)
        for k in range(2):
            A.render(cam, params)
            got = A.readback(aux=True)
            assert A.reproject_frames() == k + 1 and A.last_light_stats() == plains[k]["light"] and plains[k]["light"][0] > 0
            for p in ("depth", "obj_id", "hit_t"):
                assert got[p].tobytes() == plains[k][p].tobytes(), (k, p)
            err = float(np.abs(got["color_f32"] - chain[k]["color_f32"]).max())
            print(f"light sampling reprojection frame {k}: colour error {err:.3g}")
            assert err <= _bar(s), (k, err)
            assert np.abs(got["color"].astype(int) - chain[k]["color"].astype(int)).max() <= 1
            assert A.reproject_history().tobytes() == chain[k]["n"].tobytes()
