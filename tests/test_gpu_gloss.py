"""Glossy surfaces (RWR_FLAG_GLOSSY) on the GPU: the glossy forms of the primary kernel and of the trace kernels' EMIT
forms against the tests' CPU reference (gloss_ref.c):
  * sample-0 planes (object id, distance, depth) bit-exact; bounce-ray, shadow-ray, occluded, glass-event and glossy-ray counts
    equal - where every glossy ray went steers the ray counts of the generations after it; RGBA8 within one code; colour within the
    bar tests/test_gpu_multi_bounce.py holds deeper paths to (COLOR_TOL there, read from that file: a reflectance <= 1 travels
    through the same unorm16 throughput as an albedo), scaled by the sky's largest component as tests/test_gpu_sky.py scales it;
  * every schedule, split, frames in flight and accumulation: the same bytes;
  * frames the flag does nothing to, the setters, one model per surface, the accumulation key, the refusals.
The scenes are tests/gloss_common.py's; tests/test_gloss_host.py asserts with the reference alone that they exercise the rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gloss_common
import gloss_ref
import path_cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# the colour bar of the deeper paths, for the same B: not a tolerance of this file's own
COLOR_TOL = float(re.search(r"^COLOR_TOL\s*=\s*([0-9.eE+-]+)", open(os.path.join(HERE, "test_gpu_multi_bounce.py")).read(), re.M).group(1))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
DEFAULT = (gloss_ref.glass_ref.DEFAULT_ZENITH, gloss_ref.glass_ref.DEFAULT_HORIZON)
BAR = COLOR_TOL * max(1.0, max(max(c) for c in DEFAULT))     # tests/test_gpu_sky.py's scaling: the default sky's components are <= 1
MAX_SPHERES = gloss_ref.MAX_SPHERES


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return gloss_ref.lib(tmp_path_factory)


def _plain_spheres(c):
    for i in range(MAX_SPHERES):
        c.set_sphere_gloss(i, 0.5, None)     # (any of the three setters with None makes the surface diffuse)


@pytest.fixture()
def ctx(gpu_ctx):
    """The shared context, left as it was found: default sky, plain spheres (the part attributes go with the next upload), no
    instances, no accumulation, one frame in flight."""
    gpu_ctx.sky_set_params()
    _plain_spheres(gpu_ctx)
    yield gpu_ctx
    gpu_ctx.sky_set_params()
    _plain_spheres(gpu_ctx)
    gpu_ctx.set_instances(None)
    gpu_ctx.set_frames_in_flight(1)
    gpu_ctx.accum_reset()


def _flags(rwr, bounces, gloss=True, glass=True, mirrors=True, sky=True, shadows=False, extra=0):
    return (rwr.FLAG_AUX_OUTPUTS | extra | (rwr.FLAG_MULTI_BOUNCE if bounces > 1 else 0) | (rwr.FLAG_SHADOWS if shadows else 0) |
            (rwr.FLAG_SKY if sky else 0) | (rwr.FLAG_MIRRORS if mirrors else 0) | (rwr.FLAG_GLASS if glass else 0) |
            (rwr.FLAG_GLOSSY if gloss else 0))


def _upload(c, s, gloss=True):
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
    for k, r in s["mirror_spheres"].items():
        c.set_sphere_mirror(k, r)
    for k, (ior, tint) in s["glass_parts"].items():
        c.set_part_glass(k, ior, tint)
    for k, (ior, tint) in s["glass_spheres"].items():
        c.set_sphere_glass(k, ior, tint)
    if gloss:
        for k, (rough, refl) in s["gloss_parts"].items():
            c.set_part_gloss(k, rough, refl)
        for k, (rough, refl) in s["gloss_spheres"].items():
            c.set_sphere_gloss(k, rough, refl)


def _frame(c, cam_inv, params, **kw):
    c.render(cam_inv, params, **kw)
    out = c.readback(aux=True)
    out["stats"] = c.last_render_stats()
    out["shadow"] = c.last_shadow_stats()
    out["glass"] = c.last_glass_stats()
    out["glossy"] = c.last_gloss_stats()
    return out


def _same(a, b, what=""):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _same_counts(a, b, what=""):
    for k in ("stats", "shadow", "glass", "glossy"):
        assert a[k] == b[k], (what, k)


def _check(got, want, what, rounded=None):
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"gloss colour error {what}: {err:.3g} (bar {BAR:.3g})")
    if err > BAR and rounded is not None:     # (tell the ray record's throughput rounding from a fault; the bar itself stays)
        print(f"gloss colour error {what} against the reference with thr_unorm16: {float(np.abs(got['color_f32'] - rounded()['color_f32']).max()):.3g}")
    assert err <= BAR, (what, err)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, what


@pytest.mark.parametrize("spp", gloss_common.SPPS)
@pytest.mark.parametrize("name", gloss_common.GPU_SCENES)
def test_matches_the_reference(rwr, orc, sref, ctx, ref_loader, suzanne, cube, name, spp):
    s = gloss_common.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = gloss_common.camera(rwr, s)
    _upload(ctx, s)
    bounces, shadows = s["bounces"], spp == 2          # (the two-sample frames carry the shadow rays)
    got = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=bounces, seed=13, flags=_flags(rwr, bounces, shadows=shadows)))
    want = gloss_common.reference(sref, rwr, orc, s, 13, spp, sky=DEFAULT, shadows=shadows, name=name)
    assert want["glossy"] > 0
    print(f"gloss {name} spp {spp}: glossy rays {got['glossy']} (reference {want['glossy']}), rays {got['stats'][1]} (reference {want['rays']}), "
          f"glass events {got['glass']} (reference {want['events']})")
    assert got["glossy"] == want["glossy"], (name, spp, want["gen_gloss"].tolist())
    assert got["glass"] == want["events"], (name, spp)
    assert got["stats"] == (s["w"] * s["h"] * spp, want["rays"]), (name, spp, want["gen_rays"].tolist())
    assert got["shadow"] == ((want["shadow_rays"], want["occluded"]) if shadows else (0, 0))
    _check(got, want, f"{name} spp={spp}",
           rounded=lambda: gloss_common.reference(sref, rwr, orc, s, 13, spp, sky=DEFAULT, shadows=shadows, name=name, thr_unorm16=True))
    # sample-0 planes do not depend on the flag, nor does the first generation's ray count
    off = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=1, seed=13, flags=_flags(rwr, 1, gloss=False, shadows=shadows)))
    for k in ("obj_id", "hit_t", "depth"):
        assert got[k].tobytes() == off[k].tobytes(), (name, k)
    assert off["stats"][1] == want["gen_rays"][1] and off["glossy"] == 0


_STATS = re.compile(r"rwr wavefront pools: packets (\d+) pools / (\d+) rays, per-lane (\d+) pools / (\d+) rays.*\n"
                    r"rwr wavefront launches: packet (\d+), per-lane (\d+), per-lane wide (\d+)")
# tests/test_gpu_fuzz.py's forced-packet schedule (tests/path_cases.py FORCED_SCHEDULE) and the wide per-lane kernel asked for
SCHEDULES = {"packets": dict(path_cases.FORCED_SCHEDULE, RWR_WF_WIDE_LANE="0"),
             "wide lane": {"RWR_WF_GROUP": "5", "RWR_WF_PACKET_RAYS": "0", "RWR_WF_MIN_PACKET_POOLS": "100000", "RWR_WF_WIDE_LANE": "1"}}


@pytest.mark.parametrize("name", ("instances", "all_three"))
def test_schedules_give_the_same_frame(rwr, orc, sref, ctx, ref_loader, suzanne, cube, capfd, name):
    """Forced packets and the wide per-lane kernel asked for: the default schedule's bytes and counts.  Which kernels did run is
    read from the context's own account (RWR_WF_STATS=1, printed when it is destroyed)."""
    s = gloss_common.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = gloss_common.camera(rwr, s)
    spp = 7
    params = rwr.make_params(spp=spp, max_bounces=s["bounces"], seed=13, flags=_flags(rwr, s["bounces"], shadows=True))
    want = gloss_common.reference(sref, rwr, orc, s, 13, spp, sky=DEFAULT, shadows=True, name=name)
    _upload(ctx, s)
    default = _frame(ctx, cam_inv, params)
    _check(default, want, f"schedule {name} default")
    assert default["stats"][1] == want["rays"] and default["glossy"] == want["glossy"] and default["glass"] == want["events"]
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
                print(f"gloss schedule {name} {what}: packet pools {p_pools} ({p_rays} rays), per-lane pools {l_pools} ({l_rays} rays), "
                      f"launches packet {n_packet} / per-lane {n_lane} / wide {n_wide}")
            assert p_rays + l_rays == got["stats"][1], (name, what)     # every bounce ray went through a pool
            if what == "packets":
                assert n_packet > 0 and p_pools > 0, (name, what)
            else:
                assert n_lane + n_wide > 0 and (n_lane == 0 or n_wide == 0), (name, what)
                if name == "instances":   # a BVH too large for a copy per 256-thread workgroup: the switch decides
                    assert n_wide > 0 and n_lane == 0, (name, what)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("name", gloss_common.GPU_SCENES)
def test_accumulated_frames_are_one_frame_of_all_samples(rwr, ctx, ref_loader, suzanne, cube, name):
    s = gloss_common.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = gloss_common.camera(rwr, s)
    _upload(ctx, s)
    flags = _flags(rwr, s["bounces"])
    want = _frame(ctx, cam_inv, rwr.make_params(spp=6, max_bounces=s["bounces"], seed=11, flags=flags))
    ctx.accum_reset()
    acc = rwr.make_params(spp=2, max_bounces=s["bounces"], seed=11, flags=flags | rwr.FLAG_ACCUMULATE)
    glossy = 0
    for k in range(1, 4):
        ctx.render(cam_inv, acc)
        assert ctx.accum_samples() == 2 * k
        glossy += ctx.last_gloss_stats()      # (an accumulating frame counts its own rays)
    _same(ctx.readback(aux=True), want, "3 x 2 spp")
    assert glossy == want["glossy"] > 0


@pytest.mark.parametrize("name", [n for n in gloss_common.GPU_SCENES if n != "tiny"])   # (three rows are one strip: nothing to deal out)
def test_strips_and_frames_in_flight(rwr, ctx, ref_loader, suzanne, cube, name):
    """Strips of two ranks assemble the frame (planes, ray counts, glossy counts); 1 to 3 frames in flight give its bytes."""
    s = gloss_common.scene(name, rwr, ref_loader, suzanne, cube)
    h = s["h"]
    cam_inv = gloss_common.camera(rwr, s)
    params = rwr.make_params(spp=3, max_bounces=s["bounces"], seed=2, flags=_flags(rwr, s["bounces"], shadows=True))
    _upload(ctx, s)
    full = _frame(ctx, cam_inv, params)
    assert full["glossy"] > 0
    asm = {k: np.zeros_like(full[k]) for k in PLANES}
    rays, shadow, events, glossy = 0, np.zeros(2, np.int64), np.zeros(3, np.int64), 0
    for r in range(2):
        part = _frame(ctx, cam_inv, params, strips=(r, 2))
        rows = [y for y in range(h) if (y // 8) % 2 == r]
        rays += part["stats"][1]
        shadow += np.asarray(part["shadow"])
        events += np.asarray(part["glass"])
        glossy += part["glossy"]
        for k in PLANES:
            asm[k][rows] = part[k][rows]
        ctx.dist_loopback_deposit(r, 2, True)
    ctx.dist_loopback_finish(2, True)
    _same(asm, full, (name, "strips"))
    assert rays == full["stats"][1] and tuple(shadow.tolist()) == full["shadow"] and tuple(events.tolist()) == full["glass"] and glossy == full["glossy"]
    assert np.array_equal(ctx.dist_readback(), full["color"]), name
    for n in (1, 2, 3):
        ctx.set_frames_in_flight(n)
        for i in range(n + 1):
            got = _frame(ctx, cam_inv, params)
            _same(got, full, (name, n, i))
            _same_counts(got, full, (name, n, i))


def test_frames_the_flag_does_nothing_to(rwr, ctx, ref_loader, suzanne, cube):
    for name in ("two_parts", "all_three", "inside_sphere"):
        s = gloss_common.scene(name, rwr, ref_loader, suzanne, cube)
        cam_inv = gloss_common.camera(rwr, s)
        b = s["bounces"]
        spp = 3
        with rwr.Context(0) as fresh:      # a context on which no gloss setter was ever called (the scene's mirrors and glass are set)
            _upload(fresh, s, gloss=False)
            never = {sh: _frame(fresh, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b, gloss=False, shadows=sh)))
                     for sh in (False, True)}
            flat = {(n, sh): _frame(fresh, cam_inv, rwr.make_params(spp=n, max_bounces=0, seed=5, flags=_flags(rwr, 0, gloss=False, shadows=sh)))
                    for n, sh in ((1, False), (4, False), (1, True))}
        _upload(ctx, s)
        for sh in (False, True):
            # the flag off with gloss set: byte for byte the context that never heard of gloss
            off = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b, gloss=False, shadows=sh)))
            _same(off, never[sh], (name, "flag off", sh))
            _same_counts(off, never[sh], (name, "flag off", sh))
            assert off["glossy"] == 0
            on = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b, shadows=sh)))
            assert on["color_f32"].tobytes() != off["color_f32"].tobytes() and on["glossy"] > 0
            for k in ("depth", "obj_id", "hit_t"):
                assert on[k].tobytes() == off[k].tobytes(), (name, k)
            # ... and with the glossy flag alone the scene's mirrors and glass are the diffuse surfaces they were
            if s["mirror_parts"]:
                alone = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b, mirrors=False, glass=False, shadows=sh)))
                assert alone["color_f32"].tobytes() != on["color_f32"].tobytes() and alone["glossy"] > 0 and alone["glass"] == (0, 0, 0)
        # no bounce: the flag is ignored (the reference frame at spp 1 too)
        for (n, sh), want in flat.items():
            on = _frame(ctx, cam_inv, rwr.make_params(spp=n, max_bounces=0, seed=5, flags=_flags(rwr, 0, shadows=sh)))
            _same(on, want, (name, "no bounce", n, sh))
            _same_counts(on, want, (name, "no bounce", n, sh))
        # every glossy surface cleared again, then none ever set (a new upload): the flag alone changes nothing
        for k in s["gloss_parts"]:
            ctx.set_part_gloss(k, 0.5, None)
        for k in s["gloss_spheres"]:
            ctx.set_sphere_gloss(k, 0.5, None)
        for what in ("cleared", "never set"):
            if what == "never set":
                _upload(ctx, s, gloss=False)
            for sh in (False, True):
                on = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b, shadows=sh)))
                _same(on, never[sh], (name, what, sh))
                _same_counts(on, never[sh], (name, what, sh))
        # gloss on a sphere index the scene does not have is no gloss of the scene
        ctx.set_sphere_gloss(MAX_SPHERES - 1, 0.5, (1.0, 1.0, 1.0))
        on = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b)))
        _same(on, never[False], (name, "a sphere that is not there"))
        ctx.set_sphere_gloss(MAX_SPHERES - 1, 0.5, None)


def test_setters_and_accumulation_key(rwr, ctx, ref_loader, suzanne, cube):
    """Every accepted call of a gloss setter changes the scene's generation - with or without the flag, whether or not the value
    is new - and a refused call changes nothing; the flag (after its clearing rule) is one of the key's flags."""
    s = gloss_common.scene("two_parts", rwr, ref_loader, suzanne, cube)
    cam_inv = gloss_common.camera(rwr, s)
    _upload(ctx, s)
    b = s["bounces"]
    acc = rwr.make_params(spp=2, max_bounces=b, seed=11, flags=_flags(rwr, b) | rwr.FLAG_ACCUMULATE)
    off = rwr.make_params(spp=2, max_bounces=b, seed=11, flags=_flags(rwr, b, gloss=False) | rwr.FLAG_ACCUMULATE)
    W = gloss_common.WHITE

    def step(params=acc):
        ctx.render(cam_inv, params)
        return ctx.accum_samples()

    ctx.accum_reset()
    assert step() == 2 and step() == 4
    ctx.set_part_gloss(1, np.nextafter(np.float32(0.25), np.float32(1.0)), W)                   # one ulp of the roughness
    assert step() == 2 and step() == 4
    ctx.set_part_gloss(1, 0.25, (1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 1.0))      # one ulp of the reflectance
    assert step() == 2 and step() == 4
    ctx.set_sphere_gloss(5, 0.5, (0.5, 0.5, 0.5))                   # no sphere of this scene: the scene changed all the same
    assert step() == 2 and step() == 4
    ctx.set_sphere_gloss(5, 0.5, (0.5, 0.5, 0.5))                   # the value it has already
    assert step() == 2 and step() == 4
    ctx.set_sphere_gloss(5, 0.5, None)                              # clear
    assert step() == 2 and step() == 4
    assert step(off) == 2 and step(off) == 4                        # the flag toggled ...
    assert step() == 2                                              # ... and back
    assert step(off) == 2 and step(off) == 4
    ctx.set_part_gloss(0, 0.75, (0.5, 0.5, 0.5))                    # with the flag off a setter still changes the scene
    assert step(off) == 2 and step(off) == 4
    # refused calls change nothing: the state, the accumulation - with the flag off and with it on
    before = (ctx.get_part_gloss(0), ctx.get_part_gloss(1), ctx.get_sphere_gloss(0))
    bad_calls = [lambda: ctx.set_part_gloss(0, 0.0, W), lambda: ctx.set_part_gloss(0, np.nextafter(np.float32(2.0 ** -10), np.float32(0.0)), W),
                 lambda: ctx.set_part_gloss(0, np.nextafter(np.float32(1.0), np.float32(2.0)), W), lambda: ctx.set_part_gloss(0, -0.5, W),
                 lambda: ctx.set_part_gloss(0, np.nan, W), lambda: ctx.set_part_gloss(0, np.inf, W),
                 lambda: ctx.set_part_gloss(0, 0.5, (2.0, 0.0, 0.0)), lambda: ctx.set_part_gloss(0, 0.5, (0.5, -0.1, 0.5)),
                 lambda: ctx.set_part_gloss(0, 0.5, (0.5, 0.5, np.nan)), lambda: ctx.set_part_gloss(7, 0.5, W),
                 lambda: ctx.set_part_gloss(7, 0.5, None), lambda: ctx.set_sphere_gloss(MAX_SPHERES, 0.5, W),
                 lambda: ctx.set_sphere_gloss(0, 1.5, W), lambda: ctx.set_sphere_gloss(0, 0.5, (np.inf, 0.0, 0.0)),
                 lambda: ctx.get_part_gloss(7), lambda: ctx.get_sphere_gloss(MAX_SPHERES)]
    for bad in bad_calls:
        with pytest.raises(rwr.RwrError) as ei:
            bad()
        assert ei.value.code == rwr.ERR_INVALID_ARGUMENT
    assert step(off) == 6
    assert step() == 2 and step() == 4
    for bad in bad_calls:
        with pytest.raises(rwr.RwrError):
            bad()
    assert step() == 6
    after = (ctx.get_part_gloss(0), ctx.get_part_gloss(1), ctx.get_sphere_gloss(0))
    assert repr(before) == repr(after)
    # the ends of the range are accepted, and the getters return (1.0f + roughness) - 1.0f
    for rough in gloss_common.ROUGHNESSES + (0.3,):
        ctx.set_sphere_gloss(6, rough, (0.25, 0.5, 0.75))
        got_rough, got_refl = ctx.get_sphere_gloss(6)
        assert np.float32(got_rough) == gloss_ref.roughness_of(rough) and got_refl.tolist() == [0.25, 0.5, 0.75]
    ctx.set_sphere_gloss(6, 0.5, None)
    L = rwr.lib()
    assert L.rwr_scene_set_part_gloss(None, 0, None, C.c_float(0.5)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_scene_set_sphere_gloss(None, 0, None, C.c_float(0.5)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_scene_get_part_gloss(None, 0, None, None, None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_scene_get_sphere_gloss(None, 0, None, None, None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_last_gloss_stats(ctx._h, None) == rwr.ERR_INVALID_ARGUMENT


def test_a_surface_has_one_model(rwr, ctx, ref_loader, suzanne, cube):
    """Across all three setters, in both directions, parts and spheres."""
    s = gloss_common.scene("two_parts", rwr, ref_loader, suzanne, cube)
    cam_inv = gloss_common.camera(rwr, s)
    _upload(ctx, s, gloss=False)
    # the defaults, the getters
    assert ctx.get_part_gloss(0) is None and ctx.get_part_gloss(1) is None and all(ctx.get_sphere_gloss(i) is None for i in range(MAX_SPHERES))
    ctx.set_part_gloss(0)                       # roughness 0.25, reflectance 1, 1, 1
    rough, refl = ctx.get_part_gloss(0)
    assert rough == 0.25 and refl.tolist() == [1.0, 1.0, 1.0] and ctx.get_part_mirror(0) is None and ctx.get_part_glass(0) is None
    on, r, t = C.c_int(7), C.c_float(9.0), np.full(3, 9.0, np.float32)
    assert rwr.lib().rwr_scene_get_part_gloss(ctx._h, 1, C.byref(on), t.ctypes.data_as(C.c_void_p), C.byref(r)) == rwr.OK
    assert on.value == 0 and r.value == 0.0 and t.tolist() == [0.0, 0.0, 0.0]
    # a mirror or glass setter on a glossy surface clears the gloss, and the reverse - parts and spheres
    ctx.set_part_mirror(0, (0.5, 0.25, 1.0))
    assert ctx.get_part_gloss(0) is None and ctx.get_part_mirror(0).tolist() == [0.5, 0.25, 1.0]
    ctx.set_part_gloss(0, 0.5, (0.25, 0.5, 0.75))
    assert ctx.get_part_mirror(0) is None and ctx.get_part_glass(0) is None
    assert ctx.get_part_gloss(0)[0] == 0.5 and ctx.get_part_gloss(0)[1].tolist() == [0.25, 0.5, 0.75]
    ctx.set_part_glass(0, 2.0, (0.25, 0.5, 0.75))
    assert ctx.get_part_gloss(0) is None and ctx.get_part_mirror(0) is None and ctx.get_part_glass(0)[0] == 2.0
    ctx.set_part_gloss(0, 1.0, (0.0, 1.0, 0.5))
    assert ctx.get_part_glass(0) is None and ctx.get_part_mirror(0) is None and ctx.get_part_gloss(0)[0] == 1.0
    ctx.set_sphere_gloss(3, 2.0 ** -10, (0.0, 1.0, 0.5))
    ctx.set_sphere_mirror(3, (1.0, 1.0, 0.0))
    assert ctx.get_sphere_gloss(3) is None and ctx.get_sphere_mirror(3).tolist() == [1.0, 1.0, 0.0]
    ctx.set_sphere_gloss(3, 2.0 ** -10, (0.0, 1.0, 0.5))
    assert ctx.get_sphere_mirror(3) is None and ctx.get_sphere_gloss(3)[0] == 2.0 ** -10      # (next to a mirror's w = 1, and glossy all the same)
    ctx.set_sphere_glass(3, 1.0, (0.0, 1.0, 0.5))
    assert ctx.get_sphere_gloss(3) is None and ctx.get_sphere_glass(3)[0] == 1.0
    ctx.set_sphere_gloss(3, 1.0, (0.0, 1.0, 0.5))
    assert ctx.get_sphere_glass(3) is None and ctx.get_sphere_mirror(3) is None and ctx.get_sphere_gloss(3)[0] == 1.0
    # a refused call of one setter leaves the other model in place
    with pytest.raises(rwr.RwrError):
        ctx.set_sphere_mirror(3, (2.0, 0.0, 0.0))
    with pytest.raises(rwr.RwrError):
        ctx.set_sphere_glass(3, 5.0, (1.0, 1.0, 1.0))
    assert ctx.get_sphere_gloss(3)[1].tolist() == [0.0, 1.0, 0.5]
    ctx.set_part_mirror(1, (1.0, 1.0, 1.0))
    with pytest.raises(rwr.RwrError):
        ctx.set_part_gloss(1, 0.0, gloss_common.WHITE)
    assert ctx.get_part_mirror(1).tolist() == [1.0, 1.0, 1.0] and ctx.get_part_gloss(1) is None
    # the frame follows: part 1 as a glossy surface counts glossy rays, as a mirror or as glass it counts none
    b = s["bounces"]
    params = rwr.make_params(spp=2, max_bounces=b, seed=4, flags=_flags(rwr, b))
    ctx.set_part_gloss(0, 0.5, None)
    ctx.set_part_gloss(1, 0.25, gloss_common.WHITE)
    as_gloss = _frame(ctx, cam_inv, params)
    ctx.set_part_mirror(1, gloss_common.WHITE)
    as_mirror = _frame(ctx, cam_inv, params)
    ctx.set_part_glass(1, 1.5, gloss_common.WHITE)
    as_glass = _frame(ctx, cam_inv, params)
    assert as_gloss["glossy"] > 0 and as_mirror["glossy"] == 0 and as_glass["glossy"] == 0
    assert as_gloss["glass"] == (0, 0, 0) and as_mirror["glass"] == (0, 0, 0) and sum(as_glass["glass"]) > 0
    assert len({as_gloss["color_f32"].tobytes(), as_mirror["color_f32"].tobytes(), as_glass["color_f32"].tobytes()}) == 3
    # the sphere attributes persist across rwr_scene_set_spheres, the part attributes go with the scene
    ctx.set_part_gloss(1, 0.25, gloss_common.WHITE)
    ctx.set_spheres(rwr.make_spheres([]))
    assert ctx.get_sphere_gloss(3)[0] == 1.0
    ctx.upload_parts(s["model"])
    assert ctx.get_part_gloss(1) is None and ctx.get_part_mirror(1) is None and ctx.get_sphere_gloss(3) is not None
    ctx.set_sphere_gloss(3, 0.5, None)


def test_refusals(rwr, ctx, ref_loader, suzanne, cube):
    """RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes refuse the flag: whatever max_bounces is, gloss or no gloss."""
    s = gloss_common.scene("two_parts", rwr, ref_loader, suzanne, cube)
    cam_inv = gloss_common.camera(rwr, s)
    _upload(ctx, s)
    for gloss in (True, False):
        if not gloss:
            ctx.set_part_gloss(1, 0.5, None)
        for params in (rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_GLOSSY | rwr.FLAG_ORTHO_RAYS),
                       rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_GLOSSY | rwr.FLAG_USE_BVH),
                       rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_GLOSSY | rwr.FLAG_ORTHO_RAYS),
                       rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_GLOSSY | rwr.FLAG_USE_BVH)):
            with pytest.raises(rwr.RwrError) as ei:
                ctx.render(cam_inv, params)
            assert ei.value.code == rwr.ERR_UNSUPPORTED, params
        ctx.set_triangles(rwr.make_triangles([((0.0, 0.0, -2.0), (1.0, 0.0, -2.0), (0.0, 1.0, -2.0))]))
        try:
            for bounces in (0, 1):
                with pytest.raises(rwr.RwrError) as ei:
                    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=bounces, flags=rwr.FLAG_GLOSSY))
                assert ei.value.code == rwr.ERR_UNSUPPORTED
        finally:
            ctx.set_triangles(rwr.make_triangles())
    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=1, flags=rwr.FLAG_GLOSSY))   # the context is still usable
