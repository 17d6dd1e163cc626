"""Glass surfaces (RWR_FLAG_GLASS) on the GPU: the glass forms of the primary kernel and of the trace kernels' EMIT
forms against the tests' CPU reference (glass_ref.c):
  * sample-0 planes (object id, distance, depth) bit-exact; bounce-ray counts per call and the three event counts (Fresnel
    reflections, transmissions, total internal reflections) equal - every Fresnel decision and every refracted ray steers them;
    RGBA8 within one code; colour within the bar tests/test_gpu_multi_bounce.py holds deeper paths to (COLOR_TOL there, read from
    that file: a tint <= 1 travels through the same unorm16 throughput as an albedo), scaled by the sky's largest component as
    tests/test_gpu_sky.py scales it;
  * every schedule, split, frames in flight and accumulation: the same bytes;
  * frames the flag does nothing to, the setters, the accumulation key, the refusals.
The scenes are tests/glass_common.py's; tests/test_glass_host.py asserts with the reference alone that they exercise the glass."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import glass_common
import glass_ref
import path_cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# the colour bar of the deeper paths, for the same B: not a tolerance of this file's own
COLOR_TOL = float(re.search(r"^COLOR_TOL\s*=\s*([0-9.eE+-]+)", open(os.path.join(HERE, "test_gpu_multi_bounce.py")).read(), re.M).group(1))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
DEFAULT = (glass_ref.DEFAULT_ZENITH, glass_ref.DEFAULT_HORIZON)
BAR = COLOR_TOL * max(1.0, max(max(c) for c in DEFAULT))     # tests/test_gpu_sky.py's scaling: the default sky's components are <= 1
MAX_SPHERES = glass_ref.MAX_SPHERES


@pytest.fixture(scope="module")
def gref(tmp_path_factory):
    return glass_ref.lib(tmp_path_factory)


def _plain_spheres(c):
    for i in range(MAX_SPHERES):
        c.set_sphere_glass(i, 1.5, None)     # (either setter with None makes the surface diffuse)


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


def _flags(rwr, bounces, glass=True, mirrors=True, sky=True, shadows=False, extra=0):
    return (rwr.FLAG_AUX_OUTPUTS | extra | (rwr.FLAG_MULTI_BOUNCE if bounces > 1 else 0) | (rwr.FLAG_SHADOWS if shadows else 0) |
            (rwr.FLAG_SKY if sky else 0) | (rwr.FLAG_MIRRORS if mirrors else 0) | (rwr.FLAG_GLASS if glass else 0))


def _upload(c, s, surfaces=True):
    if isinstance(s["model"], (list, tuple)):
        c.upload_parts(s["model"])
    else:
        c.upload_model(s["model"])
    c.set_instances(s["instances"])
    c.set_spheres(s["spheres"])
    c.resize(s["w"], s["h"])
    _plain_spheres(c)
    if surfaces:
        for k, r in s["mirror_parts"].items():
            c.set_part_mirror(k, r)
        for k, r in s["mirror_spheres"].items():
            c.set_sphere_mirror(k, r)
        for k, (ior, tint) in s["glass_parts"].items():
            c.set_part_glass(k, ior, tint)
        for k, (ior, tint) in s["glass_spheres"].items():
            c.set_sphere_glass(k, ior, tint)


def _frame(c, cam_inv, params, **kw):
    c.render(cam_inv, params, **kw)
    out = c.readback(aux=True)
    out["stats"] = c.last_render_stats()
    out["shadow"] = c.last_shadow_stats()
    out["glass"] = c.last_glass_stats()
    return out


def _same(a, b, what=""):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _check(got, want, what):
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"glass colour error {what}: {err:.3g} (bar {BAR:.3g})")
    assert err <= BAR, (what, err)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, what


@pytest.mark.parametrize("spp", glass_common.SPPS)
@pytest.mark.parametrize("name", glass_common.GPU_SCENES)
def test_matches_the_reference(rwr, orc, gref, ctx, ref_loader, suzanne, cube, name, spp):
    s = glass_common.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = glass_common.camera(rwr, s)
    _upload(ctx, s)
    bounces, shadows = s["bounces"], spp == 2          # (the two-sample frames carry the shadow rays)
    got = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=bounces, seed=13, flags=_flags(rwr, bounces, shadows=shadows)))
    want = glass_common.reference(gref, rwr, orc, s, 13, spp, sky=DEFAULT, shadows=shadows, name=name)
    assert sum(want["events"]) > 0
    print(f"glass {name} spp {spp}: events {got['glass']} (reference {want['events']}), rays {got['stats'][1]} (reference {want['rays']})")
    # every Fresnel decision, and the count of rays that depend on where every refracted ray went
    assert got["glass"] == want["events"], (name, spp)
    assert got["stats"] == (s["w"] * s["h"] * spp, want["rays"]), (name, spp, want["gen_rays"].tolist())
    assert got["shadow"] == ((want["shadow_rays"], want["occluded"]) if shadows else (0, 0))
    _check(got, want, f"{name} spp={spp}")
    # sample-0 planes do not depend on the flag, nor does the first generation's ray count
    off = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=1, seed=13, flags=_flags(rwr, 1, glass=False, shadows=shadows)))
    for k in ("obj_id", "hit_t", "depth"):
        assert got[k].tobytes() == off[k].tobytes(), (name, k)
    assert off["stats"][1] == want["gen_rays"][1] and off["glass"] == (0, 0, 0)


_STATS = re.compile(r"rwr wavefront pools: packets (\d+) pools / (\d+) rays, per-lane (\d+) pools / (\d+) rays.*\n"
                    r"rwr wavefront launches: packet (\d+), per-lane (\d+), per-lane wide (\d+)")
# tests/test_gpu_fuzz.py's forced-packet schedule (tests/path_cases.py FORCED_SCHEDULE), its wide per-lane kernel, and the 256-thread
# per-lane kernel alone
SCHEDULES = {"packets": dict(path_cases.FORCED_SCHEDULE, RWR_WF_WIDE_LANE="0"),
             "wide lane": {"RWR_WF_GROUP": "5", "RWR_WF_PACKET_RAYS": "0", "RWR_WF_MIN_PACKET_POOLS": "100000", "RWR_WF_WIDE_LANE": "1"},
             "lane": {"RWR_WF_GROUP": "3", "RWR_WF_PACKET_RAYS": "0", "RWR_WF_MIN_PACKET_POOLS": "100000", "RWR_WF_WIDE_LANE": "0", "RWR_WF_OVERLAP": "2"}}


@pytest.mark.parametrize("name", glass_common.GPU_SCENES)
def test_schedules_give_the_same_frame(rwr, orc, gref, ctx, ref_loader, suzanne, cube, capfd, name):
    """Forced packets, the wide per-lane kernel asked for, the per-lane kernel alone: the default schedule's bytes and counts.
    Which kernels did run is read from the context's own account (RWR_WF_STATS=1, printed when it is destroyed)."""
    s = glass_common.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = glass_common.camera(rwr, s)
    spp = 7
    params = rwr.make_params(spp=spp, max_bounces=s["bounces"], seed=13, flags=_flags(rwr, s["bounces"], shadows=True))
    want = glass_common.reference(gref, rwr, orc, s, 13, spp, sky=DEFAULT, shadows=True, name=name)
    _upload(ctx, s)
    default = _frame(ctx, cam_inv, params)
    _check(default, want, f"schedule {name} default")
    assert default["stats"][1] == want["rays"] and default["glass"] == want["events"]
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
            assert got["stats"] == default["stats"] and got["glass"] == default["glass"] and got["shadow"] == default["shadow"], (name, what)
            m = _STATS.search(capfd.readouterr().err)
            assert m, (name, what)
            p_pools, p_rays, l_pools, l_rays, n_packet, n_lane, n_wide = map(int, m.groups())
            with capfd.disabled():
                print(f"glass schedule {name} {what}: packet pools {p_pools} ({p_rays} rays), per-lane pools {l_pools} ({l_rays} rays), "
                      f"launches packet {n_packet} / per-lane {n_lane} / wide {n_wide}")
            assert p_rays + l_rays == got["stats"][1], (name, what)     # every bounce ray went through a pool
            if what == "packets":
                assert n_packet > 0 and p_pools > 0, (name, what)
            else:
                assert n_lane + n_wide > 0 and (n_wide == 0 if what == "lane" else n_lane == 0 or n_wide == 0), (name, what)
                if what == "wide lane" and name in ("cube_room", "instances"):   # BVHs too large for a copy per 256-thread workgroup: the switch decides
                    assert n_wide > 0 and n_lane == 0, (name, what)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("name", glass_common.GPU_SCENES)
def test_accumulated_frames_are_one_frame_of_all_samples(rwr, ctx, ref_loader, suzanne, cube, name):
    s = glass_common.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = glass_common.camera(rwr, s)
    _upload(ctx, s)
    flags = _flags(rwr, s["bounces"])
    want = _frame(ctx, cam_inv, rwr.make_params(spp=6, max_bounces=s["bounces"], seed=11, flags=flags))
    ctx.accum_reset()
    acc = rwr.make_params(spp=2, max_bounces=s["bounces"], seed=11, flags=flags | rwr.FLAG_ACCUMULATE)
    events = np.zeros(3, np.int64)
    for k in range(1, 4):
        ctx.render(cam_inv, acc)
        assert ctx.accum_samples() == 2 * k
        events += np.asarray(ctx.last_glass_stats())      # (an accumulating frame counts its own samples)
    _same(ctx.readback(aux=True), want, "3 x 2 spp")
    assert tuple(events.tolist()) == want["glass"]


@pytest.mark.parametrize("name", glass_common.GPU_SCENES)
def test_strips_and_frames_in_flight(rwr, ctx, ref_loader, suzanne, cube, name):
    """Strips of two ranks assemble the frame (planes, ray counts, event counts); 1 to 3 frames in flight give its bytes."""
    s = glass_common.scene(name, rwr, ref_loader, suzanne, cube)
    h = s["h"]
    cam_inv = glass_common.camera(rwr, s)
    params = rwr.make_params(spp=3, max_bounces=s["bounces"], seed=2, flags=_flags(rwr, s["bounces"], shadows=True))
    _upload(ctx, s)
    full = _frame(ctx, cam_inv, params)
    assert sum(full["glass"]) > 0
    asm = {k: np.zeros_like(full[k]) for k in PLANES}
    rays, shadow, events = 0, np.zeros(2, np.int64), np.zeros(3, np.int64)
    for r in range(2):
        part = _frame(ctx, cam_inv, params, strips=(r, 2))
        rows = [y for y in range(h) if (y // 8) % 2 == r]
        rays += part["stats"][1]
        shadow += np.asarray(part["shadow"])
        events += np.asarray(part["glass"])
        for k in PLANES:
            asm[k][rows] = part[k][rows]
        ctx.dist_loopback_deposit(r, 2, True)
    ctx.dist_loopback_finish(2, True)
    _same(asm, full, (name, "strips"))
    assert rays == full["stats"][1] and tuple(shadow.tolist()) == full["shadow"] and tuple(events.tolist()) == full["glass"]
    assert np.array_equal(ctx.dist_readback(), full["color"]), name
    for n in (1, 2, 3):
        ctx.set_frames_in_flight(n)
        for i in range(n + 1):
            got = _frame(ctx, cam_inv, params)
            _same(got, full, (name, n, i))
            assert got["glass"] == full["glass"] and got["stats"] == full["stats"], (name, n, i)


def test_frames_the_flag_does_nothing_to(rwr, ctx, ref_loader, suzanne, cube):
    for name in ("cube_room", "facing_mirror", "inside_sphere"):
        s = glass_common.scene(name, rwr, ref_loader, suzanne, cube)
        cam_inv = glass_common.camera(rwr, s)
        b = s["bounces"]
        spp = 3
        with rwr.Context(0) as fresh:      # a context that never heard of glass (the scene's mirrors are set)
            _upload(fresh, dict(s, glass_parts={}, glass_spheres={}))
            never = {sh: _frame(fresh, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b, glass=False, shadows=sh)))
                     for sh in (False, True)}
            flat = {(n, sh): _frame(fresh, cam_inv, rwr.make_params(spp=n, max_bounces=0, seed=5, flags=_flags(rwr, 0, glass=False, shadows=sh)))
                    for n, sh in ((1, False), (4, False), (1, True))}
        _upload(ctx, s)
        for sh in (False, True):
            # glass surfaces without the flag are the diffuse surfaces they were
            off = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b, glass=False, shadows=sh)))
            _same(off, never[sh], (name, "flag off", sh))
            assert off["stats"] == never[sh]["stats"] and off["shadow"] == never[sh]["shadow"] and off["glass"] == (0, 0, 0)
            on = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b, shadows=sh)))
            assert on["color_f32"].tobytes() != off["color_f32"].tobytes() and sum(on["glass"]) > 0
            for k in ("depth", "obj_id", "hit_t"):
                assert on[k].tobytes() == off[k].tobytes(), (name, k)
            # ... and with the glass flag alone the scene's mirrors are the diffuse surfaces they were
            if s["mirror_parts"]:
                alone = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b, mirrors=False, shadows=sh)))
                assert alone["color_f32"].tobytes() != on["color_f32"].tobytes() and sum(alone["glass"]) > 0
        # no bounce: the flag is ignored (the reference frame at spp 1 too)
        for (n, sh), want in flat.items():
            on = _frame(ctx, cam_inv, rwr.make_params(spp=n, max_bounces=0, seed=5, flags=_flags(rwr, 0, shadows=sh)))
            _same(on, want, (name, "no bounce", n, sh))
            assert on["stats"] == want["stats"] and on["shadow"] == want["shadow"] and on["glass"] == (0, 0, 0)
        # every glass surface cleared again, then none ever set (a new upload): the flag alone changes nothing
        for k in s["glass_parts"]:
            ctx.set_part_glass(k, 1.5, None)
        for k in s["glass_spheres"]:
            ctx.set_sphere_glass(k, 1.5, None)
        for what in ("cleared", "never set"):
            if what == "never set":
                _upload(ctx, dict(s, glass_parts={}, glass_spheres={}))
            for sh in (False, True):
                on = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b, shadows=sh)))
                _same(on, never[sh], (name, what, sh))
                assert on["stats"] == never[sh]["stats"] and on["shadow"] == never[sh]["shadow"] and on["glass"] == (0, 0, 0)
        # glass on a sphere index the scene does not have is no glass of the scene
        ctx.set_sphere_glass(MAX_SPHERES - 1, 1.5, (1.0, 1.0, 1.0))
        on = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b)))
        _same(on, never[False], (name, "a sphere that is not there"))
        ctx.set_sphere_glass(MAX_SPHERES - 1, 1.5, None)


def test_setters_and_accumulation_key(rwr, ctx, ref_loader, suzanne, cube):
    """Every accepted call of a glass setter changes the scene's generation - with or without the flag, whether or not the value
    is new - and a refused call changes nothing; the flag (after its clearing rule) is one of the key's flags."""
    s = glass_common.scene("cube_room", rwr, ref_loader, suzanne, cube)
    cam_inv = glass_common.camera(rwr, s)
    _upload(ctx, s)
    b = s["bounces"]
    acc = rwr.make_params(spp=2, max_bounces=b, seed=11, flags=_flags(rwr, b) | rwr.FLAG_ACCUMULATE)
    off = rwr.make_params(spp=2, max_bounces=b, seed=11, flags=_flags(rwr, b, glass=False) | rwr.FLAG_ACCUMULATE)

    def step(params=acc):
        ctx.render(cam_inv, params)
        return ctx.accum_samples()

    ctx.accum_reset()
    assert step() == 2 and step() == 4
    ctx.set_part_glass(0, np.nextafter(np.float32(1.5), np.float32(2.0)), glass_common.CLEAR)     # one ulp of the index
    assert step() == 2 and step() == 4
    ctx.set_part_glass(0, 1.5, (1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 1.0))       # one ulp of the tint
    assert step() == 2 and step() == 4
    ctx.set_sphere_glass(5, 2.0, (0.5, 0.5, 0.5))                   # no sphere of this scene: the scene changed all the same
    assert step() == 2 and step() == 4
    ctx.set_sphere_glass(5, 2.0, (0.5, 0.5, 0.5))                   # the value it has already
    assert step() == 2 and step() == 4
    ctx.set_sphere_glass(5, 2.0, None)                              # clear
    assert step() == 2 and step() == 4
    assert step(off) == 2 and step(off) == 4                        # the flag toggled ...
    assert step() == 2                                              # ... and back
    assert step(off) == 2 and step(off) == 4
    ctx.set_part_glass(1, 1.2, (0.5, 0.5, 0.5))                     # with the flag off a setter still changes the scene
    assert step(off) == 2 and step(off) == 4
    # refused calls change nothing: the state, the accumulation - with the flag off and with it on
    before = (ctx.get_part_glass(0), ctx.get_part_glass(1), ctx.get_sphere_glass(0))
    bad_calls = [lambda: ctx.set_part_glass(0, 0.99, glass_common.CLEAR), lambda: ctx.set_part_glass(0, 4.5, glass_common.CLEAR),
                 lambda: ctx.set_part_glass(0, np.nan, glass_common.CLEAR), lambda: ctx.set_part_glass(0, np.inf, glass_common.CLEAR),
                 lambda: ctx.set_part_glass(0, 1.5, (2.0, 0.0, 0.0)), lambda: ctx.set_part_glass(0, 1.5, (0.5, -0.1, 0.5)),
                 lambda: ctx.set_part_glass(0, 1.5, (0.5, 0.5, np.nan)), lambda: ctx.set_part_glass(7, 1.5, glass_common.CLEAR),
                 lambda: ctx.set_part_glass(7, 1.5, None), lambda: ctx.set_sphere_glass(MAX_SPHERES, 1.5, glass_common.CLEAR),
                 lambda: ctx.set_sphere_glass(0, 0.5, glass_common.CLEAR), lambda: ctx.set_sphere_glass(0, 1.5, (np.inf, 0.0, 0.0)),
                 lambda: ctx.get_part_glass(7), lambda: ctx.get_sphere_glass(MAX_SPHERES)]
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
    after = (ctx.get_part_glass(0), ctx.get_part_glass(1), ctx.get_sphere_glass(0))
    assert repr(before) == repr(after)
    L = rwr.lib()
    assert L.rwr_scene_set_part_glass(None, 0, C.c_float(1.5), None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_scene_set_sphere_glass(None, 0, C.c_float(1.5), None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_scene_get_part_glass(None, 0, None, None, None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_scene_get_sphere_glass(None, 0, None, None, None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_last_glass_stats(ctx._h, None, None, None) == rwr.ERR_INVALID_ARGUMENT


def test_a_surface_has_one_model(rwr, ctx, ref_loader, suzanne, cube):
    s = glass_common.scene("cube_room", rwr, ref_loader, suzanne, cube)
    cam_inv = glass_common.camera(rwr, s)
    _upload(ctx, s, surfaces=False)
    # the defaults, the getters
    assert ctx.get_part_glass(0) is None and ctx.get_part_glass(1) is None and all(ctx.get_sphere_glass(i) is None for i in range(MAX_SPHERES))
    ctx.set_part_glass(0)                       # ior 1.5, tint 1, 1, 1
    ior, tint = ctx.get_part_glass(0)
    assert ior == 1.5 and tint.tolist() == [1.0, 1.0, 1.0] and ctx.get_part_mirror(0) is None
    on, i, t = C.c_int(7), C.c_float(9.0), np.full(3, 9.0, np.float32)
    assert rwr.lib().rwr_scene_get_part_glass(ctx._h, 1, C.byref(on), C.byref(i), t.ctypes.data_as(C.c_void_p)) == rwr.OK
    assert on.value == 0 and i.value == 0.0 and t.tolist() == [0.0, 0.0, 0.0]
    # a mirror setter on a glass surface clears the glass, and the reverse - parts and spheres
    ctx.set_part_mirror(0, (0.5, 0.25, 1.0))
    assert ctx.get_part_glass(0) is None and ctx.get_part_mirror(0).tolist() == [0.5, 0.25, 1.0]
    ctx.set_part_glass(0, 2.0, (0.25, 0.5, 0.75))
    assert ctx.get_part_mirror(0) is None and ctx.get_part_glass(0)[0] == 2.0 and ctx.get_part_glass(0)[1].tolist() == [0.25, 0.5, 0.75]
    ctx.set_sphere_glass(3, 4.0, (0.0, 1.0, 0.5))
    ctx.set_sphere_mirror(3, (1.0, 1.0, 0.0))
    assert ctx.get_sphere_glass(3) is None and ctx.get_sphere_mirror(3).tolist() == [1.0, 1.0, 0.0]
    ctx.set_sphere_glass(3, 1.0, (0.0, 1.0, 0.5))
    assert ctx.get_sphere_mirror(3) is None and ctx.get_sphere_glass(3)[0] == 1.0
    # a refused call of either setter leaves the other model in place
    with pytest.raises(rwr.RwrError):
        ctx.set_sphere_mirror(3, (2.0, 0.0, 0.0))
    assert ctx.get_sphere_glass(3)[1].tolist() == [0.0, 1.0, 0.5]
    ctx.set_part_mirror(1, (1.0, 1.0, 1.0))
    with pytest.raises(rwr.RwrError):
        ctx.set_part_glass(1, 5.0, glass_common.CLEAR)
    assert ctx.get_part_mirror(1).tolist() == [1.0, 1.0, 1.0] and ctx.get_part_glass(1) is None
    # the frame follows: part 0 as glass counts events, as a mirror it counts none
    b = s["bounces"]
    params = rwr.make_params(spp=2, max_bounces=b, seed=4, flags=_flags(rwr, b))
    ctx.set_part_mirror(1, None)
    as_glass = _frame(ctx, cam_inv, params)
    ctx.set_part_mirror(0, (1.0, 1.0, 1.0))
    as_mirror = _frame(ctx, cam_inv, params)
    assert sum(as_glass["glass"]) > 0 and as_mirror["glass"] == (0, 0, 0)
    assert as_glass["color_f32"].tobytes() != as_mirror["color_f32"].tobytes()
    # the sphere attributes persist across rwr_scene_set_spheres, the part attributes go with the scene
    ctx.set_spheres(rwr.make_spheres([]))
    assert ctx.get_sphere_glass(3)[0] == 1.0
    ctx.upload_parts(s["model"])
    assert ctx.get_part_glass(0) is None and ctx.get_part_mirror(0) is None and ctx.get_sphere_glass(3) is not None
    ctx.set_sphere_glass(3, 1.5, None)


def test_refusals(rwr, ctx, ref_loader, suzanne, cube):
    """RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes refuse the flag: whatever max_bounces is, glass or no glass."""
    s = glass_common.scene("cube_room", rwr, ref_loader, suzanne, cube)
    cam_inv = glass_common.camera(rwr, s)
    _upload(ctx, s)
    for glass in (True, False):
        if not glass:
            ctx.set_part_glass(0, 1.5, None)
        for params in (rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_GLASS | rwr.FLAG_ORTHO_RAYS),
                       rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_GLASS | rwr.FLAG_USE_BVH),
                       rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_GLASS | rwr.FLAG_ORTHO_RAYS),
                       rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_GLASS | rwr.FLAG_USE_BVH)):
            with pytest.raises(rwr.RwrError) as ei:
                ctx.render(cam_inv, params)
            assert ei.value.code == rwr.ERR_UNSUPPORTED, params
        ctx.set_triangles(rwr.make_triangles([((0.0, 0.0, -2.0), (1.0, 0.0, -2.0), (0.0, 1.0, -2.0))]))
        try:
            for bounces in (0, 1):
                with pytest.raises(rwr.RwrError) as ei:
                    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=bounces, flags=rwr.FLAG_GLASS))
                assert ei.value.code == rwr.ERR_UNSUPPORTED
        finally:
            ctx.set_triangles(rwr.make_triangles())
    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=1, flags=rwr.FLAG_GLASS))   # the context is still usable
