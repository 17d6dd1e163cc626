"""Emissive surfaces (RWR_FLAG_EMISSIVE) on the GPU: the GLOW forms of the primary kernel and of the two trace kernels
against the tests' CPU reference (emission_ref.c):
  * sample-0 planes (object id, distance, depth) bit-exact; ray, shadow, glass and gloss counts equal to the reference's AND to the
    same context's frame without the flag; emissive hits equal; RGBA8 within one code; colour within the bar
    tests/test_gpu_multi_bounce.py holds deeper paths to (COLOR_TOL there, read from that file) times max(1, the scene's largest Le
    component) - tests/test_gpu_sky.py's scaling rule: f32 error goes with magnitude;
  * every schedule, accumulation, strips, row bands and frames in flight: the same bytes;
  * frames the flag does nothing to, the setters and the keys, the refusals, the two post-processes.
The scenes are tests/emission_common.py's; tests/test_emission_host.py asserts with the reference alone that they exercise the rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref
import emission_common as ec
import emission_ref
import path_cases
import refusals_common
import reproject_ref as rr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# the colour bar of the deeper paths: not a tolerance of this file's own
COLOR_TOL = float(re.search(r"^COLOR_TOL\s*=\s*([0-9.eE+-]+)", open(os.path.join(HERE, "test_gpu_multi_bounce.py")).read(), re.M).group(1))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
COUNTS = ("stats", "shadow", "glass", "glossy")
MAX_SPHERES = emission_ref.MAX_SPHERES


@pytest.fixture(scope="module")
def eref(tmp_path_factory):
    return emission_ref.lib(tmp_path_factory)


def _plain_spheres(c):
    for i in range(MAX_SPHERES):
        c.set_sphere_gloss(i, 0.5, None)     # (any of the three model setters with None makes the surface diffuse)
        c.set_sphere_emission(i, None)


@pytest.fixture()
def ctx(gpu_ctx):
    """The shared context, left as it was found: default sky, plain dark spheres (the part attributes go with the next upload), no
    instances, no accumulation, one frame in flight."""
    gpu_ctx.sky_set_params()
    _plain_spheres(gpu_ctx)
    yield gpu_ctx
    gpu_ctx.sky_set_params()
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
    out["plan"] = c.last_traversal_plan()
    return out


def _same(a, b, what=""):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _same_counts(a, b, what="", emissive=True):
    for k in COUNTS + (("emissive",) if emissive else ()):
        assert a[k] == b[k], (what, k, a[k], b[k])


def _bar(s) -> float:
    return COLOR_TOL * max(1.0, ec.max_le(s))


def _check(got, want, what, bar):
    """tests/test_gpu_gloss.py's rule: planes bit for bit, colour within the bar, RGBA8 within one code."""
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"emission colour error {what}: {err:.3g} (bar {bar:.3g})")
    assert err <= bar, (what, err)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, what
    return err


def _params(rwr, s, spp, seed=13, emissive=True, bounces=None, extra=0):
    bounces = s["bounces"] if bounces is None else bounces
    return rwr.make_params(spp=spp, max_bounces=bounces, seed=seed, flags=ec.flags(rwr, s, bounces=bounces, emissive=emissive, extra=extra))


@pytest.mark.parametrize("spp", ec.SPPS)
@pytest.mark.parametrize("name", ec.SCENES)
def test_matches_the_reference(rwr, orc, eref, ctx, ref_loader, suzanne, cube, name, spp):
    s = ec.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = ec.camera(rwr, s)
    _upload(ctx, s)
    got = _frame(ctx, cam_inv, _params(rwr, s, spp))
    want = ec.reference(eref, rwr, orc, s, 13, spp, name)
    print(f"emission {name} spp {spp}: emissive hits {got['emissive']} (reference {want['emissive_hits']}: {want['gen_glow'].tolist()}), "
          f"rays {got['stats'][1]} (reference {want['rays']})")
    assert want["emissive_hits"] > 0
    assert got["emissive"] == want["emissive_hits"], (name, spp, want["gen_glow"].tolist())
    assert got["stats"] == (s["w"] * s["h"] * spp, want["rays"]), (name, spp, want["gen_rays"].tolist())
    assert got["shadow"] == ((want["shadow_rays"], want["occluded"]) if s["shadows"] else (0, 0))
    assert got["glass"] == want["events"] and got["glossy"] == want["glossy"], (name, spp)
    _check(got, want, f"{name} spp={spp}", _bar(s))
    # nothing but the sums moves: the same context's frame without the flag has the planes, the counts and the traversal plan
    off = _frame(ctx, cam_inv, _params(rwr, s, spp, emissive=False))
    for k in ("obj_id", "hit_t", "depth"):
        assert got[k].tobytes() == off[k].tobytes(), (name, k)
    _same_counts(got, off, (name, spp), emissive=False)
    assert got["plan"] == off["plan"] and off["emissive"] == 0
    assert got["color_f32"].tobytes() != off["color_f32"].tobytes()


_STATS = re.compile(r"rwr wavefront pools: packets (\d+) pools / (\d+) rays, per-lane (\d+) pools / (\d+) rays.*\n"
                    r"rwr wavefront launches: packet (\d+), per-lane (\d+), per-lane wide (\d+)")
# tests/path_cases.py FORCED_SCHEDULE's packets, the per-lane kernel alone, its wide form asked for, and 32-bit traversal stacks
_LANE = {"RWR_WF_GROUP": "5", "RWR_WF_PACKET_RAYS": "0", "RWR_WF_MIN_PACKET_POOLS": "100000"}
SCHEDULES = {"packets": dict(path_cases.FORCED_SCHEDULE, RWR_WF_WIDE_LANE="0"),
             "per lane": dict(_LANE, RWR_WF_WIDE_LANE="0"),
             "wide lane": dict(_LANE, RWR_WF_WIDE_LANE="1"),
             "stack32": {"RWR_WF_STACK16": "0"}}


@pytest.mark.parametrize("name", ("room", "instances"))
def test_schedules_give_the_same_frame(rwr, orc, eref, ctx, ref_loader, suzanne, cube, capfd, name):
    """Forced packets, the per-lane kernel alone, its wide form and 32-bit stacks: the default schedule's bytes, counts and emissive
    hits.  Which kernels did run is read from the context's own account (RWR_WF_STATS=1, printed when it is destroyed)."""
    s = ec.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = ec.camera(rwr, s)
    spp = 7
    params = _params(rwr, s, spp, extra=rwr.FLAG_SHADOWS)
    _upload(ctx, s)
    default = _frame(ctx, cam_inv, params)
    want = ec.reference(eref, rwr, orc, dict(s, shadows=True), 13, spp, name + " shadows")
    _check(default, want, f"schedule {name} default", _bar(s))
    assert default["stats"][1] == want["rays"] and default["emissive"] == want["emissive_hits"] > 0
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
                print(f"emission schedule {name} {what}: packet pools {p_pools} ({p_rays} rays), per-lane pools {l_pools} ({l_rays} rays), "
                      f"launches packet {n_packet} / per-lane {n_lane} / wide {n_wide}, plan {got['plan']}")
            assert p_rays + l_rays == got["stats"][1], (name, what)     # every bounce ray went through a pool
            if what == "packets":
                assert n_packet > 0 and p_pools > 0, (name, what)
            elif what in ("per lane", "wide lane"):
                assert p_pools == 0 and n_lane + n_wide > 0 and (n_lane == 0 or n_wide == 0), (name, what)
                if what == "per lane":
                    assert n_wide == 0, (name, what)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("name", ec.SCENES)
def test_accumulated_frames_are_one_frame_of_all_samples(rwr, ctx, ref_loader, suzanne, cube, name):
    s = ec.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = ec.camera(rwr, s)
    _upload(ctx, s)
    want = _frame(ctx, cam_inv, _params(rwr, s, 6, seed=11))
    ctx.accum_reset()
    acc = _params(rwr, s, 2, seed=11, extra=rwr.FLAG_ACCUMULATE)
    hits = 0
    for k in range(1, 4):
        ctx.render(cam_inv, acc)
        assert ctx.accum_samples() == 2 * k
        hits += ctx.last_emission_stats()      # (an accumulating frame counts its own samples)
    _same(ctx.readback(aux=True), want, "3 x 2 spp")
    assert hits == want["emissive"] > 0


@pytest.mark.parametrize("name", [n for n in ec.SCENES if n != "tiny"])   # (three rows are one strip: nothing to deal out)
def test_strips_bands_and_frames_in_flight(rwr, ctx, ref_loader, suzanne, cube, name):
    """Strips of two ranks and two row bands assemble the frame (planes, counts, emissive hits); 1 to 3 frames in flight give its bytes."""
    s = ec.scene(name, rwr, ref_loader, suzanne, cube)
    h = s["h"]
    cam_inv = ec.camera(rwr, s)
    params = _params(rwr, s, 3, seed=2, extra=rwr.FLAG_SHADOWS)
    _upload(ctx, s)
    full = _frame(ctx, cam_inv, params)
    assert full["emissive"] > 0
    asm = {k: np.zeros_like(full[k]) for k in PLANES}
    rays, shadow, hits = 0, np.zeros(2, np.int64), 0
    for r in range(2):
        part = _frame(ctx, cam_inv, params, strips=(r, 2))
        rows = [y for y in range(h) if (y // 8) % 2 == r]
        rays += part["stats"][1]
        shadow += np.asarray(part["shadow"])
        hits += part["emissive"]
        for k in PLANES:
            asm[k][rows] = part[k][rows]
        ctx.dist_loopback_deposit(r, 2, True)
    ctx.dist_loopback_finish(2, True)
    _same(asm, full, (name, "strips"))
    assert rays == full["stats"][1] and tuple(shadow.tolist()) == full["shadow"] and hits == full["emissive"]
    assert np.array_equal(ctx.dist_readback(), full["color"]), name
    asm = {k: np.zeros_like(full[k]) for k in PLANES}
    hits = 0
    for band in ((0, 16), (16, h)):
        part = _frame(ctx, cam_inv, params, rows=band)
        hits += part["emissive"]
        for k in PLANES:
            asm[k][band[0]:band[1]] = part[k][band[0]:band[1]]
    _same(asm, full, (name, "bands"))
    assert hits == full["emissive"]
    for n in (1, 2, 3):
        ctx.set_frames_in_flight(n)
        for i in range(n + 1):
            got = _frame(ctx, cam_inv, params)
            _same(got, full, (name, n, i))
            _same_counts(got, full, (name, n, i))


def test_frames_the_flag_does_nothing_to(rwr, ctx, ref_loader, suzanne, cube):
    """No emitter ever set, every Le zero, the emitter reset with None, an emitter on a sphere index the scene lacks: the frame without
    the flag byte for byte - at spp 1 without a bounce the reference frame - and no emissive hit."""
    for name in ("two_parts", "with_models", "spheres"):
        s = ec.scene(name, rwr, ref_loader, suzanne, cube)
        cam_inv = ec.camera(rwr, s)
        cases = ((3, None, 0), (1, 0, 0), (4, 0, 0), (1, 0, rwr.FLAG_SHADOWS))
        with rwr.Context(0) as fresh:      # a context on which no emission setter was ever called
            _upload(fresh, s, emitters=False)
            never = [_frame(fresh, cam_inv, _params(rwr, s, spp, seed=5, emissive=False, bounces=b, extra=x)) for spp, b, x in cases]
        _upload(ctx, s)
        on = _frame(ctx, cam_inv, _params(rwr, s, 3, seed=5))
        assert on["emissive"] > 0 and on["color_f32"].tobytes() != never[0]["color_f32"].tobytes()
        # an emitter shows at h0: the flag is not cleared at max_bounces 0, and such a frame is the integrator's at spp 1 too
        flat = _frame(ctx, cam_inv, _params(rwr, s, 1, seed=5, bounces=0))
        assert flat["emissive"] > 0 and flat["color_f32"].tobytes() != never[1]["color_f32"].tobytes()
        for k in ("depth", "obj_id", "hit_t"):
            assert flat[k].tobytes() == never[1][k].tobytes(), (name, k)

        def nothing(what):
            for (spp, b, x), want in zip(cases, never):
                for emissive in (True, False):
                    got = _frame(ctx, cam_inv, _params(rwr, s, spp, seed=5, emissive=emissive, bounces=b, extra=x))
                    _same(got, want, (name, what, spp, b, x, emissive))
                    _same_counts(got, want, (name, what, spp, b, x, emissive))
                    assert got["emissive"] == 0 and got["plan"] == want["plan"]

        for k in s["emissive_parts"]:
            ctx.set_part_emission(k, (0.0, 0.0, 0.0))
        for k in s["emissive_spheres"]:
            ctx.set_sphere_emission(k, (0.0, -0.0, 0.0))
        nothing("every Le zero")
        _upload(ctx, s)
        for k in s["emissive_parts"]:
            ctx.set_part_emission(k, None)
        for k in s["emissive_spheres"]:
            ctx.set_sphere_emission(k, None)
        nothing("reset with None")
        _upload(ctx, s, emitters=False)
        nothing("never set")
        ctx.set_sphere_emission(MAX_SPHERES - 1, (8.0, 8.0, 8.0))
        nothing("a sphere that is not there")
        ctx.set_sphere_emission(MAX_SPHERES - 1, None)


def test_setters_and_keys(rwr, ctx, ref_loader, suzanne, cube):
    """The ranges at both ends, the indices, refused calls change nothing, every accepted call restarts an accumulation and a
    reprojection history, and emission and the surface models leave each other alone."""
    s = ec.scene("two_parts", rwr, ref_loader, suzanne, cube)
    cam_inv = ec.camera(rwr, s)
    _upload(ctx, s)
    f32 = np.float32
    over, tiny = np.nextafter(f32(64.0), f32(65.0)), np.nextafter(f32(0.0), f32(1.0))
    # the ends of the range are accepted; -0.0 is accepted as 0: the surface does not emit
    ctx.set_part_emission(0, (0.0, 64.0, float(tiny)))
    assert ctx.get_part_emission(0).tolist() == [0.0, 64.0, float(tiny)]
    ctx.set_part_emission(0, (-0.0, 0.0, -0.0))
    assert ctx.get_part_emission(0) is None
    on, rad = C.c_int(7), np.full(3, 9.0, np.float32)
    assert rwr.lib().rwr_scene_get_part_emission(ctx._h, 0, C.byref(on), rad.ctypes.data_as(C.c_void_p)) == rwr.OK
    assert on.value == 0 and rad.tobytes() == np.zeros(3, np.float32).tobytes()      # (+0.0, on the bits)
    ctx.set_sphere_emission(MAX_SPHERES - 1, (64.0, 64.0, 64.0))
    assert ctx.get_sphere_emission(MAX_SPHERES - 1).tolist() == [64.0, 64.0, 64.0]
    ctx.set_sphere_emission(MAX_SPHERES - 1, None)
    assert ctx.get_sphere_emission(MAX_SPHERES - 1) is None and ctx.get_part_emission(1).tolist() == [2.0, 1.0, 0.5]

    acc = _params(rwr, s, 2, seed=11, extra=rwr.FLAG_ACCUMULATE)
    off = _params(rwr, s, 2, seed=11, emissive=False, extra=rwr.FLAG_ACCUMULATE)
    rep = _params(rwr, s, 2, seed=11, extra=rwr.FLAG_REPROJECT)

    def step(params=acc):
        ctx.render(cam_inv, params)
        return ctx.accum_samples()

    def history():
        ctx.render(cam_inv, rep)
        return ctx.reproject_frames()

    ctx.accum_reset()
    assert step() == 2 and step() == 4
    ctx.set_part_emission(1, (2.0, float(np.nextafter(f32(1.0), f32(2.0))), 0.5))     # one ulp of a component
    assert step() == 2 and step() == 4
    ctx.set_sphere_emission(5, (0.5, 0.5, 0.5))                 # no sphere of this scene: the scene changed all the same
    assert step() == 2 and step() == 4
    ctx.set_sphere_emission(5, (0.5, 0.5, 0.5))                 # the value it has already
    assert step() == 2 and step() == 4
    ctx.set_sphere_emission(5, None)
    assert step() == 2 and step() == 4
    assert step(off) == 2 and step(off) == 4                    # the flag toggled: its bit is part of the key ...
    assert step() == 2                                          # ... and back
    assert step(off) == 2
    ctx.set_part_emission(0, (1.0, 1.0, 1.0))                   # with the flag off a setter still changes the scene
    assert step(off) == 2 and step(off) == 4
    ctx.set_part_emission(0, None)
    assert history() == 1 and history() == 2                    # the reprojection history: the same rules
    ctx.set_part_emission(1, (2.0, 1.0, 0.5))
    assert history() == 1 and history() == 2
    ctx.set_part_emission(1, (2.0, 1.0, 0.5))
    assert history() == 1 and history() == 2
    # refused calls change nothing: the state, the accumulation, the history
    before = repr((ctx.get_part_emission(0), ctx.get_part_emission(1), ctx.get_sphere_emission(0)))
    bad_calls = [lambda: ctx.set_part_emission(1, (float(over), 0.0, 0.0)), lambda: ctx.set_part_emission(1, (0.0, -float(tiny), 0.0)),
                 lambda: ctx.set_part_emission(1, (0.0, 0.0, np.nan)), lambda: ctx.set_part_emission(1, (np.inf, 0.0, 0.0)),
                 lambda: ctx.set_part_emission(1, (0.0, -np.inf, 0.0)), lambda: ctx.set_part_emission(1, (-1.0, 1.0, 1.0)),
                 lambda: ctx.set_part_emission(2, (1.0, 1.0, 1.0)), lambda: ctx.set_part_emission(2, None),
                 lambda: ctx.set_sphere_emission(MAX_SPHERES, (1.0, 1.0, 1.0)), lambda: ctx.set_sphere_emission(MAX_SPHERES, None),
                 lambda: ctx.set_sphere_emission(0, (65.0, 0.0, 0.0)), lambda: ctx.get_part_emission(2), lambda: ctx.get_sphere_emission(MAX_SPHERES)]
    for bad in bad_calls:
        with pytest.raises(rwr.RwrError) as ei:
            bad()
        assert ei.value.code == rwr.ERR_INVALID_ARGUMENT
    assert history() == 3
    assert step() == 2 and step() == 4
    for bad in bad_calls:
        with pytest.raises(rwr.RwrError):
            bad()
    assert step() == 6
    assert repr((ctx.get_part_emission(0), ctx.get_part_emission(1), ctx.get_sphere_emission(0))) == before
    # emission survives the model setters, and the models survive the emission setters - parts and spheres
    ctx.set_part_mirror(1, (0.5, 0.25, 1.0))
    ctx.set_part_glass(1, 1.5, (1.0, 1.0, 1.0))
    ctx.set_part_gloss(1, 0.25, (1.0, 1.0, 1.0))
    assert ctx.get_part_emission(1).tolist() == [2.0, 1.0, 0.5] and ctx.get_part_gloss(1)[0] == 0.25
    ctx.set_part_emission(1, (3.0, 3.0, 3.0))
    assert ctx.get_part_gloss(1)[0] == 0.25 and ctx.get_part_emission(1).tolist() == [3.0, 3.0, 3.0]
    ctx.set_part_gloss(1, 0.5, None)
    assert ctx.get_part_emission(1).tolist() == [3.0, 3.0, 3.0]
    ctx.set_part_emission(1, None)
    ctx.set_sphere_mirror(3, (1.0, 1.0, 0.0))
    ctx.set_sphere_emission(3, (1.0, 2.0, 3.0))
    assert ctx.get_sphere_mirror(3).tolist() == [1.0, 1.0, 0.0] and ctx.get_sphere_emission(3).tolist() == [1.0, 2.0, 3.0]
    ctx.set_sphere_glass(3, 2.0, (1.0, 1.0, 1.0))
    ctx.set_sphere_mirror(3, None)
    assert ctx.get_sphere_emission(3).tolist() == [1.0, 2.0, 3.0]
    # the sphere attributes persist across rwr_scene_set_spheres, the part attributes go with the scene
    ctx.set_part_emission(1, (1.0, 1.0, 1.0))
    ctx.set_spheres(rwr.make_spheres([]))
    assert ctx.get_sphere_emission(3).tolist() == [1.0, 2.0, 3.0]
    ctx.upload_parts(s["model"])
    assert ctx.get_part_emission(1) is None and ctx.get_sphere_emission(3) is not None
    ctx.set_sphere_emission(3, None)
    L = rwr.lib()
    assert L.rwr_scene_set_part_emission(None, 0, None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_scene_set_sphere_emission(None, 0, None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_scene_get_part_emission(None, 0, None, None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_scene_get_sphere_emission(None, 0, None, None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_last_emission_stats(ctx._h, None) == rwr.ERR_INVALID_ARGUMENT


def test_refusals(rwr, ctx, ref_loader, suzanne, cube):
    """RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes refuse the flag - the code and the message - whatever
    max_bounces is and whether or not anything emits."""
    s = ec.scene("two_parts", rwr, ref_loader, suzanne, cube)
    cam_inv = ec.camera(rwr, s)
    _upload(ctx, s)
    text = refusals_common.OFF_REFERENCE % "EMISSIVE"
    for emitters in (True, False):
        if not emitters:
            ctx.set_part_emission(1, None)
        for params in (rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_EMISSIVE | rwr.FLAG_ORTHO_RAYS),
                       rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_EMISSIVE | rwr.FLAG_USE_BVH),
                       rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_EMISSIVE | rwr.FLAG_ORTHO_RAYS)):
            with pytest.raises(rwr.RwrError) as ei:
                ctx.render(cam_inv, params)
            assert ei.value.code == rwr.ERR_UNSUPPORTED and text in str(ei.value), (params, str(ei.value))
        ctx.set_triangles(rwr.make_triangles([((0.0, 0.0, -2.0), (1.0, 0.0, -2.0), (0.0, 1.0, -2.0))]))
        try:
            for bounces in (0, 1):
                with pytest.raises(rwr.RwrError) as ei:
                    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=bounces, flags=rwr.FLAG_EMISSIVE))
                assert ei.value.code == rwr.ERR_UNSUPPORTED and text in str(ei.value), str(ei.value)
        finally:
            ctx.set_triangles(rwr.make_triangles())
    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=1, flags=rwr.FLAG_EMISSIVE))   # the context is still usable


def test_the_denoiser_filters_the_emissive_frame(rwr, orc, eref, ctx, ref_loader, suzanne, cube, tmp_path_factory):
    """With RWR_FLAG_DENOISE the frame of `room` is denoise_ref.c applied to the emission reference's planes, within the colour bar."""
    dref = denoise_ref.lib(tmp_path_factory)
    s = ec.scene("room", rwr, ref_loader, suzanne, cube)
    cam_inv = ec.camera(rwr, s)
    _upload(ctx, s)
    ref = ec.reference(eref, rwr, orc, s, 9, 4, "room")
    nhat = denoise_ref.face_normals(dref, orc, s["model"], None)
    want = denoise_ref.denoise(dref, ref["color_f32"], ref["obj_id"], ref["hit_t"], nhat, **denoise_ref.DEFAULTS)
    ctx.set_denoise_params()
    plain = _frame(ctx, cam_inv, _params(rwr, s, 4, seed=9))
    got = _frame(ctx, cam_inv, _params(rwr, s, 4, seed=9, extra=rwr.FLAG_DENOISE))
    assert got["emissive"] == plain["emissive"] == ref["emissive_hits"] > 0
    _check(got, dict(ref, color_f32=want["color_f32"], color=want["color"]), "room denoised", _bar(s))
    assert got["color_f32"].tobytes() != plain["color_f32"].tobytes()              # the filter ran


def test_reprojection_blends_the_emissive_frames(rwr, orc, eref, ref_loader, suzanne, cube, tmp_path_factory):
    """Two reprojecting frames of `room` are the emissive frames of seed and seed + 1 (each against the CPU reference) blended by
    reproject_ref.c."""
    s = ec.scene("room", rwr, ref_loader, suzanne, cube)
    cam_inv = ec.camera(rwr, s)
    cam = cam_inv.view(rwr.CAMERA_INV_DTYPE)
    seed, spp = 21, 2
    L = rr.lib(tmp_path_factory)
    nhat = denoise_ref.face_normals(denoise_ref.lib(tmp_path_factory), orc, s["model"], None)
    with rwr.Context(0) as B:
        _upload(B, s)
        plains = [_frame(B, cam_inv, _params(rwr, s, spp, seed=seed + k)) for k in range(2)]
    for k, f in enumerate(plains):
        _check(f, ec.reference(eref, rwr, orc, s, seed + k, spp, "room"), f"reproject plain {k}", _bar(s))
    chain = rr.chain(L, plains, nhat, [cam, cam])
    with rwr.Context(0) as A:
        _upload(A, s)
        params = _params(rwr, s, spp, seed=seed, extra=rwr.FLAG_REPROJECT)
        for k in range(2):
            A.render(cam, params)
            got = A.readback(aux=True)
            assert A.reproject_frames() == k + 1 and A.last_emission_stats() == plains[k]["emissive"] > 0
            for p in ("depth", "obj_id", "hit_t"):
                assert got[p].tobytes() == plains[k][p].tobytes(), (k, p)
            err = float(np.abs(got["color_f32"] - chain[k]["color_f32"]).max())
            print(f"emission reprojection frame {k}: colour error {err:.3g}")
            assert err <= _bar(s), (k, err)
            assert np.abs(got["color"].astype(int) - chain[k]["color"].astype(int)).max() <= 1
            assert A.reproject_history().tobytes() == chain[k]["n"].tobytes()
