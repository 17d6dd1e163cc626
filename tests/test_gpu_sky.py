"""Sky light (RWR_FLAG_SKY) on the GPU: the trace kernels' SKY forms against the tests' CPU reference (sky_ref.c):
  * sample-0 planes (object id, distance, depth) bit-exact, colour within the bar tests/test_gpu_multi_bounce.py holds deeper
    paths to (COLOR_TOL there, read from that file: the default sky's components are <= 1, the magnitude of E), ray and shadow
    counts equal;
  * every schedule, split, frames in flight and accumulation: the same bytes;
  * frames the flag does nothing to, the refusals, the parameters, the denoiser behind it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref
import shadow_common
import sky_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# the colour bar of the deeper paths, for the same B: not a tolerance of this file's own
COLOR_TOL = float(re.search(r"^COLOR_TOL\s*=\s*([0-9.eE+-]+)", open(os.path.join(HERE, "test_gpu_multi_bounce.py")).read(), re.M).group(1))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
DEFAULT = (sky_ref.DEFAULT_ZENITH, sky_ref.DEFAULT_HORIZON)
_cache = {}


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return sky_ref.lib(tmp_path_factory)


@pytest.fixture()
def ctx(gpu_ctx):
    """The shared context, left as it was found: default sky, no instances, no accumulation."""
    gpu_ctx.sky_set_params()
    yield gpu_ctx
    gpu_ctx.sky_set_params()
    gpu_ctx.set_instances(None)
    gpu_ctx.accum_reset()


def _soup(ref_loader, cube):
    """About 60 triangles of all sizes and orientations in a box around the origin."""
    rng = np.random.default_rng(11)
    centre = rng.uniform(-1.2, 1.2, size=(60, 1, 3))
    tris = centre + rng.normal(scale=0.45, size=(60, 3, 3))
    return shadow_common.triangle_model(ref_loader, [tuple(map(tuple, t)) for t in tris.astype(np.float32)], cube["texture"])


def _scene(name, rwr, ref_loader, suzanne, cube):
    """(model, spheres, instances, eye, target, w, h, spp, bounces)"""
    if name == "cube_b1":
        return cube, rwr.make_spheres([]), None, (1.0, 0.8, 1.4), (0, 0, 0), 64, 48, 4, 1
    if name == "cube_b8":
        return cube, rwr.make_spheres([]), None, (1.0, 0.8, 1.4), (0, 0, 0), 64, 48, 4, 8
    if name == "soup":       # an odd size: partial tiles
        if "soup" not in _cache:
            _cache["soup"] = _soup(ref_loader, cube)
        return _cache["soup"], rwr.make_spheres([((0.9, 0.4, 0.6), 0.5), ((-0.8, -0.5, 0.2), 0.35)]), None, (0.3, 0.5, 2.2), (0, 0, 0), 37, 29, 5, 3
    if name == "cube_grid":  # 64 samples: pools dense enough for the packet kernel
        return cube, rwr.make_spheres([]), rwr.make_instance_grid(2, 3.0), (-1.5, 1.5, 2.5), (-1.5, 0.0, -1.5), 64, 48, 64, 2
    if name == "suzanne_far":
        return suzanne, rwr.make_spheres(), None, (0, 0, 3), (0, 0, -1), 200, 72, 7, 2
    if name == "suzanne_grid":
        return suzanne, rwr.make_spheres(), rwr.make_instance_grid(4, 3.0), (0, 0, 12), (0, 0, -1), 256, 80, 6, 2
    raise KeyError(name)


def _cam(rwr, s):
    return rwr.camera_build_inv_uniform(rwr.make_camera(eye=s[3], target=s[4], aspect=s[5] / s[6]))


def _flags(rwr, bounces, sky=True, shadows=False, extra=0):
    return (rwr.FLAG_AUX_OUTPUTS | extra | (rwr.FLAG_MULTI_BOUNCE if bounces > 1 else 0) | (rwr.FLAG_SHADOWS if shadows else 0) |
            (rwr.FLAG_SKY if sky else 0))


def _upload(c, s):
    c.upload_model(s[0])
    c.set_instances(s[2])
    c.set_spheres(s[1])
    c.resize(s[5], s[6])


def _frame(c, cam_inv, params, **kw):
    c.render(cam_inv, params, **kw)
    out = c.readback(aux=True)
    out["stats"] = c.last_render_stats()
    out["shadow"] = c.last_shadow_stats()
    return out


def _same(a, b, what=""):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _reference(sref, orc, s, cam_inv, seed, sky, shadows=False):
    key = (id(s[0]), s[3], s[5], s[6], s[7], s[8], seed, sky, shadows)
    if key not in _cache:
        inst = None if s[2] is None else s[2].view(orc.INSTANCE_DTYPE)
        _cache[key] = sky_ref.render_path(sref, orc, cam_inv.view(orc.CAMERA_INV_DTYPE), orc.make_screen(s[5], s[6]),
                                          orc.make_params(s[7], s[8], seed=seed), s[1].view(orc.SPHERE_DTYPE), s[0], instances=inst,
                                          shadows=shadows, sky=sky)
    return _cache[key]


def _check(got, want, what):
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"sky colour error {what}: {err:.3g}")
    assert err <= COLOR_TOL, (what, err)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, what


@pytest.mark.parametrize("shadows", [False, True], ids=["plain", "shadows"])
@pytest.mark.parametrize("name", ["cube_b1", "cube_b8", "soup", "cube_grid"])
def test_matches_the_reference(rwr, orc, sref, ctx, ref_loader, suzanne, cube, name, shadows):
    s = _scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = _cam(rwr, s)
    _upload(ctx, s)
    spp, bounces = s[7], s[8]
    got = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=bounces, seed=13, flags=_flags(rwr, bounces, shadows=shadows)))
    want = _reference(sref, orc, s, cam_inv, 13, DEFAULT, shadows)
    off = _reference(sref, orc, s, cam_inv, 13, None, shadows)
    assert want["sky_terms"] > 0 and not np.array_equal(want["color_f32"], off["color_f32"])    # the scene does see the sky
    if name.startswith("cube_b"):
        assert want["sky_terms"] == want["rays"]                                                 # a lone convex mesh: every bounce ray leaves
    else:
        first = int(round(float(want["color_f32"][..., 3].sum()) / 2.0 * spp))                   # (alpha / 2 counts the primary hits)
        assert want["sky_terms"] < want["rays"] and want["rays"] > first                          # bounce rays that hit, paths that go on
    _check(got, want, f"{name} shadows={shadows}")
    assert got["stats"] == (s[5] * s[6] * spp, want["rays"])
    assert got["shadow"] == ((want["shadow_rays"], want["occluded"]) if shadows else (0, 0))
    # another sky, components above 1 and a zero.  COLOR_TOL is the bar for terms T * L with |L| <= 1 (E, the default sky).  A sky
    # term's error - the unorm16 throughput times S, the f32 rounding of S and of T * S - is relative to S, and S lies between the
    # two colours, so the same bar scaled by the largest component of this sky (3.5) bounds it; every other term is as before.
    tinted = ((0.25, 2.0, 0.0), (3.5, 0.5, 0.125))
    bar = COLOR_TOL * max(1.0, max(max(c) for c in tinted))
    ctx.sky_set_params(*tinted)
    got = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=bounces, seed=13, flags=_flags(rwr, bounces, shadows=shadows)))
    want = _reference(sref, orc, s, cam_inv, 13, tinted, shadows)
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (name, k)
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"sky colour error {name} shadows={shadows} tinted sky: {err:.3g} (bar {bar:.3g}, the default sky's {COLOR_TOL:.3g})")
    assert err <= bar, (name, err)


_STATS = re.compile(r"rwr wavefront pools: packets (\d+) pools / (\d+) rays, per-lane (\d+) pools / (\d+) rays.*\n"
                    r"rwr wavefront launches: packet (\d+), per-lane (\d+), per-lane wide (\d+)")


@pytest.mark.parametrize("name", ["suzanne_far", "suzanne_grid"])
def test_schedules_give_the_same_frame(rwr, orc, sref, ref_loader, suzanne, cube, capfd, name):
    """The schedule overrides of test_schedules_of_the_integrator_give_the_same_frame (tests/test_gpu_path.py), with the wide
    per-lane kernel switched as tests/test_gpu_multi_bounce.py switches it: packets forced (dense 40 / 400, no minimum of packet
    pools), per-lane forced (no dense rule, a minimum of 128 packet pools), the 1 024-thread LDS form on and off.  B = 2: the EMIT
    forms and the path-ending forms both run.  Which kernels did run is read from the context's own account (RWR_WF_STATS=1, printed
    when it is destroyed): the pools the sort classed as packets / per-lane and the launches of each trace kernel."""
    s = _scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = _cam(rwr, s)
    params = rwr.make_params(spp=s[7], max_bounces=s[8], seed=3, flags=_flags(rwr, s[8]))
    want = _reference(sref, orc, s, cam_inv, 3, DEFAULT)
    keys = ("RWR_WF_ZSPLIT", "RWR_WF_OVERLAP", "RWR_WF_GROUP", "RWR_WF_PACKET_RAYS", "RWR_WF_MIN_PACKET_POOLS", "RWR_WF_WIDE_LANE", "RWR_WF_STATS")
    saved = {k: os.environ.get(k) for k in keys}
    ran = {"packet": False, "lane": False, "wide": False}
    try:
        with rwr.Context(0) as c:
            _upload(c, s)
            default = _frame(c, cam_inv, params)
        _check(default, want, f"schedule {name} default")
        assert default["stats"][1] == want["rays"]
        capfd.readouterr()
        for zsplit, queues, group, dense, wide in (("1", "1", "32", "0", "0"), ("4", "1", "32", "0", "1"), ("3", "2", "2", "0", "0"),
                                                   ("1", "2", "3", "0", "1"), ("0", "4", "1", "0", "0"), ("8", "3", "4", "0", "1"),
                                                   ("1", "1", "32", "40", "0"), ("4", "2", "4", "400", "1")):
            os.environ.update({"RWR_WF_ZSPLIT": zsplit, "RWR_WF_OVERLAP": queues, "RWR_WF_GROUP": group, "RWR_WF_PACKET_RAYS": dense,
                               "RWR_WF_MIN_PACKET_POOLS": "0" if dense != "0" else "128", "RWR_WF_WIDE_LANE": wide, "RWR_WF_STATS": "1"})
            what = (zsplit, queues, group, dense, wide)
            with rwr.Context(0) as c:        # the tunables are read when the context is created
                _upload(c, s)
                got = _frame(c, cam_inv, params)
                again = _frame(c, cam_inv, params)   # (zsplit 0: now from the first frame's live count)
                band = _frame(c, cam_inv, params, rows=(24, 56))
            _same(got, default, what)
            _same(again, default, what)
            for k in PLANES:
                assert got[k][24:56].tobytes() == band[k][24:56].tobytes(), (what, k, "band")
            assert got["stats"] == default["stats"], what
            m = _STATS.search(capfd.readouterr().err)
            assert m, what
            p_pools, p_rays, l_pools, l_rays, n_packet, n_lane, n_wide = map(int, m.groups())
            with capfd.disabled():
                print(f"schedule {name} {what}: packet pools {p_pools} ({p_rays} rays), per-lane pools {l_pools} ({l_rays} rays), "
                      f"launches packet {n_packet} / per-lane {n_lane} / wide {n_wide}")
            assert p_rays + l_rays == 2 * got["stats"][1] + band["stats"][1], what     # every bounce ray went through a pool
            # rays the packet kernel traced: no minimum of packet pools, so it took whatever the sort classed as packets (a frame
            # may have no pool of 400 rays: at least one of the two settings has to force packets, checked at the end)
            if dense != "0" and p_pools > 0:
                assert n_packet > 0, what
                ran["packet"] = True
            # rays the per-lane kernel traced: pools classed per-lane, or (with the minimum of 128) fewer packet pools than that
            # over all launches together, so in every one of them the per-lane kernel took them
            if l_pools > 0 or (dense == "0" and p_pools < 128):
                assert n_wide + n_lane > 0, what
                ran["wide" if n_wide > 0 else "lane"] = True
            assert (n_wide == 0) if wide == "0" else (n_lane == 0 or n_wide == 0), what
            if name == "suzanne_grid":   # 508 nodes: too large for a copy per 256-thread workgroup, so the switch decides
                assert (n_wide > 0 and n_lane == 0) if wide == "1" else (n_lane > 0 and n_wide == 0), what
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert ran["packet"] and ran["lane"], ran
    if name == "suzanne_grid":
        assert ran["wide"], ran


@pytest.mark.parametrize("split", ["strips", "bands", "in_flight"])
def test_splits_assemble_the_frame(rwr, suzanne, split):
    w, h = 203, 67
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0.3, 0.2, 2.6), aspect=w / h))
    params = rwr.make_params(spp=3, max_bounces=2, seed=2, flags=_flags(rwr, 2, shadows=True))
    with rwr.Context(0) as c:
        c.upload_model(suzanne)
        c.set_spheres(rwr.make_spheres())
        c.resize(w, h)
        full = _frame(c, cam_inv, params)
        c.render(cam_inv, rwr.make_params(spp=3, max_bounces=2, seed=2, flags=_flags(rwr, 2, sky=False, shadows=True)))
        assert c.readback(aux=True)["color_f32"].tobytes() != full["color_f32"].tobytes()      # the sky is in the frame
        if split == "in_flight":
            for n in (1, 2, 3):
                c.set_frames_in_flight(n)
                for i in range(n + 1):
                    _same(_frame(c, cam_inv, params), full, (n, i))
            return
        for n in (2, 3):
            asm = {k: np.zeros_like(full[k]) for k in PLANES}
            rays, shadow = 0, [0, 0]
            for r in range(n):
                if split == "strips":
                    part = _frame(c, cam_inv, params, strips=(r, n))
                    rows = [y for y in range(h) if (y // 8) % n == r]
                else:
                    band = rwr.dist_band(r, n, h)
                    part = _frame(c, cam_inv, params, rows=band)
                    rows = list(range(*band))
                rays += part["stats"][1]
                shadow[0] += part["shadow"][0]; shadow[1] += part["shadow"][1]
                for k in PLANES:
                    asm[k][rows] = part[k][rows]
                c.dist_loopback_deposit(r, n, split == "strips")
            c.dist_loopback_finish(n, split == "strips")
            _same(asm, full, (split, n))
            assert rays == full["stats"][1] and tuple(shadow) == full["shadow"]
            assert np.array_equal(c.dist_readback(), full["color"]), (split, n)


def test_accumulation_and_its_key(rwr, ctx, suzanne):
    w, h = 120, 64
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0.3, 0.2, 2.6), aspect=w / h))
    ctx.upload_model(suzanne); ctx.set_instances(None); ctx.set_spheres(rwr.make_spheres()); ctx.resize(w, h)
    flags = _flags(rwr, 2)
    want = _frame(ctx, cam_inv, rwr.make_params(spp=8, max_bounces=2, seed=11, flags=flags))
    ctx.accum_reset()
    acc = rwr.make_params(spp=2, max_bounces=2, seed=11, flags=flags | rwr.FLAG_ACCUMULATE)
    for k in range(1, 5):
        ctx.render(cam_inv, acc)
        assert ctx.accum_samples() == 2 * k
    _same(ctx.readback(aux=True), want, "4 x 2 spp")
    # one ulp in one component of the sky is another image: the accumulation starts over
    zenith = ctx.sky_get_params()["zenith"]
    zenith[1] = np.nextafter(zenith[1], np.float32(2.0))
    ctx.sky_set_params(zenith=zenith)
    ctx.render(cam_inv, acc)
    assert ctx.accum_samples() == 2
    ctx.render(cam_inv, acc)
    assert ctx.accum_samples() == 4
    # setting the same values again is no change
    ctx.sky_set_params(zenith=zenith)
    ctx.render(cam_inv, acc)
    assert ctx.accum_samples() == 6
    # without the flag the sky is no part of the frame: its parameters may change under a running accumulation
    ctx.accum_reset()
    plain = rwr.make_params(spp=2, max_bounces=2, seed=11, flags=_flags(rwr, 2, sky=False) | rwr.FLAG_ACCUMULATE)
    ctx.render(cam_inv, plain)
    assert ctx.accum_samples() == 2
    ctx.sky_set_params(zenith=(0.0, 0.25, 9.0), horizon=(4.0, 0.0, 0.5))
    ctx.render(cam_inv, plain)
    assert ctx.accum_samples() == 4
    ctx.sky_set_params()
    ctx.render(cam_inv, plain)
    assert ctx.accum_samples() == 6
    # nor at max_bounces = 0, where the flag is ignored
    ctx.accum_reset()
    flat = rwr.make_params(spp=2, max_bounces=0, seed=11, flags=rwr.FLAG_AUX_OUTPUTS | rwr.FLAG_SKY | rwr.FLAG_ACCUMULATE)
    ctx.render(cam_inv, flat)
    ctx.sky_set_params(zenith=(1.0, 2.0, 3.0))
    ctx.render(cam_inv, flat)
    assert ctx.accum_samples() == 4


def test_frames_the_flag_does_nothing_to(rwr, ctx, ref_loader, suzanne, cube):
    for name in ("cube_grid", "suzanne_far"):
        s = _scene(name, rwr, ref_loader, suzanne, cube)
        cam_inv = _cam(rwr, s)
        _upload(ctx, s)
        # a black sky, at one bounce and deeper, with and without shadow rays
        ctx.sky_set_params(zenith=(0, 0, 0), horizon=(0, 0, 0))
        for spp, bounces, shadows in ((5, 1, False), (5, 3, False), (5, 3, True)):
            off = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=bounces, seed=5, flags=_flags(rwr, bounces, sky=False, shadows=shadows)))
            on = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=bounces, seed=5, flags=_flags(rwr, bounces, shadows=shadows)))
            _same(on, off, (name, "black", spp, bounces, shadows))
            assert on["stats"] == off["stats"] and on["shadow"] == off["shadow"]
        # no bounce: the flag is ignored whatever the sky (the reference frame at spp 1 too)
        ctx.sky_set_params(zenith=(16, 16, 16), horizon=(16, 16, 16))
        for spp, shadows in ((1, False), (4, False), (1, True)):
            off = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=0, seed=5, flags=_flags(rwr, 0, sky=False, shadows=shadows)))
            on = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=0, seed=5, flags=_flags(rwr, 0, shadows=shadows)))
            _same(on, off, (name, "no bounce", spp, shadows))
            assert on["stats"] == off["stats"] and on["shadow"] == off["shadow"]
        # the brightest sky allowed does light the frame, and only where something was hit
        off = _frame(ctx, cam_inv, rwr.make_params(spp=4, max_bounces=1, seed=5, flags=_flags(rwr, 1, sky=False)))
        on = _frame(ctx, cam_inv, rwr.make_params(spp=4, max_bounces=1, seed=5, flags=_flags(rwr, 1)))
        for k in ("depth", "obj_id", "hit_t"):
            assert on[k].tobytes() == off[k].tobytes(), k
        assert (on["color_f32"] >= off["color_f32"]).all() and (on["color_f32"] > off["color_f32"]).any()
        nothing = off["color_f32"][..., 3] == 0
        assert nothing.any() and np.array_equal(on["color_f32"][nothing], off["color_f32"][nothing])


def test_parameters_and_refusals(rwr, ctx, suzanne):
    L = rwr.lib()
    assert np.allclose(ctx.sky_get_params()["zenith"], sky_ref.DEFAULT_ZENITH) and np.allclose(ctx.sky_get_params()["horizon"], sky_ref.DEFAULT_HORIZON)
    ctx.sky_set_params(zenith=(0.0, 16.0, 0.5))
    ctx.sky_set_params(horizon=(2.0, 0.25, 0.0))
    kept = ctx.sky_get_params()
    assert kept["zenith"].tolist() == [0.0, 16.0, 0.5] and kept["horizon"].tolist() == [2.0, 0.25, 0.0]
    for bad in (np.nan, np.inf, -np.inf, -1e-6, np.nextafter(np.float32(16.0), np.float32(17.0)), 1e30):
        for field in ("zenith", "horizon"):
            for c in range(3):
                v = kept[field].copy()
                v[c] = bad
                with pytest.raises(rwr.RwrError) as ei:
                    ctx.sky_set_params(**{field: v})
                assert ei.value.code == rwr.ERR_INVALID_ARGUMENT, (field, c, bad)
                now = ctx.sky_get_params()
                assert now["zenith"].tobytes() == kept["zenith"].tobytes() and now["horizon"].tobytes() == kept["horizon"].tobytes()
    p = np.zeros(1, rwr.SKY_PARAMS_DTYPE)
    assert L.rwr_sky_set_params(None, p.ctypes.data_as(C.c_void_p)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_sky_get_params(None, p.ctypes.data_as(C.c_void_p)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_sky_get_params(ctx._h, None) == rwr.ERR_INVALID_ARGUMENT
    ctx.sky_set_params()     # NULL: the defaults
    assert np.allclose(ctx.sky_get_params()["zenith"], sky_ref.DEFAULT_ZENITH) and np.allclose(ctx.sky_get_params()["horizon"], sky_ref.DEFAULT_HORIZON)
    # reference-frame-only modes refuse the flag
    w, h = 64, 48
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0, 0, 3), aspect=w / h))
    ctx.upload_model(suzanne); ctx.set_instances(None); ctx.set_spheres(rwr.make_spheres()); ctx.resize(w, h)
    for params in (rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_SKY | rwr.FLAG_ORTHO_RAYS),
                   rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_SKY | rwr.FLAG_USE_BVH),
                   rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_SKY | rwr.FLAG_ORTHO_RAYS),
                   rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_SKY | rwr.FLAG_USE_BVH)):
        with pytest.raises(rwr.RwrError) as ei:
            ctx.render(cam_inv, params)
        assert ei.value.code == rwr.ERR_UNSUPPORTED, params
    ctx.set_triangles(rwr.make_triangles([((0.0, 0.0, -2.0), (1.0, 0.0, -2.0), (0.0, 1.0, -2.0))]))
    try:
        for bounces in (0, 1):
            with pytest.raises(rwr.RwrError) as ei:
                ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=bounces, flags=rwr.FLAG_SKY))
            assert ei.value.code == rwr.ERR_UNSUPPORTED
    finally:
        ctx.set_triangles(rwr.make_triangles())
    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=1, flags=rwr.FLAG_SKY))   # the context is still usable


def test_denoiser_filters_the_sky_lit_frame(rwr, orc, sref, ctx, ref_loader, suzanne, cube, tmp_path_factory):
    """With RWR_FLAG_DENOISE the frame is denoise_ref.c applied to the sky reference's planes, within 1e-4; background passes through."""
    dref = denoise_ref.lib(tmp_path_factory)
    s = (cube, rwr.make_spheres([((1.6, 1.2, 1.4), 0.5)]), None, (2.2, 1.7, 3.1), (0, 0, 0), 64, 48, 4, 1)
    cam_inv = _cam(rwr, s)
    _upload(ctx, s)
    ref = _reference(sref, orc, s, cam_inv, 9, DEFAULT)
    assert ref["sky_terms"] > 0
    nhat = denoise_ref.face_normals(dref, orc, s[0], None)
    want = denoise_ref.denoise(dref, ref["color_f32"], ref["obj_id"], ref["hit_t"], nhat, **denoise_ref.DEFAULTS)
    ctx.set_denoise_params()
    plain = _frame(ctx, cam_inv, rwr.make_params(spp=4, max_bounces=1, seed=9, flags=_flags(rwr, 1)))
    got = _frame(ctx, cam_inv, rwr.make_params(spp=4, max_bounces=1, seed=9, flags=_flags(rwr, 1) | rwr.FLAG_DENOISE))
    for k in ("depth", "obj_id", "hit_t"):
        assert got[k].tobytes() == ref[k].tobytes(), k
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"denoised sky frame against the filtered reference: {err:.3g}")
    assert err <= 1e-4
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1
    assert got["color_f32"].tobytes() != plain["color_f32"].tobytes()              # the filter ran
    bg = ref["obj_id"] == -1
    assert bg.any() and np.array_equal(got["color_f32"][bg], plain["color_f32"][bg]) and np.array_equal(got["color"][bg], plain["color"][bg])
