"""Light rays aimed at the sky's image (RWR_FLAG_LIGHT_SKY) on the GPU:
  * the kernels' draw and factor against the tests' own (sky_light_ref.c), bit for bit;
  * frames against the CPU reference (sky_light_ref.c: mis_ref.c's chain with the flag's items): sample-0 planes bit-exact,
    rwr_last_render_stats, the six light counts and the sky's three equal, colour within COLOR_TOL (tests/test_gpu_multi_bounce.py,
    read from that file) x max(1, largest image or Le component) under RWR_FLAG_LIGHT_MIS - every light term is then at most T times
    that - and x 64 without it, where a term may reach the cap, as for the mesh light;
  * the form with 32-bit stacks; every schedule and split; accumulation; the histories' keys; a changed image; frames the flag does
    nothing to; refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sky_image_ref
import sky_light_common as sc
import sky_light_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
COLOR_TOL = float(re.search(r"^COLOR_TOL\s*=\s*([0-9.eE+-]+)", open(os.path.join(HERE, "test_gpu_multi_bounce.py")).read(), re.M).group(1))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
COUNTS = ("stats", "shadow", "emissive", "light", "part", "sky")
MAX_SPHERES = sky_light_ref.MAX_SPHERES
SUN = sc.SUN


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return sky_light_ref.lib(tmp_path_factory)


def _clear(c):
    c.sky_set_image(None)
    c.sky_set_params()
    c.set_instances(None)
    c.set_frames_in_flight(1)
    c.accum_reset()
    for i in range(MAX_SPHERES):
        c.set_sphere_gloss(i, 0.5, None)     # (any of the surface setters with None makes the surface diffuse)
        c.set_sphere_emission(i, None)


@pytest.fixture()
def ctx(gpu_ctx):
    """The shared context, left as it was found: no image, default sky, no instances, no accumulation, plain spheres."""
    _clear(gpu_ctx)
    yield gpu_ctx
    _clear(gpu_ctx)


def _upload(c, s, image=SUN):
    if isinstance(s["model"], (list, tuple)):
        c.upload_parts(s["model"])
    else:
        c.upload_model(s["model"])
    c.set_instances(s["instances"])
    c.set_spheres(s["spheres"])
    c.resize(s["w"], s["h"])
    for i in range(MAX_SPHERES):
        c.set_sphere_gloss(i, 0.5, None)
        c.set_sphere_emission(i, None)
    for k, r in s["mirror_spheres"].items():
        c.set_sphere_mirror(k, r)
    for k, le in s["emissive_parts"].items():
        c.set_part_emission(k, le)
    for k, le in s["emissive_spheres"].items():
        c.set_sphere_emission(k, le)
    c.sky_set_image(image)


def _params(rwr, s, seed, spp=None, bounces=None, **kw):
    return rwr.make_params(spp=s["spp"] if spp is None else spp, max_bounces=s["bounces"] if bounces is None else bounces, seed=seed,
                           flags=sc.flags(rwr, s, bounces=bounces, **kw))


def _frame(c, cam_inv, params, **kw):
    c.render(cam_inv, params, **kw)
    out = c.readback(aux=True)
    out["stats"] = c.last_render_stats()
    out["shadow"] = c.last_shadow_stats()
    out["emissive"] = c.last_emission_stats()
    out["light"] = c.last_light_stats()
    out["part"] = c.last_part_light_stats()
    out["sky"] = c.last_sky_light_stats()
    out["plan"] = c.last_traversal_plan()
    return out


def _same(a, b, what=""):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _same_counts(a, b, what=""):
    for k in COUNTS:
        assert a[k] == b[k], (what, k, a[k], b[k])


def _check(got, want, what, bar):
    """Planes bit for bit, the counts exactly, colour within the bar, RGBA8 within one code."""
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"sky light colour error {what}: {err:.3g} (bar {bar:.3g}); light rays, reached, suppressed {got['light']} "
          f"(reference {(want['light_rays'], want['reached'], want['suppressed'])}), the mesh light's {got['part']} ({want['part_light']}), "
          f"the sky's {got['sky']} ({want['sky_light']}), emissive hits {got['emissive']} ({want['emissive_hits']})")
    assert got["stats"][1] == want["rays"], what
    assert got["light"] == (want["light_rays"], want["reached"], want["suppressed"]), (what, want["light_gen"].tolist())
    assert got["part"] == want["part_light"], what
    assert got["sky"] == want["sky_light"], what
    assert got["emissive"] == want["emissive_hits"], what
    assert err <= bar, (what, err)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, what


# ------------------------------------------------------------------------------------------------ 1. the device functions
@pytest.mark.parametrize("n", [2, 5, 16])
def test_device_functions_bit_for_bit(ctx, sref, n):
    """omega, the texel, P and g of rwr_selftest_sky_light equal sky_light_ref.c's as bits: 4 096 random four-tuples, uniforms of
    exactly 0 and of 1 - 2^-24 in every position, normals on the axes."""
    img = sc.SUN if n == 16 else sky_image_ref.make_image(n)
    ctx.sky_set_image(img)
    assert ctx.sky_get_light_info() == {"n": n, "generation": ctx.sky_get_image_info()["generation"]}
    W, tab = sky_light_ref.table(sref, img)
    assert W > 0
    u = np.random.default_rng(40 + n).random((4096, 4)).astype(np.float32)
    ends = np.asarray([[a if (k >> b) & 1 else z for b in range(4)] for k in range(16) for a, z in ((1.0 - 2.0 ** -24, 0.0), (0.0, 0.37))], np.float32)
    u = np.concatenate([ends, u])
    for normal, lights in (((0, 1, 0), 1), ((0, -1, 0), 2), ((1, 0, 0), 3), ((-1, 0, 0), 1), ((0, 0, 1), 10), ((0, 0, -1), 1), ((0.6, 0.0, 0.8), 2)):
        got = ctx.selftest_sky_light(u, normal=normal, n_lights=lights)
        want = sky_light_ref.samples(sref, tab, n, u, normal=normal, n_lights=lights)
        for k in ("omega", "P", "g"):
            bad = np.flatnonzero((got[k].view(np.uint32) != want[k].view(np.uint32)).reshape(len(u), -1).any(axis=1))
            assert len(bad) == 0, (n, normal, k, len(bad), u[bad[:3]], got[k][bad[:3]], want[k][bad[:3]])
        assert np.array_equal(got["texel"], want["texel"]), (n, normal)
        assert (got["texel"] < n).all() and (want["P"] > 0).mean() > 0.999


# ------------------------------------------------------------------------------------------------ 2. frames
@pytest.mark.parametrize("mis", [True, False], ids=["mis", "plain"])
@pytest.mark.parametrize("name", sc.SCENES)
def test_matches_the_reference(rwr, orc, sref, ctx, ref_loader, suzanne, cube, name, mis):
    s = sc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    want = sc.reference(sref, rwr, orc, s, 13, name, mis=mis)
    assert want["sky_light"][1] > 0 and want["sky_light"][2] > 0          # (tests/test_sky_light_host.py says what each scene shows)
    cam_inv = sc.camera(rwr, s)
    _upload(ctx, s)
    got = _frame(ctx, cam_inv, _params(rwr, s, 13, mis=mis))
    _check(got, want, f"{name} mis={mis}", COLOR_TOL * sc.bar_factor(s, SUN, mis))
    # the frame without the flag, from the same loop: what the image alone gives
    off = _frame(ctx, cam_inv, _params(rwr, s, 13, mis=mis, sky_light=False))
    assert off["sky"] == (0, 0, 0) and off["color_f32"].tobytes() != got["color_f32"].tobytes()
    _check(off, sc.reference(sref, rwr, orc, s, 13, name, mis=mis, sky_light=False), f"{name} mis={mis} without the flag",
           COLOR_TOL * sc.bar_factor(s, SUN, mis or not (s["light"] or s["parts"])))


@pytest.mark.parametrize("mis", [True, False], ids=["mis", "plain"])
def test_matches_the_reference_under_sobol(rwr, orc, ctx, ref_loader, suzanne, cube, tmp_path_factory, mis):
    """lamp_panel_sun - all three light flags, L = 3 - with every number drawn from the sequence."""
    sob = sky_light_ref.lib(tmp_path_factory, sobol=True)
    s = sc.scene("lamp_panel_sun", rwr, ref_loader, suzanne, cube, orc)
    want = sc.reference(sob, rwr, orc, s, 13, "lamp_panel_sun", mis=mis)
    assert want["sky_light"][1] > 0 and want["part_light"][0] > 0
    _upload(ctx, s)
    got = _frame(ctx, sc.camera(rwr, s), _params(rwr, s, 13, mis=mis, extra=rwr.FLAG_SOBOL))
    _check(got, want, f"lamp_panel_sun sobol mis={mis}", COLOR_TOL * sc.bar_factor(s, SUN, mis))


# ------------------------------------------------------------------------------------------------ 3. forms
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


@pytest.mark.parametrize("name", ("bare_lamp_sun", "bare_panel_sun"))
def test_32_bit_stacks_beside_nodelets_in_lds(rwr, orc, sref, ctx, ref_loader, suzanne, cube, name):
    """k_wf_light's SKY forms with nodelets in LDS and 32-bit stacks, without and with PARTS: a context created under
    RWR_WF_STACK16=0 gives the 16-bit run's bytes and counts, which the reference vouches for."""
    s = sc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    cam_inv = sc.camera(rwr, s)
    params = _params(rwr, s, 13)
    _upload(ctx, s)
    got = _frame(ctx, cam_inv, params)
    _check(got, sc.reference(sref, rwr, orc, s, 13, name), f"{name} 16-bit stacks", COLOR_TOL * sc.bar_factor(s, SUN, True))
    assert got["plan"]["trace"]["nodes_in_lds"] == 1 and got["plan"]["trace"]["stack16"] == 1, got["plan"]
    assert (got["part"][0] > 0) == s["parts"]
    wide = _with_env(rwr, {"RWR_WF_STACK16": "0", "RWR_WF_WIDE_LANE": "0"}, s, cam_inv, params)
    assert wide["plan"]["trace"]["nodes_in_lds"] == 1 and wide["plan"]["trace"]["stack16"] == 0, wide["plan"]
    _same(wide, got, "32-bit stacks")
    _same_counts(wide, got, "32-bit stacks")


def test_schedules_give_the_same_frame(rwr, ref_loader, suzanne, cube, orc):
    """Packet, per-lane and wide overrides, queues and groups: all five planes the same bytes, the counts equal."""
    s = dict(sc.scene("cube_grid", rwr, ref_loader, suzanne, cube, orc), spp=7)
    cam_inv = sc.camera(rwr, s)
    params = _params(rwr, s, 3)
    default = _with_env(rwr, {}, s, cam_inv, params)
    assert default["sky"][1] > 0 and default["sky"][2] > 0
    for zsplit, queues, group, dense, wide in (("1", "1", "32", "40", "0"), ("4", "2", "4", "400", "1"), ("3", "2", "2", "0", "0"), ("1", "2", "3", "0", "1")):
        got = _with_env(rwr, {"RWR_WF_ZSPLIT": zsplit, "RWR_WF_OVERLAP": queues, "RWR_WF_GROUP": group, "RWR_WF_PACKET_RAYS": dense,
                              "RWR_WF_MIN_PACKET_POOLS": "0" if dense != "0" else "128", "RWR_WF_WIDE_LANE": wide}, s, cam_inv, params)
        _same(got, default, (zsplit, queues, group, dense, wide))
        _same_counts(got, default, (zsplit, queues, group, dense, wide))


# ------------------------------------------------------------------------------------------------ 4. splits, frames in flight, accumulation
@pytest.mark.parametrize("split", ["strips", "bands"])
def test_splits_assemble_the_frame(rwr, ctx, suzanne, split):
    w, h = 203, 67
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0.3, 0.2, 2.6), aspect=w / h))
    flags = rwr.FLAG_AUX_OUTPUTS | rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_SKY | rwr.FLAG_SKY_IMAGE | rwr.FLAG_LIGHT_SKY | rwr.FLAG_LIGHT_MIS
    params = rwr.make_params(spp=3, max_bounces=2, seed=2, flags=flags)
    ctx.upload_model(suzanne); ctx.set_spheres(rwr.make_spheres()); ctx.resize(w, h)
    ctx.sky_set_image(SUN)
    full = _frame(ctx, cam_inv, params)
    assert full["sky"][0] > full["sky"][1] > 0 and full["sky"][2] > 0
    for n in (2, 3):
        asm = {k: np.zeros_like(full[k]) for k in PLANES}
        counts = np.zeros(7, np.int64)
        for r in range(n):
            if split == "strips":
                part = _frame(ctx, cam_inv, params, strips=(r, n))
                rows = [y for y in range(h) if (y // 8) % n == r]
            else:
                band = rwr.dist_band(r, n, h)
                part = _frame(ctx, cam_inv, params, rows=band)
                rows = list(range(*band))
            counts += np.asarray((part["stats"][1],) + part["light"] + part["sky"])
            for k in PLANES:
                asm[k][rows] = part[k][rows]
        _same(asm, full, (split, n))
        assert tuple(counts) == (full["stats"][1],) + full["light"] + full["sky"], (split, n)


def test_frames_in_flight_and_accumulation(rwr, ctx, suzanne):
    """K frames of s samples are one frame of K s, one frame at a time and with two in flight."""
    w, h = 120, 64
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0.3, 0.2, 2.6), aspect=w / h))
    ctx.upload_model(suzanne); ctx.set_spheres(rwr.make_spheres()); ctx.resize(w, h)
    ctx.sky_set_image(SUN)
    flags = rwr.FLAG_AUX_OUTPUTS | rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_SKY | rwr.FLAG_SKY_IMAGE | rwr.FLAG_LIGHT_SKY | rwr.FLAG_LIGHT_MIS
    want = _frame(ctx, cam_inv, rwr.make_params(spp=6, max_bounces=2, seed=11, flags=flags))
    assert want["sky"][1] > 0
    acc = rwr.make_params(spp=2, max_bounces=2, seed=11, flags=flags | rwr.FLAG_ACCUMULATE)
    for in_flight in (1, 2):
        ctx.set_frames_in_flight(in_flight)
        ctx.accum_reset()
        for k in range(1, 4):
            ctx.render(cam_inv, acc)
        ctx.synchronize()
        assert ctx.accum_samples() == 6
        _same(ctx.readback(aux=True), want, f"3 x 2 spp, {in_flight} in flight")
    ctx.set_frames_in_flight(1)
    _same(_frame(ctx, cam_inv, rwr.make_params(spp=6, max_bounces=2, seed=11, flags=flags)), want, "again, one at a time")


# ------------------------------------------------------------------------------------------------ 5. the histories and a changed image
def test_the_flag_and_a_changed_image_restart_the_histories(rwr, ctx, suzanne):
    w, h = 120, 64
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0.3, 0.2, 2.6), aspect=w / h))
    ctx.upload_model(suzanne); ctx.set_spheres(rwr.make_spheres()); ctx.resize(w, h)
    ctx.sky_set_image(SUN)
    base = rwr.FLAG_AUX_OUTPUTS | rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_SKY | rwr.FLAG_SKY_IMAGE
    on = base | rwr.FLAG_LIGHT_SKY
    ctx.accum_reset()
    acc = lambda f: rwr.make_params(spp=2, max_bounces=2, seed=11, flags=f | rwr.FLAG_ACCUMULATE)
    seen = []
    for f, image in ((on, None), (on, None), (base, None), (on, None), (on, SUN), (on, None)):
        if image is not None:
            ctx.sky_set_image(image)
        ctx.render(cam_inv, acc(f))
        seen.append(ctx.accum_samples())
    assert seen == [2, 4, 2, 2, 2, 4], seen
    ctx.reproject_reset()
    seen = []
    for f, image in ((on, None), (on, None), (base, None), (on, None), (on, SUN), (on, None)):
        if image is not None:
            ctx.sky_set_image(image)
        ctx.render(cam_inv, rwr.make_params(spp=2, max_bounces=2, seed=11, flags=f | rwr.FLAG_REPROJECT))
        seen.append(ctx.reproject_frames())
    assert seen == [1, 2, 1, 1, 1, 2], seen
    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=0, flags=0))     # (ends the history)


def test_a_changed_image_changes_the_table(rwr, orc, sref, ctx, ref_loader, suzanne, cube):
    """A new image under a context that has rendered with the old one: the table is rebuilt, the counts differ and still match the
    reference; rwr_sky_get_light_info follows."""
    s = sc.scene("soup", rwr, ref_loader, suzanne, cube, orc)
    cam_inv = sc.camera(rwr, s)
    _upload(ctx, s)
    first = _frame(ctx, cam_inv, _params(rwr, s, 13))
    assert ctx.sky_get_light_info() == {"n": 16, "generation": ctx.sky_get_image_info()["generation"]}
    other = np.ascontiguousarray(SUN[::-1, ::-1]) * np.float32(0.5)
    other[2, 3] = (64.0, 1.0, 0.0)
    ctx.sky_set_image(other)
    got = _frame(ctx, cam_inv, _params(rwr, s, 13))
    assert got["sky"] != first["sky"]
    assert ctx.sky_get_light_info() == {"n": 16, "generation": ctx.sky_get_image_info()["generation"]}
    _check(got, sc.reference(sref, rwr, orc, s, 13, "soup", image=other), "soup, another image", COLOR_TOL * sc.bar_factor(s, other, True))
    ctx.sky_set_image(SUN)
    again = _frame(ctx, cam_inv, _params(rwr, s, 13))
    _same(again, first, "the first image again")
    _same_counts(again, first, "the first image again")


# ------------------------------------------------------------------------------------------------ 6. frames the flag does nothing to
def test_frames_the_flag_does_nothing_to(rwr, ctx, ref_loader, suzanne, cube, orc):
    """Under the gradient, without RWR_FLAG_SKY, with an all-black image, with max_bounces 0: the bytes and the counts of the frame
    without the bit (and without RWR_FLAG_LIGHT_MIS, which nothing then makes effective)."""
    for name in ("cube_grid", "lamp_panel_sun"):
        s = dict(sc.scene(name, rwr, ref_loader, suzanne, cube, orc), spp=5)
        cam_inv = sc.camera(rwr, s)
        _upload(ctx, s)
        lit = _frame(ctx, cam_inv, _params(rwr, s, 5))
        assert lit["sky"][0] > 0

        def nothing(what, **kw):
            want = _frame(ctx, cam_inv, _params(rwr, s, 5, sky_light=False, **kw))
            got = _frame(ctx, cam_inv, _params(rwr, s, 5, **kw))
            _same(got, want, (name, what))
            _same_counts(got, want, (name, what))
            assert got["sky"] == (0, 0, 0) and got["plan"] == want["plan"], (name, what)

        nothing("the gradient", image=False)
        nothing("no sky flag", sky=False)
        nothing("no bounce", bounces=0)
        ctx.sky_set_image(np.zeros((4, 4, 3), np.float32))
        assert ctx.sky_get_light_info()["n"] == 0
        nothing("a black image")
        ctx.sky_set_image(None)
        assert ctx.sky_get_light_info()["n"] == 0
        nothing("no image")


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(rwr, ctx, suzanne):
    L = rwr.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    u = np.zeros((1, 4), np.float32)
    nrm = np.asarray((0, 1, 0), np.float32)
    out = np.zeros(8, np.float32)
    with pytest.raises(rwr.RwrError) as ei:      # no image
        ctx.selftest_sky_light(u)
    assert ei.value.code == rwr.ERR_NOT_READY
    ctx.sky_set_image(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(rwr.RwrError) as ei:      # nothing to draw from
        ctx.selftest_sky_light(u)
    assert ei.value.code == rwr.ERR_NOT_READY
    ctx.sky_set_image(SUN)
    assert L.rwr_selftest_sky_light(ctx._h, None, 1, p(nrm), 1, p(out)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_selftest_sky_light(ctx._h, p(u), 1, None, 1, p(out)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_selftest_sky_light(None, p(u), 1, p(nrm), 1, p(out)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_sky_get_light_info(None, None, None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_sky_get_light_info(ctx._h, None, None) == rwr.OK
    assert L.rwr_last_sky_light_stats(ctx._h, None, None, None) == rwr.ERR_INVALID_ARGUMENT
    # reference-frame-only modes refuse the flag, at bounces 0 too, with or without an image
    w, h = 64, 48
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0, 0, 3), aspect=w / h))
    ctx.upload_model(suzanne); ctx.set_spheres(rwr.make_spheres()); ctx.resize(w, h)
    sky = rwr.FLAG_SKY | rwr.FLAG_SKY_IMAGE | rwr.FLAG_LIGHT_SKY
    for image in (None, SUN):
        ctx.sky_set_image(image)
        for params in (rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_LIGHT_SKY | rwr.FLAG_ORTHO_RAYS),
                       rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_LIGHT_SKY | rwr.FLAG_USE_BVH),
                       rwr.make_params(spp=2, max_bounces=1, flags=sky | rwr.FLAG_ORTHO_RAYS),
                       rwr.make_params(spp=2, max_bounces=1, flags=sky | rwr.FLAG_USE_BVH)):
            with pytest.raises(rwr.RwrError) as ei:
                ctx.render(cam_inv, params)
            assert ei.value.code == rwr.ERR_UNSUPPORTED, params
    with pytest.raises(rwr.RwrError) as ei:
        ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_LIGHT_SKY | rwr.FLAG_ORTHO_RAYS))
    assert "RWR_FLAG_LIGHT_SKY" in ei.value.message
    ctx.set_triangles(rwr.make_triangles([((0.0, 0.0, -2.0), (1.0, 0.0, -2.0), (0.0, 1.0, -2.0))]))
    try:
        for bounces in (0, 1):
            with pytest.raises(rwr.RwrError) as ei:
                ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=bounces, flags=rwr.FLAG_LIGHT_SKY))
            assert ei.value.code == rwr.ERR_UNSUPPORTED
    finally:
        ctx.set_triangles(rwr.make_triangles())
    ctx.render(cam_inv, rwr.make_params(spp=2, max_bounces=1, flags=sky))   # the context is still usable
    assert ctx.last_sky_light_stats()[0] > 0
