"""Sky light from an image (RWR_FLAG_SKY_IMAGE) on the GPU:
  * the kernels' S_img against the tests' own (sky_image_ref.c), bit for bit;
  * frames against the CPU reference (sky_image_ref.render_path: mis_ref.c's chain under a black sky plus the image's terms):
    sample-0 planes bit-exact, counts equal, colour within COLOR_TOL (tests/test_gpu_multi_bounce.py, read from that file) scaled
    by the image's largest texel — the scaling tests/test_gpu_sky.py derives for a tinted sky: a sky term's error is relative to S;
  * every schedule and split: the same bytes; accumulation and the histories' keys; frames the flag does nothing to; refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mis_ref
import sky_image_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
COLOR_TOL = float(re.search(r"^COLOR_TOL\s*=\s*([0-9.eE+-]+)", open(os.path.join(HERE, "test_gpu_multi_bounce.py")).read(), re.M).group(1))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
DEFAULT_SKY = ((0.5, 0.7, 1.0), (1.0, 1.0, 1.0))
IMAGE = sky_image_ref.make_image(8)
_cache = {}


@pytest.fixture(scope="module")
def iref(tmp_path_factory):
    return sky_image_ref.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def mref(tmp_path_factory):
    return mis_ref.lib(tmp_path_factory)


def _clear(c):
    c.sky_set_image(None)
    c.sky_set_params()
    c.set_instances(None)
    c.accum_reset()
    for i in range(2):
        c.set_sphere_gloss(i, 0.5, None)     # (any of the surface setters with None makes the surface diffuse)


@pytest.fixture()
def ctx(gpu_ctx):
    """The shared context, left as it was found: no image, default sky, no instances, no accumulation, diffuse spheres."""
    _clear(gpu_ctx)
    yield gpu_ctx
    _clear(gpu_ctx)


def _soup(ref_loader, cube):
    import shadow_common
    rng = np.random.default_rng(11)
    centre = rng.uniform(-1.2, 1.2, size=(60, 1, 3))
    tris = centre + rng.normal(scale=0.45, size=(60, 3, 3))
    return shadow_common.triangle_model(ref_loader, [tuple(map(tuple, t)) for t in tris.astype(np.float32)], cube["texture"])


def _scene(name, rwr, ref_loader, suzanne, cube):
    """The scenes of tests/test_gpu_sky.py: model, spheres, instances, eye, target, w, h, spp, bounces, and the surfaces:
    {"mirror": {sphere: reflectance}} or {"gloss": {sphere: (roughness, reflectance)}}."""
    s = dict(instances=None, surfaces={})
    if name == "cube_b1":
        s.update(model=cube, spheres=rwr.make_spheres([]), eye=(1.0, 0.8, 1.4), target=(0, 0, 0), w=64, h=48, spp=4, bounces=1)
    elif name == "cube_b8":
        s.update(model=cube, spheres=rwr.make_spheres([]), eye=(1.0, 0.8, 1.4), target=(0, 0, 0), w=64, h=48, spp=4, bounces=8)
    elif name in ("soup", "soup_gloss"):   # an odd size: partial tiles; sphere 0 a mirror, or glossy
        if "soup" not in _cache:
            _cache["soup"] = _soup(ref_loader, cube)
        s.update(model=_cache["soup"], spheres=rwr.make_spheres([((0.9, 0.4, 0.6), 0.5), ((-0.8, -0.5, 0.2), 0.35)]), eye=(0.3, 0.5, 2.2),
                 target=(0, 0, 0), w=37, h=29, spp=5, bounces=3,
                 surfaces={"mirror": {0: (1.0, 1.0, 1.0)}} if name == "soup" else {"gloss": {0: (0.25, (0.8, 0.9, 1.0))}})
    elif name == "grid_gloss":   # 64 samples: the packet kernel, its glossy form
        s.update(model=cube, spheres=rwr.make_spheres([((-1.5, 1.2, -1.5), 0.6)]), instances=rwr.make_instance_grid(2, 3.0), eye=(-1.5, 1.5, 2.5),
                 target=(-1.5, 0.0, -1.5), w=64, h=48, spp=64, bounces=2, surfaces={"gloss": {0: (0.25, (0.8, 0.9, 1.0))}})
    elif name == "cube_grid":  # 64 samples: pools dense enough for the packet kernel
        s.update(model=cube, spheres=rwr.make_spheres([]), instances=rwr.make_instance_grid(2, 3.0), eye=(-1.5, 1.5, 2.5), target=(-1.5, 0.0, -1.5),
                 w=64, h=48, spp=64, bounces=2)
    elif name == "suzanne_far":
        s.update(model=suzanne, spheres=rwr.make_spheres(), eye=(0, 0, 3), target=(0, 0, -1), w=200, h=72, spp=7, bounces=2)
    else:
        raise KeyError(name)
    return s


def _cam(rwr, s):
    return rwr.camera_build_inv_uniform(rwr.make_camera(eye=s["eye"], target=s["target"], aspect=s["w"] / s["h"]))


def _flags(rwr, s, image=True, sky=True, shadows=False, extra=0):
    f = rwr.FLAG_AUX_OUTPUTS | extra | (rwr.FLAG_MULTI_BOUNCE if s["bounces"] > 1 else 0) | (rwr.FLAG_SHADOWS if shadows else 0)
    f |= (rwr.FLAG_SKY if sky else 0) | (rwr.FLAG_SKY_IMAGE if image else 0)
    f |= (rwr.FLAG_MIRRORS if "mirror" in s["surfaces"] else 0) | (rwr.FLAG_GLOSSY if "gloss" in s["surfaces"] else 0)
    return f


def _params(rwr, s, seed, **kw):
    return rwr.make_params(spp=s["spp"], max_bounces=s["bounces"], seed=seed, flags=_flags(rwr, s, **kw))


def _upload(c, s):
    c.upload_model(s["model"])
    c.set_instances(s["instances"])
    c.set_spheres(s["spheres"])
    for k, refl in s["surfaces"].get("mirror", {}).items():
        c.set_sphere_mirror(k, refl)
    for k, (rough, refl) in s["surfaces"].get("gloss", {}).items():
        c.set_sphere_gloss(k, rough, refl)
    c.resize(s["w"], s["h"])


def _frame(c, cam_inv, params, **kw):
    c.render(cam_inv, params, **kw)
    out = c.readback(aux=True)
    out["stats"] = c.last_render_stats()
    out["shadow"] = c.last_shadow_stats()
    return out


def _same(a, b, what=""):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _reference(iref, mref, orc, s, cam_inv, seed, shadows):
    """The frame under IMAGE, with "gradient_f32": the colour under the default gradient."""
    key = (id(s["model"]), str(s["surfaces"]), s["eye"], s["w"], s["h"], s["spp"], s["bounces"], seed, shadows)
    if key not in _cache:
        inst = None if s["instances"] is None else s["instances"].view(orc.INSTANCE_DTYPE)
        _cache[key] = sky_image_ref.render_path(iref, mref, orc, cam_inv.view(orc.CAMERA_INV_DTYPE), orc.make_screen(s["w"], s["h"]),
                                                orc.make_params(s["spp"], s["bounces"], seed=seed), s["spheres"].view(orc.SPHERE_DTYPE), s["model"],
                                                IMAGE, gradient=DEFAULT_SKY, instances=inst, shadows=shadows,
                                                mirror_spheres=s["surfaces"].get("mirror"), gloss_spheres=s["surfaces"].get("gloss"))
    return _cache[key]


# ------------------------------------------------------------------------------------------------ 1. the device function
@pytest.mark.parametrize("n", [2, 5, 8])
def test_device_function_bit_for_bit(ctx, iref, n):
    img = sky_image_ref.make_image(n)
    assert img.max() == 64.0 and (img.reshape(-1, 3).max(axis=1) == 0.0).sum() >= 1
    dirs = np.concatenate([sky_image_ref.special_directions(), sky_image_ref.texel_centre_directions(n), sky_image_ref.random_directions(4096, 100 + n)])
    ctx.sky_set_image(img)
    assert ctx.sky_get_image_info()["n"] == n
    got = ctx.selftest_sky_image(dirs)
    want = sky_image_ref.radiance(iref, img, dirs)
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, (n, len(bad), dirs[bad[:4]], got[bad[:4]], want[bad[:4]])
    assert np.isfinite(got).all() and got.max() <= 64.0 and got.min() >= 0.0


# ------------------------------------------------------------------------------------------------ 2. frames
@pytest.mark.parametrize("shadows", [False, True], ids=["plain", "shadows"])
@pytest.mark.parametrize("name", ["cube_b1", "cube_b8", "soup", "cube_grid", "soup_gloss", "grid_gloss"])
def test_matches_the_reference(rwr, orc, iref, mref, ctx, ref_loader, suzanne, cube, name, shadows):
    s = _scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = _cam(rwr, s)
    want = _reference(iref, mref, orc, s, cam_inv, 13, shadows)
    # on the reference alone: the scene sees the sky, and the image is not the gradient
    assert want["sky_terms"] > 0 and want["sky_terms"] == int((want["misses"][..., 7] != 0).sum())
    assert not np.array_equal(want["color_f32"], want["gradient_f32"]) and not np.array_equal(want["gradient_f32"], want["black_f32"])
    if name == "soup":
        assert (want["misses"][..., 6] >= 2).any() and want["gen_mirror"].sum() > 0      # a reflected ray reached the sky
    if "gloss" in s["surfaces"]:
        assert want["glossy"] > 0
    _upload(ctx, s)
    ctx.sky_set_image(IMAGE)
    got = _frame(ctx, cam_inv, _params(rwr, s, 13, shadows=shadows))
    what = f"{name} shadows={shadows}"
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)
    assert got["stats"] == (s["w"] * s["h"] * s["spp"], want["rays"]), what
    assert got["shadow"] == ((want["shadow_rays"], want["occluded"]) if shadows else (0, 0)), what
    if "gloss" in s["surfaces"]:
        assert ctx.last_gloss_stats() == want["glossy"]
    bar = COLOR_TOL * max(1.0, float(IMAGE.max()))
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"sky image colour error {what}: {err:.3g} (bar {bar:.3g})")
    assert err <= bar, (what, err)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, what
    # the frame under the gradient, from the same records
    got = _frame(ctx, cam_inv, _params(rwr, s, 13, shadows=shadows, image=False))
    assert float(np.abs(got["color_f32"] - want["gradient_f32"]).max()) <= COLOR_TOL, what


# ------------------------------------------------------------------------------------------------ 3. schedules
def test_schedules_give_the_same_frame(rwr, ref_loader, suzanne, cube):
    """The packet, per-lane and wide overrides of test_schedules_give_the_same_frame (tests/test_gpu_sky.py): all five planes the same bytes."""
    s = _scene("suzanne_far", rwr, ref_loader, suzanne, cube)
    cam_inv = _cam(rwr, s)
    params = _params(rwr, s, 3)
    keys = ("RWR_WF_ZSPLIT", "RWR_WF_OVERLAP", "RWR_WF_GROUP", "RWR_WF_PACKET_RAYS", "RWR_WF_MIN_PACKET_POOLS", "RWR_WF_WIDE_LANE")
    saved = {k: os.environ.get(k) for k in keys}
    try:
        with rwr.Context(0) as c:
            _upload(c, s)
            c.sky_set_image(IMAGE)
            default = _frame(c, cam_inv, params)
            plain = _frame(c, cam_inv, _params(rwr, s, 3, image=False))
        assert default["color_f32"].tobytes() != plain["color_f32"].tobytes()
        for zsplit, queues, group, dense, wide in (("1", "1", "32", "40", "0"), ("4", "2", "4", "400", "1"), ("3", "2", "2", "0", "0"), ("1", "2", "3", "0", "1")):
            os.environ.update({"RWR_WF_ZSPLIT": zsplit, "RWR_WF_OVERLAP": queues, "RWR_WF_GROUP": group, "RWR_WF_PACKET_RAYS": dense,
                               "RWR_WF_MIN_PACKET_POOLS": "0" if dense != "0" else "128", "RWR_WF_WIDE_LANE": wide})
            with rwr.Context(0) as c:        # the tunables are read when the context is created
                _upload(c, s)
                c.sky_set_image(IMAGE)
                got = _frame(c, cam_inv, params)
            _same(got, default, (zsplit, queues, group, dense, wide))
            assert got["stats"] == default["stats"]
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------------ 4. splits
@pytest.mark.parametrize("split", ["strips", "bands"])
def test_splits_assemble_the_frame(rwr, ctx, suzanne, split):
    w, h = 203, 67
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0.3, 0.2, 2.6), aspect=w / h))
    flags = rwr.FLAG_AUX_OUTPUTS | rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_SHADOWS | rwr.FLAG_SKY | rwr.FLAG_SKY_IMAGE
    params = rwr.make_params(spp=3, max_bounces=2, seed=2, flags=flags)
    ctx.upload_model(suzanne); ctx.set_spheres(rwr.make_spheres()); ctx.resize(w, h)
    ctx.sky_set_image(IMAGE)
    full = _frame(ctx, cam_inv, params)
    assert _frame(ctx, cam_inv, rwr.make_params(spp=3, max_bounces=2, seed=2, flags=flags & ~rwr.FLAG_SKY_IMAGE))["color_f32"].tobytes() != full["color_f32"].tobytes()
    for n in (2, 3):
        asm = {k: np.zeros_like(full[k]) for k in PLANES}
        rays = 0
        for r in range(n):
            if split == "strips":
                part = _frame(ctx, cam_inv, params, strips=(r, n))
                rows = [y for y in range(h) if (y // 8) % n == r]
            else:
                band = rwr.dist_band(r, n, h)
                part = _frame(ctx, cam_inv, params, rows=band)
                rows = list(range(*band))
            rays += part["stats"][1]
            for k in PLANES:
                asm[k][rows] = part[k][rows]
        _same(asm, full, (split, n))
        assert rays == full["stats"][1]


# ------------------------------------------------------------------------------------------------ 5. accumulation and the keys
def test_accumulation_and_the_keys(rwr, ctx, suzanne):
    w, h = 120, 64
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0.3, 0.2, 2.6), aspect=w / h))
    ctx.upload_model(suzanne); ctx.set_spheres(rwr.make_spheres()); ctx.resize(w, h)
    ctx.sky_set_image(IMAGE)
    gen = ctx.sky_get_image_info()["generation"]
    flags = rwr.FLAG_AUX_OUTPUTS | rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_SKY | rwr.FLAG_SKY_IMAGE
    want = _frame(ctx, cam_inv, rwr.make_params(spp=6, max_bounces=2, seed=11, flags=flags))
    ctx.accum_reset()
    acc = rwr.make_params(spp=2, max_bounces=2, seed=11, flags=flags | rwr.FLAG_ACCUMULATE)
    for k in range(1, 4):
        ctx.render(cam_inv, acc)
        assert ctx.accum_samples() == 2 * k
    _same(ctx.readback(aux=True), want, "3 x 2 spp")
    # the same array again is a new generation: the accumulation starts over
    ctx.sky_set_image(IMAGE)
    assert ctx.sky_get_image_info() == {"n": 8, "generation": gen + 1}
    ctx.render(cam_inv, acc)
    assert ctx.accum_samples() == 2
    ctx.render(cam_inv, acc)
    assert ctx.accum_samples() == 4
    # without the flag the image is no part of the frame: it may change under a running accumulation
    ctx.accum_reset()
    plain = rwr.make_params(spp=2, max_bounces=2, seed=11, flags=(flags & ~rwr.FLAG_SKY_IMAGE) | rwr.FLAG_ACCUMULATE)
    ctx.render(cam_inv, plain)
    ctx.sky_set_image(sky_image_ref.make_image(5))
    ctx.render(cam_inv, plain)
    assert ctx.accum_samples() == 4
    ctx.sky_set_image(None)
    ctx.render(cam_inv, plain)
    assert ctx.accum_samples() == 6
    assert ctx.sky_get_image_info() == {"n": 0, "generation": gen + 3}
    # RWR_FLAG_REPROJECT: a new image starts a new history; without the bit it does not
    ctx.sky_set_image(IMAGE)
    for with_bit, expect in ((True, (1, 2, 1, 2)), (False, (1, 2, 3, 4))):
        ctx.reproject_reset()
        rp = rwr.make_params(spp=2, max_bounces=2, seed=11, flags=(flags if with_bit else flags & ~rwr.FLAG_SKY_IMAGE) | rwr.FLAG_REPROJECT)
        seen = []
        for k in range(4):
            if k == 2:
                ctx.sky_set_image(IMAGE)
            ctx.render(cam_inv, rp)
            seen.append(ctx.reproject_frames())
        assert tuple(seen) == expect, (with_bit, seen)
    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=0, flags=0))     # (ends the history)


# ------------------------------------------------------------------------------------------------ 6. frames the flag does nothing to
def test_frames_the_flag_does_nothing_to(rwr, ctx, ref_loader, suzanne, cube):
    for name in ("cube_grid", "suzanne_far"):
        s = dict(_scene(name, rwr, ref_loader, suzanne, cube), spp=5, bounces=2)
        cam_inv = _cam(rwr, s)
        _upload(ctx, s)
        ctx.sky_set_image(None)
        sky = _frame(ctx, cam_inv, _params(rwr, s, 5, image=False))
        none = _frame(ctx, cam_inv, _params(rwr, s, 5, image=False, sky=False))
        assert sky["color_f32"].tobytes() != none["color_f32"].tobytes()
        # no image set: the frame under the gradient
        _same(_frame(ctx, cam_inv, _params(rwr, s, 5)), sky, (name, "no image"))
        ctx.sky_set_image(IMAGE)
        # the flag without RWR_FLAG_SKY
        _same(_frame(ctx, cam_inv, _params(rwr, s, 5, sky=False)), none, (name, "no sky flag"))
        # RWR_FLAG_SKY alone, with an image in the context
        _same(_frame(ctx, cam_inv, _params(rwr, s, 5, image=False)), sky, (name, "image set, flag off"))
        # max_bounces = 0, at spp 1 (the reference frame) and above
        for spp in (1, 4):
            flat = dict(s, spp=spp, bounces=0)
            _same(_frame(ctx, cam_inv, _params(rwr, flat, 5)), _frame(ctx, cam_inv, _params(rwr, flat, 5, image=False, sky=False)), (name, "no bounce", spp))
        # an all-zero image: the frame with no sky flag at all
        ctx.sky_set_image(np.zeros((4, 4, 3), np.float32))
        black = _frame(ctx, cam_inv, _params(rwr, s, 5))
        _same(black, none, (name, "black image"))
        assert black["stats"] == none["stats"]
        # ... and RWR_FLAG_SKY alone after the image is removed
        ctx.sky_set_image(None)
        _same(_frame(ctx, cam_inv, _params(rwr, s, 5, image=False)), sky, (name, "image removed"))


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(rwr, ctx, suzanne):
    L = rwr.lib()
    ctx.sky_set_image(IMAGE)
    kept = ctx.sky_get_image_info()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for n in (1, 2049):
        assert L.rwr_sky_set_image(ctx._h, p(np.zeros(3 * 4, np.float32)), n) == rwr.ERR_INVALID_ARGUMENT, n
    for bad in (np.nan, -1e-6, 64.5, np.inf):
        img = IMAGE.copy()
        img[3, 5, 1] = bad
        with pytest.raises(rwr.RwrError) as ei:
            ctx.sky_set_image(img)
        assert ei.value.code == rwr.ERR_INVALID_ARGUMENT and f"[{(3 * 8 + 5) * 3 + 1}]" in ei.value.message, (bad, ei.value.message)
    assert ctx.sky_get_image_info() == kept                       # the image and its generation stay
    assert np.array_equal(ctx.selftest_sky_image(sky_image_ref.texel_centre_directions(8)), IMAGE.reshape(-1, 3))
    assert L.rwr_sky_set_image(None, p(IMAGE), 8) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_sky_get_image_info(None, None, None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_sky_get_image_info(ctx._h, None, None) == rwr.OK
    assert L.rwr_selftest_sky_image(ctx._h, None, 1, None) == rwr.ERR_INVALID_ARGUMENT
    ctx.sky_set_image(None)
    with pytest.raises(rwr.RwrError) as ei:
        ctx.selftest_sky_image(np.zeros((1, 3), np.float32))
    assert ei.value.code == rwr.ERR_NOT_READY
    # reference-frame-only modes refuse the flag, at bounces 0 too, with or without an image
    w, h = 64, 48
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0, 0, 3), aspect=w / h))
    ctx.upload_model(suzanne); ctx.set_spheres(rwr.make_spheres()); ctx.resize(w, h)
    for image in (None, IMAGE):
        ctx.sky_set_image(image)
        for params in (rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_SKY_IMAGE | rwr.FLAG_ORTHO_RAYS),
                       rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_SKY_IMAGE | rwr.FLAG_USE_BVH),
                       rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_SKY | rwr.FLAG_SKY_IMAGE | rwr.FLAG_ORTHO_RAYS),
                       rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_SKY | rwr.FLAG_SKY_IMAGE | rwr.FLAG_USE_BVH)):
            with pytest.raises(rwr.RwrError) as ei:
                ctx.render(cam_inv, params)
            assert ei.value.code == rwr.ERR_UNSUPPORTED, params
    with pytest.raises(rwr.RwrError) as ei:
        ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_SKY_IMAGE | rwr.FLAG_ORTHO_RAYS))
    assert "RWR_FLAG_SKY_IMAGE" in ei.value.message
    ctx.set_triangles(rwr.make_triangles([((0.0, 0.0, -2.0), (1.0, 0.0, -2.0), (0.0, 1.0, -2.0))]))
    try:
        for bounces in (0, 1):
            with pytest.raises(rwr.RwrError) as ei:
                ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=bounces, flags=rwr.FLAG_SKY_IMAGE))
            assert ei.value.code == rwr.ERR_UNSUPPORTED
    finally:
        ctx.set_triangles(rwr.make_triangles())
    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=1, flags=rwr.FLAG_SKY | rwr.FLAG_SKY_IMAGE))   # the context is still usable
