"""Soft shadows (RWR_FLAG_SOFT_SHADOWS) on the GPU, against the tests' CPU reference (soft_shadow_ref.c - the oracle's
own routines, brute force over spheres and faces for every shadow ray, the lights' disk drawn from RNG dimensions 130 + 16 k):
  * sample-0 planes bit-exact, colour within 1e-4 (rgba8 within 1), bounce-ray, shadow-ray and occluded counts equal exactly;
  * the anchors: radii 0, the flag without RWR_FLAG_SHADOWS, hard frames around a soft one, the count of shadow rays;
  * every schedule, culling off, frames in flight, bands / strips / the loopback gather, accumulation: the same bytes;
  * reprojection (seed + k, the radii in the key), one frame with sky, a mirror, a glossy part; far from the origin; refusals; the program.
The scenes and radii meet the coverage condition in the reference (tests/test_soft_shadows_host.py): at radius 0.2 the lights' size
changes the answer of 2.6 - 7 % of the shadow rays, in both directions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref
import reproject_ref as rr
import shadow_common as sc
import soft_shadow_ref as ssr
import world_offset_common as woc

pytestmark = pytest.mark.gpu
COLOR_TOL = 1e-4   # the project's bar (tests/test_gpu_shadows.py): the lights' size moves a direction, it adds no rounding to a term
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
SAMPLE0 = ("depth", "obj_id", "hit_t")
RADII = ((0.2, 0.2), (0.3, 0.0))
W, H = sc.W, sc.H


@pytest.fixture(scope="module")
def soft(tmp_path_factory):
    return ssr.lib(tmp_path_factory)


@pytest.fixture
def ctx(gpu_ctx):
    """The session's context; the radii are back at their defaults afterwards."""
    yield gpu_ctx
    gpu_ctx.shadow_set_params()
    gpu_ctx.set_instances(None)


def _flags(rwr, bounces, extra=0, shadows=True, soft=True):
    return (rwr.FLAG_AUX_OUTPUTS | extra | (rwr.FLAG_MULTI_BOUNCE if bounces > 1 else 0) | (rwr.FLAG_SHADOWS if shadows else 0) |
            (rwr.FLAG_SOFT_SHADOWS if soft else 0))


def _upload(ctx, s, w, h):
    model, spheres, inst = s[0], s[1], s[2]
    if isinstance(model, (list, tuple)):
        ctx.upload_parts(model)
    else:
        ctx.upload_model(model)
    ctx.set_instances(inst)
    ctx.set_spheres(spheres)
    ctx.resize(w, h)


def _gpu(rwr, ctx, s, cam_inv, w, h, spp, bounces, seed=7, extra=0, shadows=True, soft=True, radii=None, upload=True, **kw):
    if upload:
        _upload(ctx, s, w, h)
    if radii is not None:
        ctx.shadow_set_params(*radii)
    ctx.render(cam_inv.view(rwr.CAMERA_INV_DTYPE), rwr.make_params(spp=spp, max_bounces=bounces, seed=seed, flags=_flags(rwr, bounces, extra | s[5], shadows, soft)), **kw)
    out = ctx.readback(aux=True)
    out["stats"] = ctx.last_render_stats()
    out["shadow"] = ctx.last_shadow_stats()
    return out


def _same(a, b, what=""):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _check(got, want, what, rows=None, tol=COLOR_TOL):
    sl = slice(None) if rows is None else slice(*rows)
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k][sl].view(np.uint8), want[k][sl].view(np.uint8)), (what, k)
    err = float(np.abs(got["color_f32"][sl] - want["color_f32"][sl]).max())
    print(f"soft shadows colour error {what}: {err:.3g}; shadow rays {got['shadow']} reference {(want['shadow_rays'], want['occluded'])}")
    assert err <= tol, (what, err)
    assert np.abs(got["color"][sl].astype(int) - want["color"][sl].astype(int)).max() <= 1, what
    assert got["stats"][1] == want["rays"], what
    assert got["shadow"] == (want["shadow_rays"], want["occluded"]), what


@pytest.mark.parametrize("name", ["cube", "suzanne_side", "two_parts", "grid", "cube_nmap"])
@pytest.mark.parametrize("bounces", [0, 1, 4])
def test_matches_the_reference(rwr, orc, soft, ctx, suzanne, cube, name, bounces):
    s = sc.scene(name, rwr, orc, suzanne, cube)
    cam_inv = sc.camera(rwr, orc, s)
    upload = True
    for spp in (1, 5):
        for radii in RADII:
            want = ssr.reference(soft, orc, s, cam_inv, W, H, spp, bounces, seed=13, radii=radii, coverage=False)
            got = _gpu(rwr, ctx, s, cam_inv, W, H, spp, bounces, seed=13, radii=radii, upload=upload)
            upload = False
            _check(got, want, f"{name} B={bounces} spp={spp} radii={radii}")
            assert got["stats"][0] == W * H * spp


def test_anchors(rwr, orc, ctx, suzanne, cube):
    """Radii 0 with the flag: the hard frame; the flag without RWR_FLAG_SHADOWS: the frame without either; a hard frame keeps its
    bytes around a soft one; the number of shadow rays does not depend on the flag; the soft frame differs in colour alone."""
    s = sc.scene("suzanne_side", rwr, orc, suzanne, cube)
    cam_inv = sc.camera(rwr, orc, s)
    for spp, bounces in ((1, 0), (4, 1), (3, 3)):
        what = (spp, bounces)
        hard = _gpu(rwr, ctx, s, cam_inv, W, H, spp, bounces, soft=False)
        plain = _gpu(rwr, ctx, s, cam_inv, W, H, spp, bounces, soft=False, shadows=False, upload=False)
        zero = _gpu(rwr, ctx, s, cam_inv, W, H, spp, bounces, radii=(0.0, 0.0), upload=False)
        _same(zero, hard, what + ("radii 0",))
        assert zero["shadow"] == hard["shadow"] and zero["stats"] == hard["stats"]
        alone = _gpu(rwr, ctx, s, cam_inv, W, H, spp, bounces, shadows=False, radii=(0.2, 0.2), upload=False)
        _same(alone, plain, what + ("the flag alone",))
        assert alone["shadow"] == (0, 0) and alone["stats"] == plain["stats"]
        on = _gpu(rwr, ctx, s, cam_inv, W, H, spp, bounces, radii=(0.2, 0.2), upload=False)
        after = _gpu(rwr, ctx, s, cam_inv, W, H, spp, bounces, soft=False, upload=False)
        _same(after, hard, what + ("hard after soft",))
        assert after["shadow"] == hard["shadow"]
        assert on["shadow"][0] == hard["shadow"][0] and on["stats"] == hard["stats"], what
        for k in SAMPLE0:
            assert on[k].tobytes() == hard[k].tobytes(), what + (k,)
        assert on["color_f32"][..., 3].tobytes() == hard["color_f32"][..., 3].tobytes()
        assert on["color_f32"].tobytes() != hard["color_f32"].tobytes(), what
        # one radius 0: the other light alone has a size
        mesh_only = _gpu(rwr, ctx, s, cam_inv, W, H, spp, bounces, radii=(0.2, 0.0), upload=False)
        assert mesh_only["color_f32"].tobytes() != hard["color_f32"].tobytes() and mesh_only["shadow"][0] == hard["shadow"][0]
    # the flag alone at spp 1 without a bounce is the reference frame, from the frame kernel: no wavefront frame, no shadow ray
    ref = _gpu(rwr, ctx, s, cam_inv, W, H, 1, 0, soft=False, shadows=False, upload=False)
    alone = _gpu(rwr, ctx, s, cam_inv, W, H, 1, 0, shadows=False, radii=(0.2, 0.2), upload=False)
    _same(alone, ref, "reference frame")


@pytest.mark.parametrize("scene", ["suzanne_far", "grid"])
def test_schedules_give_the_same_frame(rwr, orc, soft, suzanne, cube, scene):
    """tests/test_gpu_shadows.py's sweep with the lights' size on: dense and listed tiles, Z-split sample shares, one to three ray
    queues, small and large launch groups, packets forced on and off, the wide per-lane kernel on and off, 1-3 frames in flight,
    culling off, whole frame or a band: the same bytes and counts (RNG keys are global pixel and global sample).  The grid's BVH
    does not fit LDS: the NODES_IN_LDS = false form."""
    if scene == "suzanne_far":
        w, h, spp = 200, 72, 7
        s = (suzanne, orc.make_spheres(), None, (2.5, 0.5, 3.0), (0, 0, 0), 0)
    else:
        w, h, spp = 256, 80, 6
        s = (suzanne, orc.make_spheres(), rwr.make_instance_grid(4, 3.0).view(orc.INSTANCE_DTYPE), (9.0, 2.0, 9.0), (0, 0, 0), 0)
    cam_inv = sc.camera(rwr, orc, s, w, h)
    radii = (0.2, 0.2)
    want = ssr.reference(soft, orc, s, cam_inv, w, h, spp, 3, seed=3, radii=radii, coverage=False)
    assert 0.1 <= want["occluded"] / want["shadow_rays"] <= 0.9
    keys = ("RWR_WF_ZSPLIT", "RWR_WF_OVERLAP", "RWR_WF_GROUP", "RWR_WF_PACKET_RAYS", "RWR_WF_MIN_PACKET_POOLS", "RWR_WF_WIDE_LANE")
    saved = {k: os.environ.get(k) for k in keys}
    frames = []
    try:
        for zsplit, queues, group, dense, wide, fif in (("1", "1", "32", "0", "0", 1), ("4", "1", "32", "0", "1", 2),
                                                        ("3", "2", "3", "0", "0", 3), ("0", "3", "4", "0", "1", 2),
                                                        ("1", "1", "32", "40", "0", 1), ("4", "2", "4", "400", "1", 2)):
            os.environ.update({"RWR_WF_ZSPLIT": zsplit, "RWR_WF_OVERLAP": queues, "RWR_WF_GROUP": group, "RWR_WF_PACKET_RAYS": dense,
                               "RWR_WF_MIN_PACKET_POOLS": "0" if dense != "0" else "128", "RWR_WF_WIDE_LANE": wide})
            what = (zsplit, queues, group, dense, wide, fif)
            with rwr.Context(0) as c:        # the tunables are read when the context is created
                c.set_frames_in_flight(fif)
                got = _gpu(rwr, c, s, cam_inv, w, h, spp, 3, seed=3, radii=radii)
                again = _gpu(rwr, c, s, cam_inv, w, h, spp, 3, seed=3, upload=False)   # (zsplit 0: from the live count)
                third = _gpu(rwr, c, s, cam_inv, w, h, spp, 3, seed=3, upload=False)
                nocull = _gpu(rwr, c, s, cam_inv, w, h, spp, 3, seed=3, extra=rwr.FLAG_NO_CULL, upload=False)
                band = _gpu(rwr, c, s, cam_inv, w, h, spp, 3, seed=3, upload=False, rows=(24, 56))
            if not frames:
                _check(got, want, f"schedule {scene} {what}")
            for other in (again, third, nocull):
                _same(got, other, what)
                assert other["shadow"] == got["shadow"] and other["stats"] == got["stats"], what
            for k in PLANES:
                assert np.array_equal(got[k][24:56].view(np.uint8), band[k][24:56].view(np.uint8)), (what, k, "band")
            frames.append(got)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for f in frames[1:]:
        _same(f, frames[0], "schedules")
        assert f["shadow"] == frames[0]["shadow"] and f["stats"] == frames[0]["stats"]


@pytest.mark.parametrize("s_,K", [(1, 4), (3, 3), (16, 2)])
def test_accumulation(rwr, orc, ctx, suzanne, cube, s_, K):
    """K frames of s samples equal one frame of K * s: the disk draws are keyed by the global sample."""
    s = sc.scene("suzanne_side", rwr, orc, suzanne, cube)
    w, h = 120, 64
    cam_inv = sc.camera(rwr, orc, s, w, h).view(rwr.CAMERA_INV_DTYPE)
    _upload(ctx, s, w, h)
    ctx.shadow_set_params(0.2, 0.2)
    for bounces in (0, 3):
        flags = _flags(rwr, bounces)
        ctx.render(cam_inv, rwr.make_params(spp=K * s_, max_bounces=bounces, seed=11, flags=flags))
        want = ctx.readback(aux=True)
        want_rays = ctx.last_shadow_stats()
        ctx.accum_reset()
        total = [0, 0]
        for k in range(1, K + 1):
            ctx.render(cam_inv, rwr.make_params(spp=s_, max_bounces=bounces, seed=11, flags=flags | rwr.FLAG_ACCUMULATE))
            assert ctx.accum_samples() == k * s_
            a, b = ctx.last_shadow_stats()   # its own samples
            total[0] += a; total[1] += b
        _same(ctx.readback(aux=True), want, (s_, K, bounces))
        assert tuple(total) == want_rays, (s_, K, bounces)
        ctx.accum_reset()


def test_accumulation_key_holds_the_radii(rwr, orc, ctx, suzanne, cube):
    """An accepted rwr_shadow_set_params that changes a value restarts the accumulation while the flag is effective, and does not
    while it is off (or cleared: no RWR_FLAG_SHADOWS)."""
    s = sc.scene("suzanne_side", rwr, orc, suzanne, cube)
    cam_inv = sc.camera(rwr, orc, s).view(rwr.CAMERA_INV_DTYPE)
    _upload(ctx, s, W, H)
    for flags, restarts in ((_flags(rwr, 1), True), (_flags(rwr, 1, soft=False), False), (_flags(rwr, 1, shadows=False), False)):
        ctx.accum_reset()
        ctx.shadow_set_params(0.2, 0.2)
        params = rwr.make_params(spp=2, max_bounces=1, seed=4, flags=flags | rwr.FLAG_ACCUMULATE)
        ctx.render(cam_inv, params)
        ctx.render(cam_inv, params)
        assert ctx.accum_samples() == 4
        ctx.shadow_set_params(0.2, 0.2)     # the same values: the key's bytes are the same
        ctx.render(cam_inv, params)
        assert ctx.accum_samples() == 6
        ctx.shadow_set_params(sphere=0.25)
        ctx.render(cam_inv, params)
        assert ctx.accum_samples() == (2 if restarts else 8), (hex(flags), restarts)
        with pytest.raises(rwr.RwrError):
            ctx.shadow_set_params(mesh=2.0)   # refused: nothing changes
        ctx.render(cam_inv, params)
        assert ctx.accum_samples() == (4 if restarts else 10)
    ctx.accum_reset()


@pytest.mark.parametrize("strips", [True, False], ids=["strips", "bands"])
def test_multi_gpu_layouts_assemble_the_frame(rwr, orc, suzanne, cube, strips):
    s = sc.scene("suzanne_side", rwr, orc, suzanne, cube)
    w, h = 203, 67
    cam_inv = sc.camera(rwr, orc, s, w, h).view(rwr.CAMERA_INV_DTYPE)
    params = rwr.make_params(spp=3, max_bounces=3, seed=2, flags=_flags(rwr, 3))
    with rwr.Context(0) as c:
        _upload(c, s, w, h)
        c.shadow_set_params(0.2, 0.2)
        c.render(cam_inv, params)
        full = c.readback(aux=True)
        full_rays = c.last_shadow_stats()
        c.render(cam_inv, rwr.make_params(spp=3, max_bounces=3, seed=2, flags=_flags(rwr, 3, soft=False)))
        assert c.readback(aux=True)["color_f32"].tobytes() != full["color_f32"].tobytes()   # the full frame is a soft one
        for n in (2, 3):
            asm = {k: np.zeros_like(full[k]) for k in PLANES}
            total = [0, 0]
            for r in range(n):
                if strips:
                    c.render(cam_inv, params, strips=(r, n))
                    rows = [y for y in range(h) if (y // 8) % n == r]
                else:
                    band = rwr.dist_band(r, n, h)
                    c.render(cam_inv, params, rows=band)
                    rows = list(range(*band))
                a, b = c.last_shadow_stats()
                total[0] += a; total[1] += b
                part = c.readback(aux=True)
                for k in PLANES:
                    asm[k][rows] = part[k][rows]
                c.dist_loopback_deposit(r, n, strips)
            c.dist_loopback_finish(n, strips)
            _same(asm, full, (strips, n))
            assert tuple(total) == full_rays
            assert np.array_equal(c.dist_readback(), full["color"]), (strips, n)


def test_reprojection(rwr, orc, soft, tmp_path_factory, suzanne, cube):
    """Two reprojecting frames with the flag are the soft frames of seed and seed + 1 (each against the CPU reference) blended by
    reproject_ref.c; the key holds the radii: a changed radius starts a new history, and does not without the flag."""
    s = sc.scene("cube", rwr, orc, suzanne, cube)
    cam_inv = sc.camera(rwr, orc, s)
    cam = cam_inv.view(rwr.CAMERA_INV_DTYPE)
    radii, seed, spp, bounces = (0.2, 0.2), 21, 2, 1
    L = rr.lib(tmp_path_factory)
    nhat = denoise_ref.face_normals(denoise_ref.lib(tmp_path_factory), orc, s[0], None)
    flags = _flags(rwr, bounces)
    with rwr.Context(0) as B:
        plains = [_gpu(rwr, B, s, cam_inv, W, H, spp, bounces, seed=seed + k, radii=radii, upload=k == 0) for k in range(2)]
    for k, f in enumerate(plains):
        _check(f, ssr.reference(soft, orc, s, cam_inv, W, H, spp, bounces, seed=seed + k, radii=radii, coverage=False), f"reproject plain {k}")
    assert plains[0]["color_f32"].tobytes() != plains[1]["color_f32"].tobytes()
    chain = rr.chain(L, plains, nhat, [cam, cam])
    with rwr.Context(0) as A:
        _upload(A, s, W, H)
        A.shadow_set_params(*radii)
        params = rwr.make_params(spp=spp, max_bounces=bounces, seed=seed, flags=flags | rwr.FLAG_REPROJECT)
        for k in range(2):
            A.render(cam, params)
            got = A.readback(aux=True)
            assert A.reproject_frames() == k + 1
            assert A.last_shadow_stats() == plains[k]["shadow"]
            for p in SAMPLE0:
                assert got[p].tobytes() == plains[k][p].tobytes(), (k, p)
            err = float(np.abs(got["color_f32"] - chain[k]["color_f32"]).max())
            print(f"soft shadows reprojection frame {k}: colour error {err:.3g}")
            assert err <= COLOR_TOL, (k, err)
            assert np.abs(got["color"].astype(int) - chain[k]["color"].astype(int)).max() <= 1
            assert A.reproject_history().tobytes() == chain[k]["n"].tobytes()
        A.shadow_set_params(*radii)          # the same values: the history goes on
        A.render(cam, params)
        assert A.reproject_frames() == 3
        A.shadow_set_params(mesh=0.25)       # a changed radius: a new history
        A.render(cam, params)
        assert A.reproject_frames() == 1
        A.render(cam, params)
        assert A.reproject_frames() == 2
        # without the flag the radii are not part of the key
        hard = rwr.make_params(spp=spp, max_bounces=bounces, seed=seed, flags=_flags(rwr, bounces, soft=False) | rwr.FLAG_REPROJECT)
        A.render(cam, hard)
        assert A.reproject_frames() == 1     # (other flags: a new history)
        A.shadow_set_params(mesh=0.3)
        A.render(cam, hard)
        assert A.reproject_frames() == 2


def test_combined_with_sky_mirror_and_gloss(rwr, orc, soft, suzanne, cube):
    """Sky + a mirror sphere + a glossy part + soft shadows in one frame, against the reference."""
    s = sc.scene("two_parts", rwr, orc, suzanne, cube)
    cam_inv = sc.camera(rwr, orc, s)
    sky = ((0.5, 0.7, 1.0), (1.0, 1.0, 1.0))
    rough = 0.25
    radii = (0.2, 0.2)
    want = ssr.reference(soft, orc, s, cam_inv, W, H, 4, 3, seed=9, radii=radii, coverage=False, sky=sky, mirror_spheres={0: (0.9, 0.9, 0.9)},
                         gloss_parts={1: (rough, (0.8, 0.7, 0.6))})
    hard = ssr.reference(soft, orc, s, cam_inv, W, H, 4, 3, seed=9, coverage=False, sky=sky, mirror_spheres={0: (0.9, 0.9, 0.9)},
                         gloss_parts={1: (rough, (0.8, 0.7, 0.6))})
    assert want["glossy"] > 0 and want["sky_terms"] > 0 and want["color_f32"].tobytes() != hard["color_f32"].tobytes()
    extra = rwr.FLAG_SKY | rwr.FLAG_MIRRORS | rwr.FLAG_GLOSSY
    with rwr.Context(0) as c:
        _upload(c, s, W, H)
        c.sky_set_params(*sky)
        c.set_sphere_mirror(0, (0.9, 0.9, 0.9))
        c.set_part_gloss(1, rough, (0.8, 0.7, 0.6))
        got = _gpu(rwr, c, s, cam_inv, W, H, 4, 3, seed=9, extra=extra, radii=radii, upload=False)
        assert c.last_gloss_stats() == want["glossy"]
    _check(got, want, "sky + mirror sphere + glossy part + soft shadows")


def test_far_from_the_origin(rwr, orc, soft, ctx, ref_loader, res_dir):
    """tests/world_offset_common.py's scenes moved by 1e4: counts and planes still equal the reference's."""
    off = woc.OFFSETS["1e4"]
    meshes = woc.meshes(ref_loader, res_dir)
    w, h = 96, 64
    for name in ("suzanne", "cube", "soup257"):
        model = woc.translated(meshes[name][0], off)
        spheres = woc.spheres_at(rwr, off, [((1.6, 1.2, 1.4), 0.5)]).view(orc.SPHERE_DTYPE)
        eye, target = tuple(np.add((2.5, 0.5, 1.0), off)), tuple(np.add((0.0, 0.0, 0.0), off))
        s = (model, spheres, None, eye, target, 0)
        cam_inv = sc.camera(rwr, orc, s, w, h)
        want = ssr.reference(soft, orc, s, cam_inv, w, h, 3, 2, seed=5, radii=(0.2, 0.2), coverage=False)
        assert want["shadow_rays"] > 100 and 0 < want["occluded"] < want["shadow_rays"], (name, want["shadow_rays"], want["occluded"])
        got = _gpu(rwr, ctx, s, cam_inv, w, h, 3, 2, seed=5, radii=(0.2, 0.2))
        _check(got, want, f"far {name} spp=3 B=2")


def test_refusals_and_null_arguments(rwr, orc, ctx, suzanne, cube):
    s = sc.scene("suzanne_side", rwr, orc, suzanne, cube)
    cam_inv = sc.camera(rwr, orc, s).view(rwr.CAMERA_INV_DTYPE)
    _upload(ctx, s, W, H)
    both = rwr.FLAG_SHADOWS | rwr.FLAG_SOFT_SHADOWS
    for params in (rwr.make_params(flags=both | rwr.FLAG_ORTHO_RAYS), rwr.make_params(flags=both | rwr.FLAG_USE_BVH),
                   rwr.make_params(spp=2, max_bounces=1, flags=both | rwr.FLAG_USE_BVH), rwr.make_params(flags=rwr.FLAG_SOFT_SHADOWS | rwr.FLAG_USE_BVH)):
        with pytest.raises(rwr.RwrError) as ei:
            ctx.render(cam_inv, params)
        assert ei.value.code == rwr.ERR_UNSUPPORTED, params
    with pytest.raises(rwr.RwrError) as ei:      # the flag alone is refused in its own name; with RWR_FLAG_SHADOWS that flag's refusal keeps its text
        ctx.render(cam_inv, rwr.make_params(flags=rwr.FLAG_SOFT_SHADOWS | rwr.FLAG_ORTHO_RAYS))
    assert ei.value.code == rwr.ERR_UNSUPPORTED and "RWR_FLAG_SOFT_SHADOWS" in ei.value.message
    with pytest.raises(rwr.RwrError) as ei:
        ctx.render(cam_inv, rwr.make_params(flags=both | rwr.FLAG_ORTHO_RAYS))
    assert "RWR_FLAG_SHADOWS:" in ei.value.message
    ctx.set_triangles(rwr.make_triangles([((0, 0, -1), (1, 0, -1), (0, 1, -1))]))
    try:
        for flags in (both, rwr.FLAG_SOFT_SHADOWS):
            with pytest.raises(rwr.RwrError) as ei:
                ctx.render(cam_inv, rwr.make_params(flags=flags))
            assert ei.value.code == rwr.ERR_UNSUPPORTED
    finally:
        ctx.set_triangles(rwr.make_triangles())
    # the context is still usable
    ctx.shadow_set_params(0.2, 0.2)
    ctx.render(cam_inv, rwr.make_params(flags=both))
    rays, occluded = ctx.last_shadow_stats()
    assert rays > 0 and 0 < occluded < rays
    # the parameters: the getter round-trips, NULL restores the defaults, anything out of range is refused and the old values stay
    ctx.shadow_set_params(0.125, 0.75)
    assert ctx.shadow_get_params() == {"mesh": np.float32(0.125), "sphere": np.float32(0.75)}
    ctx.shadow_set_params(sphere=0.5)
    assert ctx.shadow_get_params() == {"mesh": np.float32(0.125), "sphere": np.float32(0.5)}
    for bad in ({"mesh": -0.01}, {"mesh": 1.0001}, {"sphere": -1.0}, {"sphere": 2.0}, {"mesh": float("inf")}, {"sphere": float("-inf")},
                {"mesh": float("nan")}, {"sphere": float("nan")}, {"mesh": float("nan"), "sphere": 0.1}):
        with pytest.raises(rwr.RwrError) as ei:
            ctx.shadow_set_params(**bad)
        assert ei.value.code == rwr.ERR_INVALID_ARGUMENT, bad
        assert ctx.shadow_get_params() == {"mesh": np.float32(0.125), "sphere": np.float32(0.5)}, bad
    ctx.shadow_set_params(0.0, 1.0)   # the ends of the range
    assert ctx.shadow_get_params() == {"mesh": np.float32(0.0), "sphere": np.float32(1.0)}
    ctx.shadow_set_params()
    assert ctx.shadow_get_params() == {"mesh": np.float32(0.05), "sphere": np.float32(0.05)}
    L = rwr.lib()
    p = np.zeros(1, rwr.SHADOW_PARAMS_DTYPE)
    vp = p.ctypes.data_as(C.c_void_p)
    assert L.rwr_shadow_set_params(None, vp) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_shadow_get_params(None, vp) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_shadow_get_params(ctx._h, None) == rwr.ERR_INVALID_ARGUMENT
    assert ctx.shadow_get_params() == {"mesh": np.float32(0.05), "sphere": np.float32(0.05)}


def test_cli_soft_shadows(rwr, ctx, suzanne, tmp_path):
    """rwr_render --soft-shadows 0.2 --spp 4 --bounces 3 writes the PNG the driver writes of its own frame with the flag and those
    radii, and not the hard frame's.  (The program's start camera sits inside the mesh, where every shadow ray is occluded whatever
    the lights' size: eight key steps to the right first, to a view with shadow edges - in the CPU reference 14 pixels of that frame
    differ in rgba8 between the soft and the hard frame, by up to 13 levels.)"""
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")
    w, h = 96, 64
    out = str(tmp_path / "soft.png")
    r = subprocess.run([exe, "--res", rwr.RES_DIR, "--size", f"{w}x{h}", "--keys", "D*8", "--frames", "1", "--spp", "4", "--bounces", "3", "--soft-shadows", "0.2",
                        "--out", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cam = rwr.make_camera(aspect=w / h)
    for keys in [rwr.KEY_RIGHT] * 8 + [0]:
        cam = rwr.circle_controller_update(cam, keys)
    cam_inv = rwr.camera_build_inv_uniform(cam)
    ctx.upload_model(suzanne); ctx.set_instances(None); ctx.set_spheres(rwr.make_spheres()); ctx.resize(w, h)
    ctx.shadow_set_params(0.2, 0.2)

    def driver_png(flags, name):
        ctx.render(cam_inv, rwr.make_params(spp=4, max_bounces=3, seed=0, flags=flags))
        path = str(tmp_path / name)
        rwr.write_png(path, ctx.readback()["color"], flip_vertical=True, encode_srgb=True)
        return open(path, "rb").read()

    assert open(out, "rb").read() == driver_png(rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_SHADOWS | rwr.FLAG_SOFT_SHADOWS, "driver.png")
    assert open(out, "rb").read() != driver_png(rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_SHADOWS, "driver_hard.png")
    assert "--soft-shadows" in subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
