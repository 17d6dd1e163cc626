"""Shadow rays (RWR_FLAG_SHADOWS) on the GPU, against the tests' CPU reference (shadow_ref.c - the oracle's own
routines, brute force over spheres and faces for every shadow ray):
  * sample-0 planes bit-exact, colour within 1e-4 (rgba8 within 1), bounce-ray, shadow-ray and occluded counts equal exactly;
  * every schedule, culling off, frames in flight, bands / strips / the loopback gather, accumulation: the same bytes;
  * frames without the flag around one with it keep their bytes; a scene far from the origin; a random slice; refusals; the program.
The scenes and the coverage condition they meet in the reference (a tenth of the shadow rays on either side): shadow_common.py."""
import os
import subprocess
import time

import numpy as np
import pytest

import fuzz_common
import shadow_common as sc
import shadow_ref
import world_offset_common as woc

pytestmark = pytest.mark.gpu
COLOR_TOL = 1e-4   # the project's bar (tests/test_gpu_multi_bounce.py), unchanged for deeper paths: shadows add a select, no rounding
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return shadow_ref.lib(tmp_path_factory)


def _flags(rwr, bounces, extra=0, shadows=True):
    return rwr.FLAG_AUX_OUTPUTS | extra | (rwr.FLAG_MULTI_BOUNCE if bounces > 1 else 0) | (rwr.FLAG_SHADOWS if shadows else 0)


def _upload(ctx, s, w, h):
    model, spheres, inst = s[0], s[1], s[2]
    if isinstance(model, (list, tuple)):
        ctx.upload_parts(model)
    else:
        ctx.upload_model(model)
    ctx.set_instances(inst)
    ctx.set_spheres(spheres)
    ctx.resize(w, h)


def _gpu(rwr, ctx, s, cam_inv, w, h, spp, bounces, seed=7, extra=0, shadows=True, upload=True, **kw):
    if upload:
        _upload(ctx, s, w, h)
    ctx.render(cam_inv.view(rwr.CAMERA_INV_DTYPE), rwr.make_params(spp=spp, max_bounces=bounces, seed=seed, flags=_flags(rwr, bounces, extra | s[5], shadows)), **kw)
    out = ctx.readback(aux=True)
    out["stats"] = ctx.last_render_stats()
    out["shadow"] = ctx.last_shadow_stats()
    return out


def _same(a, b, what=""):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _check(got, want, what, rows=None):
    sl = slice(None) if rows is None else slice(*rows)
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k][sl].view(np.uint8), want[k][sl].view(np.uint8)), (what, k)
    err = float(np.abs(got["color_f32"][sl] - want["color_f32"][sl]).max())
    print(f"shadows colour error {what}: {err:.3g}; shadow rays {got['shadow']} reference {(want['shadow_rays'], want['occluded'])}")
    assert err <= COLOR_TOL, (what, err)
    assert np.abs(got["color"][sl].astype(int) - want["color"][sl].astype(int)).max() <= 1, what
    assert got["stats"][1] == want["rays"], what
    assert got["shadow"] == (want["shadow_rays"], want["occluded"]), what


@pytest.mark.parametrize("name", list(sc.SCENES))
@pytest.mark.parametrize("bounces", [0, 1, 4])
def test_matches_the_reference(rwr, orc, sref, gpu_ctx, suzanne, cube, name, bounces):
    s = sc.scene(name, rwr, orc, suzanne, cube)
    cam_inv = sc.camera(rwr, orc, s)
    for spp in (1, 5):
        want = sc.reference(shadow_ref, sref, orc, s, cam_inv, sc.W, sc.H, spp, bounces, seed=13)
        if spp == 1 and bounces == 0:
            sc.check_class(name, want)   # the coverage condition: neither "always lit" nor "always dark" would pass a mixed scene
        got = _gpu(rwr, gpu_ctx, s, cam_inv, sc.W, sc.H, spp, bounces, seed=13)
        _check(got, want, f"{name} B={bounces} spp={spp}")
        assert got["stats"][0] == sc.W * sc.H * spp
    gpu_ctx.set_instances(None)


def test_frames_without_the_flag_keep_their_bytes_and_count_nothing(rwr, orc, gpu_ctx, suzanne, cube):
    s = sc.scene("suzanne_side", rwr, orc, suzanne, cube)
    cam_inv = sc.camera(rwr, orc, s)
    for spp, bounces in ((1, 0), (4, 1), (3, 3)):
        before = _gpu(rwr, gpu_ctx, s, cam_inv, sc.W, sc.H, spp, bounces, shadows=False)
        assert before["shadow"] == (0, 0)
        with_flag = _gpu(rwr, gpu_ctx, s, cam_inv, sc.W, sc.H, spp, bounces, upload=False)
        assert with_flag["shadow"][0] > 0
        after = _gpu(rwr, gpu_ctx, s, cam_inv, sc.W, sc.H, spp, bounces, shadows=False, upload=False)
        _same(before, after, (spp, bounces))
        assert after["shadow"] == (0, 0) and before["stats"] == after["stats"] == with_flag["stats"]
        for k in ("depth", "obj_id", "hit_t"):
            assert with_flag[k].tobytes() == before[k].tobytes(), k
        assert (with_flag["color_f32"] <= before["color_f32"] + 2e-4).all()
        assert (with_flag["color_f32"][..., :3] < before["color_f32"][..., :3] - 1e-3).any()


@pytest.mark.parametrize("scene", ["suzanne_far", "grid"])
def test_schedules_give_the_same_frame(rwr, orc, sref, suzanne, cube, scene):
    """Dense and listed tiles, Z-split sample shares, one to three ray queues, small and large launch groups, packets forced on
    and off, the wide per-lane kernel on and off (its SHADOW forms; the grid's BVH is the one large enough to take it), 1-3 frames
    in flight, culling off, whole frame or a band: the same bytes and counts."""
    if scene == "suzanne_far":
        w, h, spp = 200, 72, 7
        s = (suzanne, orc.make_spheres(), None, (2.5, 0.5, 3.0), (0, 0, 0), 0)
    else:
        w, h, spp = 256, 80, 6
        s = (suzanne, orc.make_spheres(), rwr.make_instance_grid(4, 3.0).view(orc.INSTANCE_DTYPE), (9.0, 2.0, 9.0), (0, 0, 0), 0)
    cam_inv = sc.camera(rwr, orc, s, w, h)
    want = sc.reference(shadow_ref, sref, orc, s, cam_inv, w, h, spp, 3, seed=3)
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
            with rwr.Context(0) as ctx:        # the tunables are read when the context is created
                ctx.set_frames_in_flight(fif)
                got = _gpu(rwr, ctx, s, cam_inv, w, h, spp, 3, seed=3)
                again = _gpu(rwr, ctx, s, cam_inv, w, h, spp, 3, seed=3, upload=False)   # (zsplit 0: from the live count)
                third = _gpu(rwr, ctx, s, cam_inv, w, h, spp, 3, seed=3, upload=False)
                nocull = _gpu(rwr, ctx, s, cam_inv, w, h, spp, 3, seed=3, extra=rwr.FLAG_NO_CULL, upload=False)
                band = _gpu(rwr, ctx, s, cam_inv, w, h, spp, 3, seed=3, upload=False, rows=(24, 56))
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


@pytest.mark.parametrize("s_,K", [(1, 4), (3, 3), (16, 2)])
def test_accumulation(rwr, orc, gpu_ctx, suzanne, cube, s_, K):
    s = sc.scene("suzanne_side", rwr, orc, suzanne, cube)
    w, h = 120, 64
    cam_inv = sc.camera(rwr, orc, s, w, h).view(rwr.CAMERA_INV_DTYPE)
    _upload(gpu_ctx, s, w, h)
    for bounces in (0, 3):
        flags = _flags(rwr, bounces)
        gpu_ctx.render(cam_inv, rwr.make_params(spp=K * s_, max_bounces=bounces, seed=11, flags=flags))
        want = gpu_ctx.readback(aux=True)
        want_rays = gpu_ctx.last_shadow_stats()
        gpu_ctx.accum_reset()
        total = [0, 0]
        for k in range(1, K + 1):
            gpu_ctx.render(cam_inv, rwr.make_params(spp=s_, max_bounces=bounces, seed=11, flags=flags | rwr.FLAG_ACCUMULATE))
            assert gpu_ctx.accum_samples() == k * s_
            a, b = gpu_ctx.last_shadow_stats()   # its own samples
            total[0] += a; total[1] += b
        _same(gpu_ctx.readback(aux=True), want, (s_, K, bounces))
        assert tuple(total) == want_rays, (s_, K, bounces)
        gpu_ctx.accum_reset()


@pytest.mark.parametrize("strips", [True, False], ids=["strips", "bands"])
def test_multi_gpu_layouts_assemble_the_frame(rwr, orc, suzanne, cube, strips):
    s = sc.scene("suzanne_side", rwr, orc, suzanne, cube)
    w, h = 203, 67
    cam_inv = sc.camera(rwr, orc, s, w, h).view(rwr.CAMERA_INV_DTYPE)
    params = rwr.make_params(spp=3, max_bounces=3, seed=2, flags=_flags(rwr, 3))
    with rwr.Context(0) as ctx:
        _upload(ctx, s, w, h)
        ctx.render(cam_inv, params)
        full = ctx.readback(aux=True)
        full_rays = ctx.last_shadow_stats()
        for n in (2, 3):
            asm = {k: np.zeros_like(full[k]) for k in PLANES}
            total = [0, 0]
            for r in range(n):
                if strips:
                    ctx.render(cam_inv, params, strips=(r, n))
                    rows = [y for y in range(h) if (y // 8) % n == r]
                else:
                    band = rwr.dist_band(r, n, h)
                    ctx.render(cam_inv, params, rows=band)
                    rows = list(range(*band))
                a, b = ctx.last_shadow_stats()
                total[0] += a; total[1] += b
                part = ctx.readback(aux=True)
                for k in PLANES:
                    asm[k][rows] = part[k][rows]
                ctx.dist_loopback_deposit(r, n, strips)
            ctx.dist_loopback_finish(n, strips)
            _same(asm, full, (strips, n))
            assert tuple(total) == full_rays
            assert np.array_equal(ctx.dist_readback(), full["color"]), (strips, n)


def test_far_from_the_origin(rwr, orc, sref, gpu_ctx, ref_loader, res_dir):
    """tests/world_offset_common.py's scenes moved by 1e4: counts and planes still equal the reference's."""
    off = woc.OFFSETS["1e4"]
    meshes = woc.meshes(ref_loader, res_dir)
    names = ("suzanne", "cube", "soup257")
    w, h = 96, 64
    for name in names:
        model = woc.translated(meshes[name][0], off)
        spheres = woc.spheres_at(rwr, off, [((1.6, 1.2, 1.4), 0.5)]).view(orc.SPHERE_DTYPE)
        eye, target = tuple(np.add((2.5, 0.5, 1.0), off)), tuple(np.add((0.0, 0.0, 0.0), off))
        s = (model, spheres, None, eye, target, 0)
        cam_inv = sc.camera(rwr, orc, s, w, h)
        for spp, bounces in ((1, 0), (3, 2)):
            want = sc.reference(shadow_ref, sref, orc, s, cam_inv, w, h, spp, bounces, seed=5)
            assert want["shadow_rays"] > 100 and 0 < want["occluded"] < want["shadow_rays"], (name, want["shadow_rays"], want["occluded"])
            got = _gpu(rwr, gpu_ctx, s, cam_inv, w, h, spp, bounces, seed=5)
            _check(got, want, f"far {name} spp={spp} B={bounces}")


def test_random_slice(rwr, orc, sref, ref_loader, suzanne):
    """Soups of 1-1 500 faces, spheres, instances, 1-3 frames in flight, against the reference with the counts compared exactly."""
    rng = np.random.default_rng(4242)
    t_end = time.time() + 45.0
    n = mixed = 0
    with rwr.Context(0) as ctx:
        while time.time() < t_end or n < 8:
            n_faces = int(rng.choice([1, 2, 7, 64, 65, 129, 256, 300, 777, 1500]))
            model = fuzz_common.soup(ref_loader, rng, n_faces, extent=float(rng.choice([0.5, 2.5])), tri_size=float(rng.choice([0.05, 0.4, 1.5])), tex=suzanne["texture"])
            w, h = int(rng.integers(8, 130)), int(rng.integers(8, 90))
            spheres = orc.make_spheres([(tuple(rng.uniform(-3, 3, 3)), float(rng.uniform(0.05, 1.5))) for _ in range(int(rng.integers(0, 9)))])
            inst = None
            if rng.random() < 0.4 and n_faces < 400:
                k = int(rng.integers(2, 5))
                inst = np.zeros(k, dtype=orc.INSTANCE_DTYPE)
                for i in range(k):
                    m = np.eye(4, dtype=np.float32)
                    m[3, :3] = rng.uniform(-3, 3, 3)
                    inst["model"][i] = m
            spp, bounces = int(rng.choice([1, 2, 5])), int(rng.choice([0, 1, 3]))
            if w * h * n_faces * (1 if inst is None else len(inst)) * spp * (1 + bounces) > 3e7:
                spp, bounces = 1, int(bounces > 0)
            s = (model, spheres, inst, tuple(rng.uniform(-4, 4, 3)), tuple(rng.uniform(-1, 1, 3)), 0)
            cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=s[3], target=s[4], aspect=w / h, fovy=float(rng.uniform(20, 110)))).view(orc.CAMERA_INV_DTYPE)
            ctx.set_frames_in_flight(int(rng.integers(1, 4)))
            seed = int(rng.integers(0, 1000))
            want = sc.reference(shadow_ref, sref, orc, s, cam_inv, w, h, spp, bounces, seed=seed)
            got = _gpu(rwr, ctx, s, cam_inv, w, h, spp, bounces, seed=seed)
            _check(got, want, f"random {n}: {n_faces} faces {w}x{h} spp={spp} B={bounces}")
            n += 1
            mixed += 0 < want["occluded"] < want["shadow_rays"]
    assert n >= 8 and mixed >= 4, (n, mixed)


def test_refusals_and_null_arguments(rwr, orc, gpu_ctx, suzanne, cube):
    import ctypes as C
    s = sc.scene("suzanne_side", rwr, orc, suzanne, cube)
    cam_inv = sc.camera(rwr, orc, s).view(rwr.CAMERA_INV_DTYPE)
    _upload(gpu_ctx, s, sc.W, sc.H)
    for params in (rwr.make_params(flags=rwr.FLAG_SHADOWS | rwr.FLAG_ORTHO_RAYS), rwr.make_params(flags=rwr.FLAG_SHADOWS | rwr.FLAG_USE_BVH),
                   rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_SHADOWS | rwr.FLAG_USE_BVH)):
        with pytest.raises(rwr.RwrError) as ei:
            gpu_ctx.render(cam_inv, params)
        assert ei.value.code == rwr.ERR_UNSUPPORTED, params
    gpu_ctx.set_triangles(rwr.make_triangles([((0, 0, -1), (1, 0, -1), (0, 1, -1))]))
    try:
        with pytest.raises(rwr.RwrError) as ei:
            gpu_ctx.render(cam_inv, rwr.make_params(flags=rwr.FLAG_SHADOWS))
        assert ei.value.code == rwr.ERR_UNSUPPORTED
    finally:
        gpu_ctx.set_triangles(rwr.make_triangles())
    # the context is still usable
    gpu_ctx.render(cam_inv, rwr.make_params(flags=rwr.FLAG_SHADOWS))
    rays, occluded = gpu_ctx.last_shadow_stats()
    assert rays > 0 and 0 < occluded < rays
    L = rwr.lib()
    a = C.c_uint64()
    assert L.rwr_last_shadow_stats(None, C.byref(a), C.byref(a)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_last_shadow_stats(gpu_ctx._h, None, C.byref(a)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_last_shadow_stats(gpu_ctx._h, C.byref(a), None) == rwr.ERR_INVALID_ARGUMENT
    assert gpu_ctx.last_shadow_stats() == (rays, occluded)


def test_cli_shadows(rwr, gpu_ctx, suzanne, tmp_path):
    """rwr_render --shadows --spp 4 --bounces 3 writes the PNG the driver writes of its own frame with the flag."""
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")
    w, h = 96, 64
    out = str(tmp_path / "shadows.png")
    r = subprocess.run([exe, "--res", rwr.RES_DIR, "--size", f"{w}x{h}", "--keys", "-*1", "--frames", "1", "--spp", "4", "--bounces", "3", "--shadows",
                        "--out", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(aspect=w / h))
    gpu_ctx.upload_model(suzanne); gpu_ctx.set_instances(None); gpu_ctx.set_spheres(rwr.make_spheres()); gpu_ctx.resize(w, h)

    def driver_png(flags, name):
        gpu_ctx.render(cam_inv, rwr.make_params(spp=4, max_bounces=3, seed=0, flags=flags))
        path = str(tmp_path / name)
        rwr.write_png(path, gpu_ctx.readback()["color"], flip_vertical=True, encode_srgb=True)
        return open(path, "rb").read()

    assert open(out, "rb").read() == driver_png(rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_SHADOWS, "driver.png")
    assert open(out, "rb").read() != driver_png(rwr.FLAG_MULTI_BOUNCE, "driver_plain.png")
    assert "--shadows" in subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
