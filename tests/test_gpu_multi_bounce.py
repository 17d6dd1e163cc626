"""Deeper paths (RWR_FLAG_MULTI_BOUNCE) on the GPU: the wavefront integrator's generation loop against the tests'
CPU reference (path_ref.c — the oracle's own routines with the definition's path loop):
  * sample-0 planes (object id, distance, depth) bit-exact, colour within 1e-4 (rgba8 within 1), the bounce-ray count equal;
  * with the flag and max_bounces <= 1 the frame of no flag, byte for byte; the limits;
  * every schedule, accumulation, bands / strips / the loopback gather: the same bytes at B = 3.
The throughput travels as unorm16 and is re-quantised every generation, so the colour error grows with B: the largest one seen
is printed (run with -s)."""
import os
import subprocess

import numpy as np
import pytest

import path_ref

pytestmark = pytest.mark.gpu
COLOR_TOL = 1e-4
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
_worst = {}


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return path_ref.lib(tmp_path_factory)


def _flags(rwr, bounces, extra=0):
    return rwr.FLAG_AUX_OUTPUTS | extra | (rwr.FLAG_MULTI_BOUNCE if bounces > 1 else 0)


def _gpu(rwr, ctx, model, spheres, cam_inv, w, h, params, instances=None, **kw):
    if isinstance(model, (list, tuple)):
        ctx.upload_parts(model)
    else:
        ctx.upload_model(model)
    ctx.set_instances(instances)
    ctx.set_spheres(spheres)
    ctx.resize(w, h)
    ctx.render(cam_inv, params, **kw)
    out = ctx.readback(aux=True)
    out["stats"] = ctx.last_render_stats()
    return out


def _same(a, b, what=""):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _check(got, want, what, rows=None):
    sl = slice(None) if rows is None else slice(*rows)
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k][sl].view(np.uint8), want[k][sl].view(np.uint8)), (what, k)
    err = float(np.abs(got["color_f32"][sl] - want["color_f32"][sl]).max())
    _worst[what] = err
    print(f"multi-bounce colour error {what}: {err:.3g} (largest so far {max(_worst.values()):.3g})")
    assert err <= COLOR_TOL, (what, err)
    assert np.abs(got["color"][sl].astype(int) - want["color"][sl].astype(int)).max() <= 1, what


SCENES = ["suzanne_front", "suzanne_near", "suzanne_side", "inside_cube", "grid4", "two_parts", "cube_nmap"]


def _scene(name, rwr, suzanne, cube):
    """(model, spheres, instances, eye, target, extra flags, w, h)"""
    sph = rwr.make_spheres()
    if name == "suzanne_front":
        return suzanne, sph, None, (0, 0, 3), (0.2, 0.2, -2.0), 0, 96, 54
    if name == "suzanne_near":
        return suzanne, sph, None, (0, 0, 0), (0.2, 0.2, -2.0), 0, 96, 54
    if name == "suzanne_side":
        return suzanne, sph, None, (2.4, 0.9, 1.0), (0.2, 0.2, -2.0), 0, 96, 54
    if name == "inside_cube":
        return cube, rwr.make_spheres([]), None, (0.1, 0.2, 0.3), (0.0, 0.0, -1.0), 0, 80, 60
    if name == "grid4":
        return suzanne, sph, rwr.make_instance_grid(4, 3.0), (0, 0, 12), (0, 0, 0), 0, 96, 64
    if name == "two_parts":
        return [suzanne, cube], sph, rwr.make_instance_grid(2, 3.0), (-1.5, 1.0, 6.0), (-1.5, 0, 0), 0, 96, 64
    if name == "cube_nmap":
        return cube, rwr.make_spheres([((1.6, 1.2, 1.4), 0.5)]), None, (2.2, 1.7, 3.1), (0, 0, 0), rwr.FLAG_NORMAL_MAP, 80, 60
    raise KeyError(name)


def _reference(pref, orc, rwr, scene, cam_inv, spp, bounces, seed, rows=None):
    model, spheres, inst, _, _, extra, w, h = scene
    return path_ref.render_path(pref, orc, cam_inv.view(orc.CAMERA_INV_DTYPE), orc.make_screen(w, h),
                                orc.make_params(spp, bounces, seed=seed, flags=extra), spheres.view(orc.SPHERE_DTYPE), model,
                                instances=None if inst is None else inst.view(orc.INSTANCE_DTYPE), rows=rows)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("bounces", [2, 3, 8])
def test_matches_the_reference(rwr, orc, pref, gpu_ctx, suzanne, cube, name, bounces):
    scene = _scene(name, rwr, suzanne, cube)
    model, spheres, inst, eye, target, extra, w, h = scene
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=eye, target=target, aspect=w / h))
    for spp in (1, 5):
        params = rwr.make_params(spp=spp, max_bounces=bounces, seed=13, flags=_flags(rwr, bounces, extra))
        got = _gpu(rwr, gpu_ctx, model, spheres, cam_inv, w, h, params, instances=inst)
        want = _reference(pref, orc, rwr, scene, cam_inv, spp, bounces, 13)
        _check(got, want, f"{name} B={bounces} spp={spp}")
        primary, bounce_rays = got["stats"]
        assert primary == w * h * spp
        assert bounce_rays == want["rays"], (name, bounces, spp)
        if name == "inside_cube":
            assert bounce_rays == w * h * spp * bounces
    gpu_ctx.set_instances(None)


def test_flag_at_one_bounce_or_none_changes_nothing_and_the_limits(rwr, gpu_ctx, suzanne):
    w, h = 96, 54
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0, 0, 3), target=(0.2, 0.2, -2.0), aspect=w / h))
    for spp, bounces in ((1, 0), (3, 0), (1, 1), (4, 1)):
        plain = _gpu(rwr, gpu_ctx, suzanne, rwr.make_spheres(), cam_inv, w, h,
                     rwr.make_params(spp=spp, max_bounces=bounces, seed=5, flags=rwr.FLAG_AUX_OUTPUTS))
        flagged = _gpu(rwr, gpu_ctx, suzanne, rwr.make_spheres(), cam_inv, w, h,
                       rwr.make_params(spp=spp, max_bounces=bounces, seed=5, flags=rwr.FLAG_AUX_OUTPUTS | rwr.FLAG_MULTI_BOUNCE))
        _same(plain, flagged, (spp, bounces))
        assert plain["stats"] == flagged["stats"]
    for params, code in ((rwr.make_params(spp=2, max_bounces=2), rwr.ERR_UNSUPPORTED),
                         (rwr.make_params(spp=2, max_bounces=9, flags=rwr.FLAG_MULTI_BOUNCE), rwr.ERR_INVALID_ARGUMENT),
                         (rwr.make_params(spp=2, max_bounces=100, flags=rwr.FLAG_MULTI_BOUNCE), rwr.ERR_INVALID_ARGUMENT),
                         (rwr.make_params(spp=1, max_bounces=2, flags=rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_USE_BVH), rwr.ERR_UNSUPPORTED),
                         (rwr.make_params(spp=1, max_bounces=2, flags=rwr.FLAG_MULTI_BOUNCE | rwr.FLAG_ORTHO_RAYS), rwr.ERR_UNSUPPORTED)):
        with pytest.raises(rwr.RwrError) as ei:
            gpu_ctx.render(cam_inv, params)
        assert ei.value.code == code, params
    # the deepest path allowed renders
    gpu_ctx.render(cam_inv, rwr.make_params(spp=2, max_bounces=rwr.MAX_BOUNCES, flags=rwr.FLAG_MULTI_BOUNCE))


@pytest.mark.parametrize("scene", ["suzanne_far", "grid"])
def test_schedules_give_the_same_frame(rwr, orc, pref, suzanne, scene):
    """Dense and listed tiles, Z-split sample shares, one to three ray queues, groups of 3 ... 64 samples, packet thresholds
    forced on and off, the wide per-lane kernel on and off, 1-3 frames in flight, whole frame or a band: the same bytes at B = 3,
    and the reference's frame."""
    if scene == "suzanne_far":
        w, h, eye, inst, spp = 200, 72, (0, 0, 3), None, 7
    else:
        w, h, eye, inst, spp = 256, 80, (0, 0, 12), rwr.make_instance_grid(4, 3.0), 6
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=eye, aspect=w / h))
    params = rwr.make_params(spp=spp, max_bounces=3, seed=3, flags=_flags(rwr, 3))
    sc = (suzanne, rwr.make_spheres(), inst, eye, (0, 0, -1), 0, w, h)
    want = _reference(pref, orc, rwr, sc, cam_inv, spp, 3, 3)
    keys = ("RWR_WF_ZSPLIT", "RWR_WF_OVERLAP", "RWR_WF_GROUP", "RWR_WF_PACKET_RAYS", "RWR_WF_MIN_PACKET_POOLS", "RWR_WF_WIDE_LANE")
    saved = {k: os.environ.get(k) for k in keys}
    frames = []
    try:
        for zsplit, queues, group, dense, wide, fif in (("1", "1", "32", "0", "0", 1), ("4", "1", "32", "0", "1", 2),
                                                        ("3", "2", "3", "0", "0", 3), ("1", "2", "64", "0", "1", 1),
                                                        ("0", "3", "4", "0", "1", 2), ("8", "3", "5", "0", "0", 3),
                                                        ("1", "1", "32", "40", "0", 1), ("4", "2", "4", "400", "1", 2)):
            os.environ.update({"RWR_WF_ZSPLIT": zsplit, "RWR_WF_OVERLAP": queues, "RWR_WF_GROUP": group, "RWR_WF_PACKET_RAYS": dense,
                               "RWR_WF_MIN_PACKET_POOLS": "0" if dense != "0" else "128", "RWR_WF_WIDE_LANE": wide})
            what = (zsplit, queues, group, dense, wide, fif)
            with rwr.Context(0) as ctx:        # the tunables are read when the context is created
                ctx.set_frames_in_flight(fif)
                got = _gpu(rwr, ctx, suzanne, rwr.make_spheres(), cam_inv, w, h, params, instances=inst)
                again = _gpu(rwr, ctx, suzanne, rwr.make_spheres(), cam_inv, w, h, params, instances=inst)   # (zsplit 0: from the live count)
                third = _gpu(rwr, ctx, suzanne, rwr.make_spheres(), cam_inv, w, h, params, instances=inst)
                band = _gpu(rwr, ctx, suzanne, rwr.make_spheres(), cam_inv, w, h, params, instances=inst, rows=(24, 56))
            _check(got, want, f"schedule {scene} {what}")
            assert got["stats"][1] == want["rays"], what
            _same(got, again, what)
            _same(got, third, what)
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


@pytest.mark.parametrize("s,K", [(1, 4), (3, 3), (16, 2)])
def test_accumulation(rwr, gpu_ctx, suzanne, s, K):
    w, h = 120, 64
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0.3, 0.2, 2.6), aspect=w / h))
    gpu_ctx.upload_model(suzanne); gpu_ctx.set_instances(None); gpu_ctx.set_spheres(rwr.make_spheres()); gpu_ctx.resize(w, h)
    flags = _flags(rwr, 3)
    gpu_ctx.render(cam_inv, rwr.make_params(spp=K * s, max_bounces=3, seed=11, flags=flags))
    want = gpu_ctx.readback(aux=True)
    for k in range(1, K + 1):
        gpu_ctx.render(cam_inv, rwr.make_params(spp=s, max_bounces=3, seed=11, flags=flags | rwr.FLAG_ACCUMULATE))
        assert gpu_ctx.accum_samples() == k * s
    _same(gpu_ctx.readback(aux=True), want, (s, K))
    # another depth is another image: the accumulation starts over
    gpu_ctx.render(cam_inv, rwr.make_params(spp=2, max_bounces=2, seed=11, flags=flags | rwr.FLAG_ACCUMULATE))
    assert gpu_ctx.accum_samples() == 2
    gpu_ctx.render(cam_inv, rwr.make_params(spp=3, max_bounces=3, seed=11, flags=flags | rwr.FLAG_ACCUMULATE))
    assert gpu_ctx.accum_samples() == 3
    gpu_ctx.accum_reset()


@pytest.mark.parametrize("strips", [True, False], ids=["strips", "bands"])
def test_multi_gpu_layouts_assemble_the_frame(rwr, suzanne, strips):
    w, h = 203, 67
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0.3, 0.2, 2.6), aspect=w / h))
    params = rwr.make_params(spp=3, max_bounces=3, seed=2, flags=_flags(rwr, 3))
    with rwr.Context(0) as ctx:
        ctx.upload_model(suzanne)
        ctx.set_spheres(rwr.make_spheres())
        ctx.resize(w, h)
        ctx.render(cam_inv, params)
        full = ctx.readback(aux=True)
        bounce_full = ctx.last_render_stats()[1]
        for n in (2, 3):
            asm = {k: np.zeros_like(full[k]) for k in PLANES}
            total = 0
            for r in range(n):
                if strips:
                    ctx.render(cam_inv, params, strips=(r, n))
                    rows = [y for y in range(h) if (y // 8) % n == r]
                else:
                    band = rwr.dist_band(r, n, h)
                    ctx.render(cam_inv, params, rows=band)
                    rows = list(range(*band))
                total += ctx.last_render_stats()[1]
                part = ctx.readback(aux=True)
                for k in PLANES:
                    asm[k][rows] = part[k][rows]
                ctx.dist_loopback_deposit(r, n, strips)
            ctx.dist_loopback_finish(n, strips)
            _same(asm, full, (strips, n))
            assert total == bounce_full
            assert np.array_equal(ctx.dist_readback(), full["color"]), (strips, n)


def test_full_size_on_selected_rows(rwr, orc, pref, gpu_ctx, suzanne):
    w, h, spp, bounces = 1920, 1080, 8, 4
    scene = (suzanne, rwr.make_spheres(), None, (0, 0, 0), (0, 0, -1), 0, w, h)
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(aspect=w / h))
    got = _gpu(rwr, gpu_ctx, suzanne, rwr.make_spheres(), cam_inv, w, h,
               rwr.make_params(spp=spp, max_bounces=bounces, seed=1, flags=_flags(rwr, bounces)))
    for rows in ((0, 2), (539, 541), (1078, 1080)):
        want = _reference(pref, orc, rwr, scene, cam_inv, spp, bounces, 1, rows=rows)
        _check(got, want, f"1080p rows {rows}", rows=rows)
    assert (got["obj_id"] >= 0).mean() > 0.05


def test_cli_bounces(rwr, gpu_ctx, suzanne, tmp_path):
    """rwr_render --bounces 3 --spp 4 (the flag is set by the program) writes the library's frame."""
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")
    w, h = 96, 64
    out = str(tmp_path / "b3.png")
    r = subprocess.run([exe, "--res", rwr.RES_DIR, "--size", f"{w}x{h}", "--keys", "-*1", "--frames", "1", "--spp", "4", "--bounces", "3",
                        "--out", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = rwr.decode_image_rgba8(open(out, "rb").read()).astype(int)[::-1]          # PNG row 0 = top = framebuffer row h-1

    def lib_frame(bounces):
        cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(aspect=w / h))
        frame = _gpu(rwr, gpu_ctx, suzanne, rwr.make_spheres(), cam_inv, w, h,
                     rwr.make_params(spp=4, max_bounces=bounces, seed=0, flags=_flags(rwr, bounces)))
        lin = frame["color"].astype(float) / 255
        enc = np.where(lin <= 0.0031308, 12.92 * lin, 1.055 * np.power(lin, 1 / 2.4) - 0.055)
        enc[..., 3] = lin[..., 3]
        return np.rint(enc * 255)

    d = np.abs(got - lib_frame(3))
    assert d.max() <= 3 and (d > 0).mean() < 0.01      # (+-1 LSB in linear RGBA8 can move the sRGB byte by up to 3 near black)
    assert (np.abs(got - lib_frame(1)) > 0).sum() > (d > 0).sum()   # and it is not the one-bounce frame
