"""The a-trous denoiser (RWR_FLAG_DENOISE) on the GPU against the tests' CPU reference (denoise_ref.c):
  * parity: the frame without the flag (AUX), filtered by the reference, against the frame with the flag - colour within 1e-4,
    rgba8 within 1 code, depth / id / t bit-identical; sizes that are no multiple of a tile, smaller than the filter's reach,
    1 / 3 / 5 iterations (the LDS-staged steps alone, and with the far steps), another sigma;
  * frames in flight, a frame without the flag after one with it, accumulation, refusals and parameters, the program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref
import shadow_common as sc

pytestmark = pytest.mark.gpu
COLOR_TOL = 1e-4   # the project's bar (tests/test_gpu_multi_bounce.py)
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")


@pytest.fixture(scope="module")
def dref(tmp_path_factory):
    return denoise_ref.lib(tmp_path_factory)


@pytest.fixture()
def ctx(rwr, gpu_ctx):
    """The shared context with the filter's defaults, one frame in flight, no instances - before and after."""
    def clean():
        gpu_ctx.set_frames_in_flight(1)
        gpu_ctx.set_denoise_params()
        gpu_ctx.set_instances(None)
        gpu_ctx.set_triangles(rwr.make_triangles())
        gpu_ctx.accum_reset()
    clean()
    yield gpu_ctx
    clean()


def _upload(ctx, s, w, h):
    model, spheres, inst = s[0], s[1], s[2]
    if isinstance(model, (list, tuple)):
        ctx.upload_parts(model)
    else:
        ctx.upload_model(model)
    ctx.set_instances(inst)
    ctx.set_spheres(spheres)
    ctx.resize(w, h)


def _flags(rwr, bounces, shadows=False):
    return (rwr.FLAG_MULTI_BOUNCE if bounces > 1 else 0) | (rwr.FLAG_SHADOWS if shadows else 0)


def _frame(rwr, ctx, cam_inv, spp, bounces, flags, seed=9):
    ctx.render(cam_inv.view(rwr.CAMERA_INV_DTYPE), rwr.make_params(spp=spp, max_bounces=bounces, seed=seed, flags=flags))
    return ctx.readback(aux=True)


def _same(a, b, what=""):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _parity(rwr, orc, dref, ctx, s, w, h, spp, bounces, shadows=False, **params):
    """plain: the frame without the flag; want: the reference's filter of it; got: the frame with the flag."""
    cam_inv = sc.camera(rwr, orc, s, w, h)
    _upload(ctx, s, w, h)
    ctx.set_denoise_params()
    if params:
        ctx.set_denoise_params(**params)
    base = _flags(rwr, bounces, shadows)
    plain = _frame(rwr, ctx, cam_inv, spp, bounces, base | rwr.FLAG_AUX_OUTPUTS)
    nhat = denoise_ref.face_normals(dref, orc, s[0], s[2])
    want = denoise_ref.denoise(dref, plain["color_f32"], plain["obj_id"], plain["hit_t"], nhat, **{**denoise_ref.DEFAULTS, **params})
    got = _frame(rwr, ctx, cam_inv, spp, bounces, base | rwr.FLAG_DENOISE)   # AUX implied
    what = (w, h, spp, bounces, params)
    for k in ("depth", "obj_id", "hit_t"):
        assert got[k].tobytes() == plain[k].tobytes(), (what, k)
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    moved = float(np.abs(want["color_f32"] - plain["color_f32"]).max())
    print(f"denoise parity {what}: colour error {err:.3g}; the filter moves a pixel by up to {moved:.3g}")
    assert err <= COLOR_TOL, (what, err)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, what
    assert got["color_f32"][..., 3].tobytes() == plain["color_f32"][..., 3].tobytes(), what
    return plain, got, moved


def test_cube_one_sample(rwr, orc, dref, ctx, suzanne, cube):
    s = sc.scene("cube", rwr, orc, suzanne, cube)
    _, _, moved = _parity(rwr, orc, dref, ctx, s, 96, 64, 1, 1)
    assert moved > 1e-3   # the filter did something


def test_suzanne_and_spheres_with_shadows(rwr, orc, dref, ctx, suzanne, cube):
    s = sc.scene("suzanne_side", rwr, orc, suzanne, cube)   # from the side: the two spheres stand clear of the mesh
    plain, _, moved = _parity(rwr, orc, dref, ctx, s, 128, 72, 4, 2, shadows=True)
    ids = plain["obj_id"]
    assert (ids >= 0).any() and (ids == -2).any() and (ids == -3).any() and (ids == -1).any()   # mesh, both spheres, background
    assert moved > 1e-3


def test_instance_grid(rwr, orc, dref, ctx, suzanne, cube):
    grid2 = rwr.make_instance_grid(2, 3.0).view(orc.INSTANCE_DTYPE)
    s = (suzanne, orc.make_spheres(), grid2, (6.5, -1.0, 2.0), (1.5, -1.5, 0), 0)
    plain, _, _ = _parity(rwr, orc, dref, ctx, s, 160, 96, 2, 1)
    assert plain["obj_id"].max() >= len(suzanne["faces"])   # faces of a later instance are seen: their normals are the instance's


@pytest.mark.parametrize("size", [(67, 37), (5, 3)])
def test_odd_and_tiny_frames(rwr, orc, dref, ctx, suzanne, cube, size):
    """67 x 37: no multiple of any tile, narrower than the reach of step 16 (2 x 16 x 2 + 1 = 65 wide taps fit, 37 rows do not);
    5 x 3: smaller than every step's reach."""
    s = sc.scene("cube", rwr, orc, suzanne, cube)
    _parity(rwr, orc, dref, ctx, s, size[0], size[1], 2, 1)


@pytest.mark.parametrize("params", [{"iterations": 1}, {"iterations": 3}, {"iterations": 5}, {"sigma_color": 0.5}, {"iterations": 2, "sigma_color": 0.11},
                                    {"normal_cos_min": -1.0, "depth_rel": 1e9}, {"normal_cos_min": 0.9999, "depth_rel": 0.0}])
def test_parameters(rwr, orc, dref, ctx, suzanne, cube, params):
    """1, 3 and 5 iterations (the last launch is an LDS-staged one, a far one), other tolerances: every face one surface, and
    next to none."""
    s = sc.scene("suzanne_side", rwr, orc, suzanne, cube)
    _parity(rwr, orc, dref, ctx, s, 120, 67, 2, 1, **params)
    assert ctx.denoise_params()["iterations"] == params.get("iterations", 5)


def test_frames_in_flight_give_the_same_bytes(rwr, orc, ctx, suzanne, cube):
    s = sc.scene("suzanne_side", rwr, orc, suzanne, cube)
    w, h = 130, 70
    cam_inv = sc.camera(rwr, orc, s, w, h)
    _upload(ctx, s, w, h)
    frames = []
    for fif in (1, 2, 3):
        ctx.set_frames_in_flight(fif)
        for k in range(fif + 1):   # every slot, and the first one again
            frames.append(_frame(rwr, ctx, cam_inv, 3, 1, rwr.FLAG_DENOISE))
    for f in frames[1:]:
        _same(f, frames[0], "frames in flight")


def test_flag_off_after_flag_on(rwr, orc, ctx, suzanne, cube):
    """A frame without the flag that follows a denoised one is a fresh context's frame, byte for byte (with and without AUX)."""
    s = sc.scene("cube", rwr, orc, suzanne, cube)
    w, h = 96, 64
    cam_inv = sc.camera(rwr, orc, s, w, h)
    for spp, bounces, flags in ((1, 0, 0), (1, 0, rwr.FLAG_AUX_OUTPUTS), (3, 1, rwr.FLAG_AUX_OUTPUTS)):
        with rwr.Context(0) as fresh:
            _upload(fresh, s, w, h)
            fresh.render(cam_inv.view(rwr.CAMERA_INV_DTYPE), rwr.make_params(spp=spp, max_bounces=bounces, seed=9, flags=flags))
            want = fresh.readback(aux=bool(flags))
        _upload(ctx, s, w, h)
        _frame(rwr, ctx, cam_inv, spp, bounces, flags | rwr.FLAG_DENOISE)
        ctx.render(cam_inv.view(rwr.CAMERA_INV_DTYPE), rwr.make_params(spp=spp, max_bounces=bounces, seed=9, flags=flags))
        got = ctx.readback(aux=bool(flags))
        for k in want:
            assert got[k].tobytes() == want[k].tobytes(), (spp, bounces, flags, k)
        if not flags:
            with pytest.raises(rwr.RwrError):   # the plain frame has no aux planes, whatever the frame before had
                ctx.readback(aux=True)


def test_accumulation(rwr, orc, ctx, suzanne, cube):
    s = sc.scene("suzanne_side", rwr, orc, suzanne, cube)
    w, h = 120, 64
    cam_inv = sc.camera(rwr, orc, s, w, h)
    cam = cam_inv.view(rwr.CAMERA_INV_DTYPE)
    _upload(ctx, s, w, h)
    for fif in (1, 2):
        ctx.set_frames_in_flight(fif)
        want = _frame(rwr, ctx, cam_inv, 8, 1, rwr.FLAG_DENOISE)
        ctx.accum_reset()
        for k in range(1, 5):
            ctx.render(cam, rwr.make_params(spp=2, max_bounces=1, seed=9, flags=rwr.FLAG_DENOISE | rwr.FLAG_ACCUMULATE))
            assert ctx.accum_samples() == 2 * k
        _same(ctx.readback(aux=True), want, ("K = 4 frames of 2 spp", fif))
        ctx.accum_reset()
    ctx.set_frames_in_flight(1)
    # the flag comes on at frame 3 of an AUX accumulation, the parameters change at frame 4: the accumulation goes on, and the
    # frames shown are the filter (with the parameters of the moment) over the accumulated image
    acc = rwr.FLAG_AUX_OUTPUTS | rwr.FLAG_ACCUMULATE
    for k, flags in enumerate((acc, acc, acc | rwr.FLAG_DENOISE, acc | rwr.FLAG_DENOISE, acc), 1):
        if k == 4:
            ctx.set_denoise_params(iterations=2, sigma_color=0.2)
        ctx.render(cam, rwr.make_params(spp=2, max_bounces=1, seed=9, flags=flags))
        assert ctx.accum_samples() == 2 * k, k
        got = ctx.readback(aux=True)
        if k == 3:
            _same(got, _one_frame(rwr, ctx, s, cam, 6, rwr.FLAG_DENOISE), "frame 3")
        if k == 4:
            _same(got, _one_frame(rwr, ctx, s, cam, 8, rwr.FLAG_DENOISE), "frame 4")
        if k == 5:   # the history never saw the filter
            _same(got, _one_frame(rwr, ctx, s, cam, 10, rwr.FLAG_AUX_OUTPUTS), "frame 5")


def _one_frame(rwr, ctx, s, cam, spp, flags):
    """ONE frame of spp samples in a context of its own (the accumulation under test goes on untouched), same parameters."""
    with rwr.Context(0) as other:
        _upload(other, s, ctx.width, ctx.height)
        other.set_denoise_params(**ctx.denoise_params())
        other.render(cam, rwr.make_params(spp=spp, max_bounces=1, seed=9, flags=flags))
        return other.readback(aux=True)


def test_refusals_and_parameters(rwr, orc, ctx, suzanne, cube):
    s = sc.scene("suzanne_side", rwr, orc, suzanne, cube)
    w, h = 96, 64
    cam = sc.camera(rwr, orc, s, w, h).view(rwr.CAMERA_INV_DTYPE)
    _upload(ctx, s, w, h)
    ctx.set_denoise_params(iterations=3, sigma_color=0.25, normal_cos_min=0.5, depth_rel=0.125)
    kept = {"iterations": 3, "sigma_color": 0.25, "normal_cos_min": 0.5, "depth_rel": 0.125}
    assert ctx.denoise_params() == kept
    dn = rwr.FLAG_DENOISE

    def refused(code, **kw):
        with pytest.raises(rwr.RwrError) as ei:
            ctx.render(cam, **kw)
        assert ei.value.code == code, kw
        assert ctx.denoise_params() == kept

    # parts of a frame
    refused(rwr.ERR_UNSUPPORTED, params=rwr.make_params(flags=dn), rows=(0, 32))
    refused(rwr.ERR_UNSUPPORTED, params=rwr.make_params(flags=dn), rows=(8, h))
    refused(rwr.ERR_UNSUPPORTED, params=rwr.make_params(flags=dn), strips=(0, 2))
    refused(rwr.ERR_UNSUPPORTED, params=rwr.make_params(flags=dn), strips=(1, 2))
    # the reference frame's own forms
    refused(rwr.ERR_UNSUPPORTED, params=rwr.make_params(flags=dn | rwr.FLAG_ORTHO_RAYS))
    refused(rwr.ERR_UNSUPPORTED, params=rwr.make_params(flags=dn | rwr.FLAG_USE_BVH))
    refused(rwr.ERR_UNSUPPORTED, params=rwr.make_params(spp=2, max_bounces=1, flags=dn | rwr.FLAG_USE_BVH))
    ctx.set_triangles(rwr.make_triangles([((0, 0, -1), (1, 0, -1), (0, 1, -1))]))
    try:
        refused(rwr.ERR_UNSUPPORTED, params=rwr.make_params(flags=dn))
    finally:
        ctx.set_triangles(rwr.make_triangles())
    # a call that covers the whole frame behaves as rwr_render
    whole = _frame_of(ctx, cam, rwr.make_params(spp=2, max_bounces=1, seed=4, flags=dn))
    for kw in ({"rows": (0, h)}, {"strips": (0, 1)}):
        ctx.render(cam, rwr.make_params(spp=2, max_bounces=1, seed=4, flags=dn), **kw)
        _same(ctx.readback(aux=True), whole, kw)
    # parameters out of range or NaN: refused, the previous ones stay
    nan, inf = float("nan"), float("inf")
    for bad in ({"iterations": 0}, {"iterations": 6}, {"sigma_color": 0.0}, {"sigma_color": -1.0}, {"sigma_color": nan}, {"sigma_color": inf},
                {"sigma_color": 1e-30}, {"normal_cos_min": nan}, {"depth_rel": -0.5}, {"depth_rel": nan}):
        with pytest.raises(rwr.RwrError) as ei:
            ctx.set_denoise_params(**bad)
        assert ei.value.code == rwr.ERR_INVALID_ARGUMENT, bad
        assert ctx.denoise_params() == kept, bad
    L = rwr.lib()
    p = np.zeros(1, rwr.DENOISE_PARAMS_DTYPE)
    assert L.rwr_denoise_set_params(None, p.ctypes.data_as(C.c_void_p)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_denoise_get_params(None, p.ctypes.data_as(C.c_void_p)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_denoise_get_params(ctx._h, None) == rwr.ERR_INVALID_ARGUMENT
    assert ctx.denoise_params() == kept
    # the context is still usable, and NULL restores the defaults
    _same(_frame_of(ctx, cam, rwr.make_params(spp=2, max_bounces=1, seed=4, flags=dn)), whole, "after the refusals")
    ctx.set_denoise_params()
    assert ctx.denoise_params() == pytest.approx(denoise_ref.DEFAULTS)


def _frame_of(ctx, cam, params):
    ctx.render(cam, params)
    return ctx.readback(aux=True)


def test_cli_denoise(rwr, ctx, suzanne, tmp_path):
    """rwr_render --denoise writes the PNG of the library's own frame with the flag, not the one without it."""
    exe = os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render")
    w, h = 96, 64
    common = [exe, "--res", rwr.RES_DIR, "--size", f"{w}x{h}", "--keys", "-*1", "--frames", "1", "--spp", "2", "--bounces", "1"]
    outs = {}
    for name, extra in (("plain", []), ("denoise", ["--denoise"]), ("tuned", ["--denoise", "--denoise-iterations", "2", "--denoise-sigma", "0.3"])):
        outs[name] = str(tmp_path / f"{name}.png")
        r = subprocess.run(common + extra + ["--out", outs[name]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(aspect=w / h))
    ctx.upload_model(suzanne); ctx.set_spheres(rwr.make_spheres()); ctx.resize(w, h)

    def driver_png(flags, name, **params):
        ctx.set_denoise_params()
        if params:
            ctx.set_denoise_params(**params)
        ctx.render(cam_inv, rwr.make_params(spp=2, max_bounces=1, seed=0, flags=flags))
        path = str(tmp_path / name)
        rwr.write_png(path, ctx.readback()["color"], flip_vertical=True, encode_srgb=True)
        return open(path, "rb").read()

    read = lambda k: open(outs[k], "rb").read()   # noqa: E731
    assert read("plain") == driver_png(0, "d0.png")
    assert read("denoise") == driver_png(rwr.FLAG_DENOISE, "d1.png")
    assert read("tuned") == driver_png(rwr.FLAG_DENOISE, "d2.png", iterations=2, sigma_color=0.3)
    assert read("denoise") != read("plain") and read("tuned") != read("denoise")
    r = subprocess.run(common + ["--denoise-iterations", "9"], capture_output=True, text=True)
    assert r.returncode != 0
    assert "--denoise" in subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
