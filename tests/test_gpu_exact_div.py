"""The frame kernel's hit test computes its plane distance t = tnum / ndotd (compute.wgsl:99-102) by a short exact form
(rwr_device_p2.h hit_t) when the wave's operands lie in its domain, and by the IEEE division otherwise.  The library checks
the form against the division on the GPU itself; whole frames must stay byte-identical to the one-pixel-per-lane kernel
(k_primary), which divides as the shader does, including views that move the spheres across the screen."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")


def test_short_division_matches_the_ieee_quotient_bit_for_bit(gpu_ctx):
    n, bad, n_sel, bad_sel = gpu_ctx.selftest_exact_div(count=1 << 30, seed=11)
    assert n >= 1 << 30          # two quotients per lane and round, most in the domain
    assert bad == 0
    assert n_sel > n             # the hit test's own choice, edges and out-of-domain waves included
    assert bad_sel == 0


def _frame(rwr, ctx, cam_inv, w, h, flags=0):
    ctx.render(cam_inv, rwr.make_params(flags=rwr.FLAG_AUX_OUTPUTS | flags))
    return ctx.readback(aux=True)


def _agree(rwr, ctx, cam_inv, w, h):
    ctx.resize(w, h)
    a = _frame(rwr, ctx, cam_inv, w, h)
    b = _frame(rwr, ctx, cam_inv, w, h, flags=rwr.FLAG_ONE_PIXEL_PER_LANE)
    for k in PLANES:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (w, h, k)
    return a


@pytest.mark.parametrize("name,model,w,h,eye", [
    ("cfg1", "cube", 256, 256, (0, 0, 0)),
    ("cfg2", "suzanne", 1920, 1080, (0, 0, 0)),
    ("cfg2b", "suzanne", 1920, 1080, (0, 0, 3)),
])
def test_bench_configs_match_one_pixel_per_lane(rwr, gpu_ctx, suzanne, cube, name, model, w, h, eye):
    gpu_ctx.upload_model(suzanne if model == "suzanne" else cube); gpu_ctx.set_instances(None)
    gpu_ctx.set_spheres(rwr.make_spheres())
    cam = rwr.camera_build_inv_uniform(rwr.make_camera(eye=eye, target=(0, 0, -1), aspect=w / h))
    out = _agree(rwr, gpu_ctx, cam, w, h)
    assert (out["obj_id"] >= 0).any()


def test_camera_sweep_across_the_spheres_matches_one_pixel_per_lane(rwr, gpu_ctx, suzanne):
    gpu_ctx.upload_model(suzanne); gpu_ctx.set_instances(None); gpu_ctx.set_spheres(rwr.make_spheres())
    w, h = 480, 270
    sphere_px = 0
    for k in range(12):
        a = 2.0 * np.pi * k / 12
        eye = (0.5 + 1.6 * np.cos(a), 0.45 + 0.9 * np.sin(a), 1.5 + 0.5 * np.sin(2 * a))
        cam = rwr.camera_build_inv_uniform(rwr.make_camera(eye=eye, target=(0.5, 0.45, -3.5), aspect=w / h))
        out = _agree(rwr, gpu_ctx, cam, w, h)
        sphere_px += int((out["obj_id"] < -1).sum())
    assert sphere_px > 0


def test_fresh_context_with_an_empty_mesh_renders_the_spheres(rwr, orc, suzanne):
    """A context whose only mesh has no faces has no shading records at all: the frame kernel must not touch them (every
    frame path: AUX, the plain frame, and the one-launch form with frames in flight)."""
    w, h = 128, 96
    empty = dict(suzanne, faces=suzanne["faces"][:0])
    cam = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(3, 0.45, -3.5), target=(0.5, 0.45, -3.5), aspect=w / h))
    want = orc.render_frame(cam.view(orc.CAMERA_INV_DTYPE), orc.make_screen(w, h), orc.make_spheres(), empty)
    with rwr.Context(0) as ctx:
        ctx.upload_model(empty); ctx.set_spheres(rwr.make_spheres()); ctx.resize(w, h)
        ctx.render(cam, rwr.make_params(flags=rwr.FLAG_AUX_OUTPUTS))
        got = ctx.readback(aux=True)
        assert np.array_equal(got["obj_id"], want["obj_id"])
        assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32))
        assert (got["obj_id"] == -2).any() and (got["obj_id"] == -3).any()
        for fif in (1, 2):
            ctx.set_frames_in_flight(fif)
            for _ in range(3):
                ctx.render(cam, rwr.make_params())
            plain = ctx.readback()
            assert np.array_equal(np.asarray(plain["color"]).view(np.uint8), got["color"].view(np.uint8)), fif
        ctx.set_frames_in_flight(1)
