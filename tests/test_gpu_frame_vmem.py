"""The frame kernel (k_primary_p2) reads its culling records once per workgroup through LDS and its diffuse texture as
one quad record per pixel decoded through an LDS table: every plane must stay byte-identical to the one-pixel-per-lane
kernel (k_primary), which keeps the per-wave culling and the four-tap float4 texture."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")


def _frame(rwr, ctx, cam_inv, w, h, flags=0, rows=None, strips=None):
    ctx.resize(w, h)
    ctx.render(cam_inv, rwr.make_params(flags=rwr.FLAG_AUX_OUTPUTS | flags), rows=rows, strips=strips)
    return ctx.readback(aux=True)


def _agree(rwr, ctx, cam_inv, w, h, **kw):
    a = _frame(rwr, ctx, cam_inv, w, h, **kw)
    b = _frame(rwr, ctx, cam_inv, w, h, flags=rwr.FLAG_ONE_PIXEL_PER_LANE, **kw)
    for k in PLANES:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (w, h, k)
    return a


def _cam(rwr, w, h, **kw):
    return rwr.camera_build_inv_uniform(rwr.make_camera(aspect=w / h, **kw))


def test_models_at_bench_cameras(rwr, gpu_ctx, suzanne, cube):
    for model, (w, h) in [(suzanne, (1920, 1080)), (cube, (256, 256)), (suzanne, (333, 187))]:
        gpu_ctx.upload_model(model); gpu_ctx.set_instances(None); gpu_ctx.set_spheres(rwr.make_spheres())
        for kw in (dict(), dict(eye=(0, 0, 3), target=(0, 0, -1)), dict(eye=(2.2, 1.7, 3.1), target=(0, 0, 0))):
            out = _agree(rwr, gpu_ctx, _cam(rwr, w, h, **kw), w, h)
            assert (out["obj_id"] >= 0).any()


def _retextured(model, tex, uv_scale):
    m = dict(model)
    v = model["vertices"].copy()
    v["tex_coords"] = (v["tex_coords"] - 0.5) * uv_scale + 0.5   # outside [0, 1]: the clamp edges
    m["vertices"], m["texture"] = v, tex
    return m


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (7, 13), (64, 3)])
def test_texture_sizes_and_clamp_edges(rwr, gpu_ctx, suzanne, shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    tex = rng.integers(0, 256, size=shape + (4,), dtype=np.uint8)
    gpu_ctx.upload_model(_retextured(suzanne, tex, 3.0)); gpu_ctx.set_instances(None); gpu_ctx.set_spheres(rwr.make_spheres())
    w, h = 320, 200
    _agree(rwr, gpu_ctx, _cam(rwr, w, h, eye=(0, 0, 3), target=(0, 0, -1)), w, h)


def test_two_materials(rwr, gpu_ctx, suzanne, cube):
    rng = np.random.default_rng(5)
    parts = [_retextured(suzanne, rng.integers(0, 256, size=(5, 11, 4), dtype=np.uint8), 1.5), dict(cube)]
    v = parts[1]["vertices"].copy()
    v["position"] = v["position"] * 0.5 + np.array([1.2, 0.0, 0.0], np.float32)
    parts[1]["vertices"] = v
    gpu_ctx.upload_parts(parts); gpu_ctx.set_instances(None); gpu_ctx.set_spheres(rwr.make_spheres())
    w, h = 400, 240
    out = _agree(rwr, gpu_ctx, _cam(rwr, w, h, eye=(0.5, 0.5, 4), target=(0.5, 0, 0)), w, h)
    assert (out["obj_id"] >= 0).any()


def _heightfield(ref_loader, n, tex):
    g = np.linspace(-1.0, 1.0, n + 1, dtype=np.float64)
    x, y = np.meshgrid(g, g)
    z = -4.0 + 0.25 * np.sin(5.0 * x) * np.cos(4.0 * y) + 0.6 * x
    verts = np.zeros((n + 1) * (n + 1), ref_loader.VERTEX_DTYPE)
    verts["position"] = np.stack([2.2 * x, 1.3 * y, z], -1).reshape(-1, 3).astype(np.float32)
    verts["tex_coords"] = np.stack([(x + 1) / 2, (y + 1) / 2], -1).reshape(-1, 2).astype(np.float32)
    i = np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]
    a, b, c, d = i, i + 1, i + n + 1, i + n + 2
    faces = np.zeros(2 * n * n, ref_loader.FACE_DTYPE)
    faces["indices"] = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([b, d, c], -1).reshape(-1, 3)]).astype(np.uint32)
    mat = np.zeros(1, ref_loader.MATERIAL_DTYPE)
    mat["ambient"], mat["diffuse"], mat["specular"] = 0.05, 0.8, 0.3
    return {"vertices": verts, "faces": faces, "material": mat, "texture": tex}


def test_binned_scene_with_bands_and_strips(rwr, gpu_ctx, ref_loader, suzanne):
    """More than 256 faces: screen-bin lists, several 256-entry rounds per workgroup where faces are dense."""
    gpu_ctx.upload_model(_heightfield(ref_loader, 60, suzanne["texture"])); gpu_ctx.set_instances(None)
    gpu_ctx.set_spheres(rwr.make_spheres())
    w, h = 640, 360
    cam = _cam(rwr, w, h)
    full = _agree(rwr, gpu_ctx, cam, w, h)
    assert (full["obj_id"] >= 0).any()
    _agree(rwr, gpu_ctx, cam, w, h, rows=(40, 200))
    _agree(rwr, gpu_ctx, cam, w, h, strips=(1, 3))


def test_fused_setup_frames_in_flight_moving_camera(rwr, suzanne):
    saved = os.environ.get("RWR_FUSED_SETUP")
    os.environ["RWR_FUSED_SETUP"] = "1"
    try:
        w, h = 480, 270
        with rwr.Context(0) as ctx:
            ctx.upload_model(suzanne); ctx.set_spheres(rwr.make_spheres()); ctx.resize(w, h)
            cams = [_cam(rwr, w, h, eye=(0.3 * np.sin(k), 0.1 * k, 3.0), target=(0, 0, -1)) for k in range(4)]
            for fif in (2, 3):
                ctx.set_frames_in_flight(fif)
                for cam in cams:   # (rwr_render without AUX: the fused launch is the plain frame's)
                    ctx.render(cam, rwr.make_params())
                    a = ctx.readback()
                    ctx.render(cam, rwr.make_params(flags=rwr.FLAG_ONE_PIXEL_PER_LANE))
                    b = ctx.readback()
                    for k in a:
                        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), (fif, k)
            ctx.set_frames_in_flight(1)
    finally:
        if saved is None:
            os.environ.pop("RWR_FUSED_SETUP", None)
        else:
            os.environ["RWR_FUSED_SETUP"] = saved
