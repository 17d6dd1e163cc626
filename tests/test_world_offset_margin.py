"""The culling margins against the literal hits of the oracle far from the world origin (CPU only; the GPU side is
tests/test_gpu_world_offset.py).  For every pixel the oracle shows a face at, tests/world_offset_common.audit measures in
float64 how far the pixel's centre ray passes outside that face, and the margin that each conservative test grants it:
the edge functions and the face rectangle of csrc/rwr_cull.h make_frame_tri (with the half-pixel guard between tile
bounds and pixel centres) and the whole-mesh rectangle of frame_consts.cpp.  Every stray must be covered (ratio <= 1), and the
margins without the world-magnitude term must NOT cover the far scenes: that is the hazard the term exists for."""
import numpy as np
import pytest

import world_offset_common as W

SIZES = [(480, 270, 60.0), (1920, 1080, 60.0), (480, 270, 8.0)]


@pytest.fixture(scope="module")
def meshes(ref_loader, res_dir):
    return W.meshes(ref_loader, res_dir)


@pytest.mark.parametrize("name", ["suzanne", "soup256", "soup257", "cube", "heightfield"])
@pytest.mark.parametrize("off", list(W.OFFSETS))
def test_every_stray_is_covered_by_the_margins(rwr, orc, meshes, name, off):
    model, center, radius = meshes[name]
    offset = W.OFFSETS[off]
    m, spheres = W.translated(model, offset), W.spheres_at(rwr, offset)
    worst_old = 0.0
    for view, (eye, target) in W.views(center, radius).items():
        for w, h, fovy in SIZES:
            if w > 480 and (name in ("cube", "heightfield") or view != "fill"):
                continue   # (oracle time)
            cam = W.camera(rwr, eye, target, offset, w, h, fovy)
            frame = orc.render_frame(cam.view(orc.CAMERA_INV_DTYPE), orc.make_screen(w, h), spheres.view(orc.SPHERE_DTYPE), m)
            a = W.audit(cam, w, h, fovy, m, frame)
            tag = (view, w, h, fovy)
            assert a["pixels"] >= 20, tag
            assert a["edge"] <= 1.0 and a["rect"] <= 1.0 and a["mesh"] <= 1.0, tag + (a["edge"], a["rect"], a["mesh"])
            if off == "0":
                assert a["unbounded"] == 0.0, tag   # at the origin the world bound never switches culling off
                assert a["stray_px"].max() <= 0.01, tag
            old = W.audit(cam, w, h, fovy, m, frame, world_term=False)
            worst_old = max(worst_old, old["edge"], old["rect"])
    if off == "1e5" or (off == "3e4" and name in ("suzanne", "soup256", "soup257")):
        assert worst_old > 1.0, worst_old   # without the world term some literal hit lies outside every margin
    elif off in ("0", "1e3"):
        assert worst_old <= 0.25, worst_old


def test_the_world_term_is_negligible_at_the_bench_cameras(rwr, meshes):
    """At the headline cameras (|O| <= 3, |p| <= 1.5) the world term adds about a tenth to the (0.02 px) edge margins of
    a typical face and a few hundredths of a pixel to the rectangles."""
    model = meshes["suzanne"][0]
    p = model["vertices"]["position"].astype(np.float64)[model["faces"]["indices"].astype(np.int64)]
    for eye in ((0, 0, 0), (0, 0, 3)):
        cam = rwr.camera_build_inv_uniform(rwr.make_camera(eye=eye, target=(0, 0, -1), aspect=1920 / 1080))
        cc = W.cull_consts(cam, 1920, 1080)
        rho, _ = W.face_rho(cc, p)
        visible = np.isfinite(rho)
        assert visible.mean() >= 0.97, eye
        assert float(rho[visible].max()) / W.KCULL_REL <= 0.2 or eye == (0, 0, 0), (eye, float(rho[visible].max()))
        assert float(np.median(rho[visible])) / W.KCULL_REL <= 0.15, eye
        assert 2.0 * float(np.median(rho[visible])) * max(cc["gx"], cc["gy"]) <= 0.1, eye
