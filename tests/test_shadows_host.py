"""Shadow rays (RWR_FLAG_SHADOWS), host side: the tests' CPU reference (shadow_ref.c) against path_ref.c with the
switch off, the definition's consequences with it on, a hand-derived known answer, the coverage condition of the parity scenes,
and the public constants.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import path_ref
import shadow_common as sc
import shadow_ref
from test_multi_bounce_host import _scene as mb_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return shadow_ref.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return path_ref.lib(tmp_path_factory)


@pytest.mark.parametrize("name", ["suzanne", "cube", "grid", "two_parts", "cube_nmap"])
def test_switch_off_is_the_path_reference(sref, pref, rwr, orc, suzanne, cube, name):
    model, spheres, inst, eye, target, flags = mb_scene(name, rwr, orc, suzanne, cube)
    w, h = 48, 32
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=eye, target=target, aspect=w / h)).view(orc.CAMERA_INV_DTYPE)
    for bounces in (0, 1, 3):
        for spp in (1, 3):
            params = orc.make_params(spp, bounces, seed=7, flags=flags)
            got = shadow_ref.render_path(sref, orc, cam_inv, orc.make_screen(w, h), params, spheres, model, instances=inst, shadows=False)
            want = path_ref.render_path(pref, orc, cam_inv, orc.make_screen(w, h), params, spheres, model, instances=inst)
            for k in PLANES:
                assert got[k].tobytes() == want[k].tobytes(), (name, bounces, spp, k)
            assert got["rays"] == want["rays"]
            assert got["shadow_rays"] == 0 and got["occluded"] == 0


@pytest.mark.parametrize("name", list(sc.SCENES))
def test_coverage_condition(sref, rwr, orc, suzanne, cube, name):
    """At the tests' size every parity scene is in its class: mixed scenes have a tenth of their shadow rays on either side."""
    s = sc.scene(name, rwr, orc, suzanne, cube)
    ref = sc.reference(shadow_ref, sref, orc, s, sc.camera(rwr, orc, s), sc.W, sc.H, 1, 0)
    print(f"{name}: {ref['occluded']} of {ref['shadow_rays']} shadow rays occluded")
    sc.check_class(name, ref)


@pytest.mark.parametrize("name", sc.MIXED + ["suzanne_front", "two_parts_front"])
def test_switch_on(sref, rwr, orc, suzanne, cube, name):
    s = sc.scene(name, rwr, orc, suzanne, cube)
    cam_inv = sc.camera(rwr, orc, s)
    for bounces, spp in ((0, 1), (1, 3), (3, 2)):
        on = sc.reference(shadow_ref, sref, orc, s, cam_inv, sc.W, sc.H, spp, bounces)
        off = sc.reference(shadow_ref, sref, orc, s, cam_inv, sc.W, sc.H, spp, bounces, shadows=False)
        what = (name, bounces, spp)
        for k in ("depth", "obj_id", "hit_t"):
            assert on[k].tobytes() == off[k].tobytes(), what + (k,)
        assert on["color_f32"][..., 3].tobytes() == off["color_f32"][..., 3].tobytes(), what
        # spp 1 without a bounce: the unshadowed frame is the reference frame, whose E(h0) is not clamped; the assets' E stay below 16
        assert (on["color_f32"] <= off["color_f32"]).all(), what
        if name == "cube_back":
            # a convex body alone: its occluded hits are those whose face looks away from the light, where E is the ambient
            # part already (no Lambert term, no highlight), and no bounce ray meets it again - shadows change no pixel
            assert on["color_f32"].tobytes() == off["color_f32"].tobytes(), what
        elif sc.SCENES[name] == "mixed":
            assert (on["color_f32"][..., :3] < off["color_f32"][..., :3]).any(), what
        assert on["rays"] == off["rays"], what
        # every hit shaded casts one: primary hits (alpha / 2 per sample) + bounce hits = the rays a frame one bounce deeper
        # traces beyond the primary ones (every hit emits the next ray; the path prefix property)
        deeper = sc.reference(shadow_ref, sref, orc, s, cam_inv, sc.W, sc.H, spp, bounces + 1, shadows=False)
        primary_hits = int(round(float(off["color_f32"][..., 3].sum()) / 2.0 * spp))
        assert on["shadow_rays"] == deeper["rays"], what
        assert on["shadow_rays"] >= primary_hits and (bounces or on["shadow_rays"] == primary_hits), what
        if sc.SCENES[name] == "mixed":
            assert 0 < on["occluded"] < on["shadow_rays"], what
    # wherever the primary hit's ray got through, the pixel is the unshadowed one; where it did not, the colour is the ambient part
    on = sc.reference(shadow_ref, sref, orc, s, cam_inv, sc.W, sc.H, 1, 0)
    plain = sc.reference(shadow_ref, sref, orc, s, cam_inv, sc.W, sc.H, 1, 0, shadows=False)
    dark = on["occluded0"] != 0
    assert int(dark.sum()) == on["occluded"], name
    assert not dark[on["obj_id"] == -1].any()
    through = ~dark
    assert np.array_equal(on["color_f32"][through], plain["color_f32"][through]), name   # (the assets' E(h0) stay below the cap of 16)
    amb_only = sc.reference(shadow_ref, sref, orc, s, cam_inv, sc.W, sc.H, 1, 0, shadows=2)
    assert np.array_equal(on["color_f32"][dark], amb_only["color_f32"][dark]), name
    if sc.SCENES[name] == "lit":
        assert through[on["obj_id"] != -1].mean() > 0.95, name


@pytest.mark.parametrize("name", ["closed_room", "inside_suzanne"])
def test_everything_occluded(sref, rwr, orc, suzanne, cube, name):
    s = sc.scene(name, rwr, orc, suzanne, cube)
    cam_inv = sc.camera(rwr, orc, s)
    w, h = 32, 24
    for bounces, spp in ((0, 1), (0, 3), (2, 2), (4, 1)):
        if bounces and name != "closed_room":
            continue   # (suzanne is not watertight: a deep path may find its way out; its primary hits are all in the dark)
        on = sc.reference(shadow_ref, sref, orc, s, cam_inv, w, h, spp, bounces)
        assert on["shadow_rays"] > 0 and on["occluded"] == on["shadow_rays"], (name, bounces, spp)
        if name == "closed_room":
            assert (on["obj_id"] >= 0).all()
            assert on["shadow_rays"] == w * h * spp * (1 + bounces)
            amb = np.asarray(s[0]["material"]["ambient"], np.float32).reshape(3)
            rgb = on["color_f32"][..., :3]
            if bounces == 0:   # the ambient-only path sum is the ambient term itself
                want = sum([amb] * spp, np.zeros(3, np.float32)) / np.float32(spp)
                assert np.array_equal(rgb, np.broadcast_to(want.astype(np.float32), rgb.shape))
            # ... and at any depth the sum ambient * (1 + T1 + T1 T2 + ...) of the same path with E = ambient at every hit, which the
            # reference forms without asking the visibility routine (shadows=2): byte for byte, every plane
            forced = sc.reference(shadow_ref, sref, orc, s, cam_inv, w, h, spp, bounces, shadows=2)
            for k in PLANES:
                assert on[k].tobytes() == forced[k].tobytes(), (bounces, spp, k)
            assert (on["shadow_rays"], on["occluded"], on["rays"]) == (forced["shadow_rays"], forced["occluded"], forced["rays"])
            if bounces:        # every throughput is an albedo product in [0, 1]: more than the ambient term, at most 1 + B of them
                assert (rgb >= amb * np.float32(0.999)).all() and (rgb <= amb * np.float32(1 + bounces) * np.float32(1.001)).all()
                assert (rgb > amb * np.float32(1.01)).any()


def _point_in_triangle(p, tri):
    """Signed distances of the 2-D point(s) p to the three edges (positive inside), for a counter-clockwise triangle."""
    a, b, c = (np.asarray(v, np.float64)[:2] for v in tri)
    def edge(u, v):
        n = np.array([-(v - u)[1], (v - u)[0]]) / np.linalg.norm(v - u)
        return (p - u) @ n
    return np.minimum(np.minimum(edge(a, b), edge(b, c)), edge(c, a))


def test_known_answer_one_triangle_and_a_blocker(sref, rwr, orc, ref_loader, suzanne):
    """A large triangle in the plane z = 0 that faces the mesh light -(1, -1, -5) / sqrt(27), seen from above and aside: nothing in front of
    it - no shadow ray is occluded and the frame is the unshadowed one.  With a second triangle in the plane z = 1 the shadow on
    the floor is that triangle moved by -(1 - 1e-4) * L.xy / L.z = (+0.19998, -0.19998): a floor point (x, y) is dark exactly when
    (x - 0.19998, y + 0.19998) lies in the blocker; the blocker's own top is lit."""
    w, h = 96, 64
    s_open = (sc.triangle_model(ref_loader, [sc.FLOOR], suzanne["texture"]), np.zeros(0, orc.SPHERE_DTYPE), None, (3.0, -3.0, 6.0), (0, 0, 0), 0)
    cam_inv = sc.camera(rwr, orc, s_open, w, h)
    on = sc.reference(shadow_ref, sref, orc, s_open, cam_inv, w, h, 1, 0)
    off = sc.reference(shadow_ref, sref, orc, s_open, cam_inv, w, h, 1, 0, shadows=False)
    assert on["shadow_rays"] == int((on["obj_id"] == 0).sum()) > 1000 and on["occluded"] == 0
    assert on["color_f32"].tobytes() == off["color_f32"].tobytes()

    s_block = (sc.triangle_model(ref_loader, [sc.FLOOR, sc.BLOCKER], suzanne["texture"]),) + s_open[1:]
    on = sc.reference(shadow_ref, sref, orc, s_block, cam_inv, w, h, 1, 0)
    off = sc.reference(shadow_ref, sref, orc, s_block, cam_inv, w, h, 1, 0, shadows=False)
    amb = np.asarray(s_block[0]["material"]["ambient"], np.float32).reshape(3)
    shift = (1.0 - 1e-4) / 5.0
    n_dark = n_lit = 0
    for y in range(h):
        for x in range(w):
            oid = int(on["obj_id"][y, x])
            if oid == 1:     # the blocker's top: nothing above it
                assert np.array_equal(on["color_f32"][y, x], off["color_f32"][y, x])
                continue
            if oid != 0:
                continue
            o, d, _ = orc.pixel_to_ray(cam_inv, orc.make_screen(w, h), x, y)
            p = o.astype(np.float64) + float(on["hit_t"][y, x]) * d.astype(np.float64)
            inside = _point_in_triangle(np.array([p[0] - shift, p[1] + shift]), sc.BLOCKER)
            if abs(inside) < 1e-3:
                continue     # on the shadow's edge: rounding decides
            if inside > 0:
                assert np.array_equal(on["color_f32"][y, x, :3], amb), (x, y)
                n_dark += 1
            else:
                assert np.array_equal(on["color_f32"][y, x], off["color_f32"][y, x]), (x, y)
                n_lit += 1
    assert n_dark > 20 and n_lit > 1000
    assert abs(on["occluded"] - n_dark) <= 40   # the pixels left out on the edge


def test_header_driver_and_library_agree(rwr):
    text = open(os.path.join(ROOT, "include", "rwr_hip.h")).read()
    m = re.search(r"RWR_FLAG_SHADOWS\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and int(m.group(1)) == 7
    assert rwr.FLAG_SHADOWS == 1 << 7
    bits = [int(v) for v in re.findall(r"RWR_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", text)]
    assert bits.count(7) == 1 and len(set(bits)) == len(bits)
    assert re.search(r"RWR_API\s+int\s+rwr_last_shadow_stats\s*\(\s*rwr_context\s*\*\s*\w*,\s*uint64_t\s*\*\s*\w*,\s*uint64_t\s*\*\s*\w*\)", text)
    lib = C.CDLL(rwr.LIB_PATH)
    assert hasattr(lib, "rwr_last_shadow_stats")
    assert hasattr(rwr.Context, "last_shadow_stats")
