"""Scenes far from the world origin against the CPU oracle, in every frame path (tests/world_offset_common.py).

The exact hit test rounds at world magnitude, so far from the origin its literal hits stray outside their faces by up to
several pixels; the conservative culling (csrc/rwr_cull.h, the whole-mesh rectangle, the bins, the tile lists, the
wavefront integrator's tiles) must keep every face such a hit needs.  Each case proves it reached the hazard: the float64
audit of the oracle's own frame finds pixels whose stray exceeds half a pixel where the case says so.

Bars (tests/test_gpu_primary.py): obj_id, hit_t and depth bit-exact, colour within 1e-4, RGBA8 within 1 LSB; a plain
frame's RGBA8 equals the AUX frame's byte for byte and its depth equals the oracle's."""
import numpy as np
import pytest

import fuzz_common
import path_ref
import world_offset_common as W

pytestmark = pytest.mark.gpu

COLOR_TOL = 1e-4

# (mesh, offset, view, w, h, fovy, expect strays > 0.5 px)  -- the strays as tests/test_world_offset_margin.py measures them
CASES = [
    ("suzanne", "0", "fill", 1920, 1080, 60.0, False),
    ("suzanne", "3e4", "fill", 1920, 1080, 60.0, True),
    ("suzanne", "1e5", "fill", 480, 270, 8.0, True),
    ("suzanne", "1e5", "grazing", 1920, 1080, 60.0, True),
    ("suzanne", "1e4", "small", 333, 187, 8.0, False),
    ("suzanne", "1e5", "small", 3840, 2160, 60.0, False),
    ("soup256", "1e4", "fill", 480, 270, 8.0, True),
    ("soup256", "1e5", "fill", 1920, 1080, 60.0, True),
    ("soup256", "3e4", "grazing", 333, 187, 8.0, False),
    ("soup257", "3e4", "fill", 480, 270, 8.0, True),
    ("soup257", "1e5", "grazing", 480, 270, 8.0, True),
    ("soup257", "0", "small", 333, 187, 60.0, False),
    ("cube", "1e5", "fill", 1920, 1080, 60.0, True),
    ("cube", "3e4", "grazing", 480, 270, 8.0, True),
    ("cube", "1e5", "small", 480, 270, 8.0, True),
    ("heightfield", "1e5", "grazing", 480, 270, 8.0, True),
    ("heightfield", "0", "fill", 333, 187, 60.0, False),
]


def _id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-{c[3]}x{c[4]}-f{c[5]:.0f}"


@pytest.fixture(scope="module")
def meshes(ref_loader, res_dir):
    return W.meshes(ref_loader, res_dir)


def _contexts(rwr, settings):
    """{name: context} with the given environment knobs (read when a context is created)."""
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for name, env in settings.items():
            for k, v in env.items():
                mp.setenv(k, v)
            out[name] = rwr.Context(0)
            mp.undo()
    finally:
        mp.undo()
    return out


@pytest.fixture(scope="module")
def ctxs(rwr):
    out = _contexts(rwr, {"lists": {}, "nolists": {"RWR_TILE_LISTS": "0"}})
    yield out
    for c in out.values():
        c.close()


def _scene(rwr, meshes, case):
    name, off, view, w, h, fovy, _ = case
    model, center, radius = meshes[name]
    offset = W.OFFSETS[off]
    eye, target = W.views(center, radius)[view]
    return W.translated(model, offset), W.spheres_at(rwr, offset), W.camera(rwr, eye, target, offset, w, h, fovy)


def _load(rwr, ctx, model, spheres, w, h):
    ctx.upload_model(model)
    ctx.set_instances(None)
    ctx.set_spheres(spheres)
    ctx.resize(w, h)


def _aux(rwr, ctx, cam, flags=0, **kw):
    ctx.render(cam, rwr.make_params(flags=rwr.FLAG_AUX_OUTPUTS | flags), **kw)
    return ctx.readback(aux=True)


def _plain(rwr, ctx, cam, **kw):
    ctx.render(cam, rwr.make_params(), **kw)
    r = ctx.readback()
    return r["color"].copy(), r["depth"].copy()


def _parity(got, want, what, rows=slice(None)):
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(np.ascontiguousarray(got[k][rows]).view(np.uint32), np.ascontiguousarray(want[k][rows]).view(np.uint32)), \
            (what, k, int((got[k][rows] != want[k][rows]).sum()))
    err = float(np.abs(got["color_f32"][rows] - want["color_f32"][rows]).max()) if got["color_f32"][rows].size else 0.0
    assert err <= COLOR_TOL, (what, err)
    assert (np.abs(got["color"][rows].astype(int) - want["color"][rows].astype(int)) <= 1).all(), what


def _oracle(orc, cam, w, h, spheres, model):
    return orc.render_frame(cam.view(orc.CAMERA_INV_DTYPE), orc.make_screen(w, h), spheres.view(orc.SPHERE_DTYPE), model)


def _strip_rows(h, r, n):
    return [y for s in range(r, (h + 7) // 8, n) for y in range(8 * s, min(h, 8 * s + 8))]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_far_scene_matches_the_oracle_in_every_form(rwr, orc, meshes, ctxs, case):
    name, off, view, w, h, fovy, expect = case
    model, spheres, cam = _scene(rwr, meshes, case)
    want = _oracle(orc, cam, w, h, spheres, model)
    a = W.audit(cam, w, h, fovy, model, want)
    assert a["pixels"] >= 20, a["pixels"]                          # not a vacuous case
    if expect:
        assert (a["stray_px"] > 0.5).sum() > 0, float(a["stray_px"].max())   # the hazard is reached
    for c in ctxs.values():
        _load(rwr, c, model, spheres, w, h)
    on, off_ = ctxs["lists"], ctxs["nolists"]
    got = _aux(rwr, on, cam)
    _parity(got, want, "default")
    color, depth = _plain(rwr, on, cam)
    assert np.array_equal(color, got["color"]), "plain RGBA8"
    assert np.array_equal(depth.view(np.uint32), want["depth"].view(np.uint32)), "plain depth"
    _parity(_aux(rwr, off_, cam), want, "tile lists off")
    for flag, what in ((rwr.FLAG_ONE_PIXEL_PER_LANE, "one pixel"), (rwr.FLAG_NO_CULL, "no cull"), (rwr.FLAG_USE_BVH, "bvh")):
        _parity(_aux(rwr, on, cam, flag), want, what)
    band = (h // 4, (3 * h) // 4 + 1)
    _parity(_aux(rwr, on, cam, rows=band), want, "band", slice(*band))
    rows = _strip_rows(h, 1, 3)
    _parity(_aux(rwr, on, cam, strips=(1, 3)), want, "strips", rows)
    _parity(_aux(rwr, off_, cam, strips=(1, 3)), want, "strips, lists off", rows)


def test_spheres_far_from_the_origin(rwr, orc, meshes, ctxs):
    """The sphere rectangles far from the origin: both spheres in view (the mesh behind the camera)."""
    w, h = 640, 360
    model, center, radius = meshes["suzanne"]
    for off in ("0", "3e4", "1e5"):
        offset = W.OFFSETS[off]
        m, sph = W.translated(model, offset), W.spheres_at(rwr, offset)
        cam = W.camera(rwr, (0.3, 0.4, -1.6), (0.5, 0.45, -3.5), offset, w, h)
        want = _oracle(orc, cam, w, h, sph, m)
        assert (want["obj_id"] < -1).sum() >= 1000
        for c in ctxs.values():
            _load(rwr, c, m, sph, w, h)
            _parity(_aux(rwr, c, cam), want, ("spheres", off))


PLAIN_CASES = [c for c in CASES if c[0] in ("suzanne", "cube") and c[3] <= 1920]


@pytest.fixture(scope="module")
def launch_ctxs(rwr):
    out = _contexts(rwr, {"two": {"RWR_FUSED_SETUP": "0"}, "fused": {"RWR_FUSED_SETUP": "1"}, "graph": {"RWR_FRAME_GRAPH": "1"}})
    yield out
    for c in out.values():
        c.close()


@pytest.mark.parametrize("case", PLAIN_CASES, ids=_id)
def test_plain_frames_in_every_launch_form(rwr, orc, meshes, launch_ctxs, case):
    """Two launches with one frame in flight, the fused form with 2 and 3 frames in flight and several frames queued before
    the readback, the frame graph (moving, then replayed): RGBA8 = the AUX frame's, depth = the oracle's."""
    name, off, view, w, h, fovy, _ = case
    model, spheres, cam = _scene(rwr, meshes, case)
    want = _oracle(orc, cam, w, h, spheres, model)
    _, center, radius = meshes[name]
    others = [W.camera(rwr, e, t, W.OFFSETS[off], w, h, fovy) for v, (e, t) in W.views(center, radius).items() if v != view]
    ref = launch_ctxs["two"]
    _load(rwr, ref, model, spheres, w, h)
    aux = _aux(rwr, ref, cam)
    _parity(aux, want, "aux")

    def check(frame, what):
        assert np.array_equal(frame[0], aux["color"]), (what, "rgba8")
        assert np.array_equal(frame[1].view(np.uint32), want["depth"].view(np.uint32)), (what, "depth")

    check(_plain(rwr, ref, cam), "two launches")
    for form, fifs in (("fused", (2, 3)), ("graph", (1, 2))):
        c = launch_ctxs[form]
        _load(rwr, c, model, spheres, w, h)
        try:
            for fif in fifs:
                c.set_frames_in_flight(fif)
                for cams in (others + [cam], [cam, cam, cam]):     # moving, then standing still (a graph replays)
                    for k in cams:
                        c.render(k, rwr.make_params())
                    r = c.readback()
                    check((r["color"], r["depth"]), (form, fif))
        finally:
            c.synchronize()
            c.set_frames_in_flight(1)


KNOBS = {"bin64": {"RWR_BIN_MIN_FACES": "64"}, "bin1024": {"RWR_BIN_MIN_FACES": "1024"},
         "wave0": {"RWR_WAVE_CULL_MIN": "0"}, "wavebig": {"RWR_WAVE_CULL_MIN": "1000000000"}}


@pytest.fixture(scope="module")
def knob_ctxs(rwr):
    out = _contexts(rwr, KNOBS)
    yield out
    for c in out.values():
        c.close()


@pytest.mark.parametrize("name", ["suzanne", "soup257", "cube"])
@pytest.mark.parametrize("off", ["0", "1e5"])
def test_binning_and_wave_cull_knobs(rwr, orc, meshes, knob_ctxs, name, off):
    """RWR_BIN_MIN_FACES=64 bins suzanne; =1024 leaves the 257- and 428-face scenes unbinned above the tile-list limit (several
    256-face LDS rounds); RWR_WAVE_CULL_MIN at 0 and very large: every setting gives the oracle's frame."""
    view = "fill" if off == "0" else "grazing"
    w, h, fovy = (480, 270, 8.0) if off == "1e5" else (640, 360, 60.0)
    case = (name, off, view, w, h, fovy, False)
    model, spheres, cam = _scene(rwr, meshes, case)
    want = _oracle(orc, cam, w, h, spheres, model)
    assert (want["obj_id"] >= 0).sum() >= 50
    for k, c in knob_ctxs.items():
        _load(rwr, c, model, spheres, w, h)
        _parity(_aux(rwr, c, cam), want, k)
        color, depth = _plain(rwr, c, cam)
        assert np.array_equal(depth.view(np.uint32), want["depth"].view(np.uint32)), (k, "plain depth")


@pytest.mark.parametrize("case", [c for c in CASES if c[1] in ("3e4", "1e5") and c[0] != "heightfield"][:6], ids=_id)
def test_wavefront_reference_frame(rwr, orc, meshes, gpu_ctx, case):
    """The wavefront integrator at spp = 1, b = 0 gives the reference frame (its primary culling and live-tile list)."""
    name, off, view, w, h, fovy, _ = case
    model, spheres, cam = _scene(rwr, meshes, case)
    want = _oracle(orc, cam, w, h, spheres, model)
    _load(rwr, gpu_ctx, model, spheres, w, h)
    gpu_ctx.render(cam, rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_AUX_OUTPUTS))
    _parity(gpu_ctx.readback(aux=True), want, "wavefront spp 1")


def test_wavefront_one_bounce_on_selected_rows(rwr, orc, meshes, gpu_ctx):
    """spp = 4, b = 1 at 1920x1080 and 1e5 from the origin: the oracle's path renderer on selected rows."""
    case = ("suzanne", "1e5", "grazing", 1920, 1080, 60.0, True)
    model, spheres, cam = _scene(rwr, meshes, case)
    w, h = 1920, 1080
    _load(rwr, gpu_ctx, model, spheres, w, h)
    gpu_ctx.render(cam, rwr.make_params(spp=4, max_bounces=1, seed=7, flags=rwr.FLAG_AUX_OUTPUTS))
    got = gpu_ctx.readback(aux=True)
    assert (got["obj_id"] >= 0).sum() >= 10000
    for r0, r1 in ((0, 4), (500, 508), (1076, 1080)):
        want = orc.render_path(cam.view(orc.CAMERA_INV_DTYPE), orc.make_screen(w, h), orc.make_params(4, 1, seed=7),
                               spheres.view(orc.SPHERE_DTYPE), model, rows=(r0, r1))
        _parity(got, want, ("rows", r0), slice(r0, r1))


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return path_ref.lib(tmp_path_factory)


def test_multi_bounce_far_from_the_origin(rwr, orc, pref, meshes, gpu_ctx):
    case = ("suzanne", "3e4", "grazing", 160, 90, 60.0, False)
    model, spheres, cam = _scene(rwr, meshes, case)
    w, h = 160, 90
    _load(rwr, gpu_ctx, model, spheres, w, h)
    gpu_ctx.render(cam, rwr.make_params(spp=2, max_bounces=3, seed=11, flags=rwr.FLAG_AUX_OUTPUTS | rwr.FLAG_MULTI_BOUNCE))
    got = gpu_ctx.readback(aux=True)
    want = path_ref.render_path(pref, orc, cam.view(orc.CAMERA_INV_DTYPE), orc.make_screen(w, h), orc.make_params(2, 3, seed=11),
                                spheres.view(orc.SPHERE_DTYPE), model)
    assert (want["obj_id"] >= 0).sum() >= 50
    _parity(got, want, "multi-bounce")


def test_fuzz_far_from_the_origin(rwr, orc, ref_loader):
    """A bounded slice of the randomised parity run with a world offset of up to 1e5 per frame and the plain-frame check."""
    with rwr.Context(0) as ctx:
        n, n_path, _, worst = fuzz_common.run(rwr, orc, ref_loader, ctx, seed=31337, seconds=30.0, far=True, plain=True)
    assert n >= 20 and worst <= COLOR_TOL, (n, n_path, worst)
