"""Per-tile face sets (RWR_TILE_LISTS, default on): for unbinned scenes k_frame_setup's last blocks make every 32x4 tile's set of
faces that survive its culling, and the two-pixel frame kernel walks that set instead of culling the face records itself.  The
frames must be byte-identical with the sets (RWR_TILE_LISTS=1), without them (=0: the kernel's own culling) and with the
one-pixel-per-lane kernel, and the sets must hold exactly the faces the kernel's own culling keeps (its debug counts)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")


@pytest.fixture(scope="module")
def ctxs(rwr):
    """{knob value: context}; the knob is read when a context is created."""
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for v in ("1", "0"):
            mp.setenv("RWR_TILE_LISTS", v)
            out[v] = rwr.Context(0)
    finally:
        mp.undo()
    yield out
    for c in out.values():
        c.close()


def _setup(rwr, ctx, model, w, h, normal_map=None):
    ctx.upload_model(model)
    ctx.set_instances(None)
    ctx.set_spheres(rwr.make_spheres())
    if normal_map is not None:
        ctx.set_normal_map(0, normal_map)
    ctx.resize(w, h)


def _cam(rwr, eye, w, h, target=(0, 0, -1)):
    return rwr.camera_build_inv_uniform(rwr.make_camera(eye=eye, target=target, aspect=w / h))


def _aux(rwr, ctx, cam, flags=0, **kw):
    ctx.render(cam, rwr.make_params(flags=rwr.FLAG_AUX_OUTPUTS | flags), **kw)
    return ctx.readback(aux=True)


def _plain(rwr, ctx, cam, flags=0, **kw):
    ctx.render(cam, rwr.make_params(flags=flags), **kw)
    r = ctx.readback()
    return {"color": r["color"], "depth": r["depth"]}


def _same(a, b, what, rows=None):
    for k in a:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (what, k)


def _all_forms_agree(rwr, ctxs, cam, flags=0):
    """Every plane of an AUX frame and the colour / depth of a plain one: lists on = lists off = one pixel per lane; the
    debug counts (faces kept by the culling, faces tested) with lists on = off.  Returns the debug planes."""
    on, off = ctxs["1"], ctxs["0"]
    a = _aux(rwr, on, cam, flags)
    _same(a, _aux(rwr, off, cam, flags), "aux off")
    _same(a, _aux(rwr, on, cam, flags | rwr.FLAG_ONE_PIXEL_PER_LANE), "aux one pixel")
    p = _plain(rwr, on, cam, flags)
    _same(p, _plain(rwr, off, cam, flags), "plain off")
    _same(p, _plain(rwr, on, cam, flags | rwr.FLAG_ONE_PIXEL_PER_LANE), "plain one pixel")
    if flags & rwr.FLAG_NO_CULL:
        return a
    d = _aux(rwr, on, cam, flags | rwr.FLAG_DEBUG_COUNTS)
    _same(d, _aux(rwr, off, cam, flags | rwr.FLAG_DEBUG_COUNTS), "debug counts")
    return a, d


@pytest.mark.parametrize("eye", [(0, 0, 0), (0, 0, 3)], ids=["cfg2", "cfg2b"])
def test_bench_views_are_the_same_with_and_without_tile_lists(rwr, ctxs, suzanne, eye):
    w, h = 1920, 1080
    for c in ctxs.values():
        _setup(rwr, c, suzanne, w, h)
    a, d = _all_forms_agree(rwr, ctxs, _cam(rwr, eye, w, h))
    assert (a["obj_id"] >= 0).any()
    assert d["obj_id"].max() >= 1


def test_whole_mesh_in_a_few_tiles(rwr, ctxs, suzanne):
    """Suzanne far away: some tiles keep far more faces than a short per-tile list of face indices would hold."""
    w, h = 640, 360
    for c in ctxs.values():
        _setup(rwr, c, suzanne, w, h)
    a, d = _all_forms_agree(rwr, ctxs, _cam(rwr, (0.0, 0.0, 60.0), w, h, target=(0, 0, 0)))
    assert (a["obj_id"] >= 0).any()
    assert d["obj_id"].max() > 31
    assert int((d["obj_id"] > 0).sum()) <= 8 * 128   # ... within a few tiles


def test_camera_sweep_across_the_spheres(rwr, ctxs, suzanne):
    w, h = 480, 270
    for c in ctxs.values():
        _setup(rwr, c, suzanne, w, h)
    sphere_px = 0
    for k in range(12):
        a = 2.0 * np.pi * k / 12
        eye = (0.5 + 1.6 * np.cos(a), 0.45 + 0.9 * np.sin(a), 1.5 + 0.5 * np.sin(2 * a))
        out, _ = _all_forms_agree(rwr, ctxs, _cam(rwr, eye, w, h, target=(0.5, 0.45, -3.5)))
        sphere_px += int((out["obj_id"] < -1).sum())
    assert sphere_px > 0


def test_no_cull_and_normal_map(rwr, ctxs, suzanne, cube):
    w, h = 400, 232
    for c in ctxs.values():
        _setup(rwr, c, suzanne, w, h, normal_map=cube["normal_map"])
    cam = _cam(rwr, (0.3, 0.2, 2.6), w, h, target=(0, 0, 0))
    _all_forms_agree(rwr, ctxs, cam, rwr.FLAG_NO_CULL)
    a, _ = _all_forms_agree(rwr, ctxs, cam, rwr.FLAG_NORMAL_MAP)
    assert (a["obj_id"] >= 0).any()
    for c in ctxs.values():
        c.set_normal_map(0, None)


def test_strips_and_bands(rwr, ctxs, suzanne):
    w, h = 328, 181
    for c in ctxs.values():
        _setup(rwr, c, suzanne, w, h)
    cam = _cam(rwr, (0.2, 0.1, 2.4), w, h, target=(0, 0, 0))
    for flags in (0, rwr.FLAG_AUX_OUTPUTS):
        full = _plain(rwr, ctxs["0"], cam, flags)
        for r in range(3):   # every third 8-row strip (row pitch 24)
            rows = [y for s in range(r, (h + 7) // 8, 3) for y in range(8 * s, min(h, 8 * s + 8))]
            got = {v: _plain(rwr, c, cam, flags, strips=(r, 3)) for v, c in ctxs.items()}
            _same(got["1"], got["0"], ("strips", r, flags), rows)
            _same(got["1"], full, ("strips vs whole", r, flags), rows)
        for b in ((0, 64), (40, 133), (96, 181)):
            got = {v: _plain(rwr, c, cam, flags, rows=b) for v, c in ctxs.items()}
            _same(got["1"], got["0"], ("band", b, flags), slice(*b))
            _same(got["1"], full, ("band vs whole", b, flags), slice(*b))


@pytest.mark.parametrize("fif", [1, 2, 3])
def test_frames_in_flight_with_a_moving_camera(rwr, ctxs, suzanne, fif):
    w, h = 1280, 720   # (large enough for two launches per frame with frames in flight: the fused form ignores the sets)
    for c in ctxs.values():
        _setup(rwr, c, suzanne, w, h)
        c.set_frames_in_flight(fif)
    try:
        cams = [_cam(rwr, (0.08 * k, 0.03 * k, 2.8 - 0.2 * k), w, h, target=(0, 0, -1)) for k in range(6)]
        for k, cam in enumerate(cams):
            _same(_plain(rwr, ctxs["1"], cam), _plain(rwr, ctxs["0"], cam), ("frame", fif, k))
        frames = {}
        for v, c in ctxs.items():   # several frames queued before any is read back
            for cam in cams:
                c.render(cam, rwr.make_params())
            frames[v] = c.readback()
        _same({"color": frames["1"]["color"], "depth": frames["1"]["depth"]},
              {"color": frames["0"]["color"], "depth": frames["0"]["depth"]}, ("queued", fif))
    finally:
        for c in ctxs.values():
            c.synchronize()
            c.set_frames_in_flight(1)
