"""Tile classes (RWR_TILE_CLASS, default on): with the per-tile face sets k_frame_setup leaves one class word per 32x4 tile — no face
/ exactly one (and which) / more, whether the tile lies in the mesh's pixel rectangle, and which spheres' rectangles it touches —
and the two-pixel frame kernel takes one of three ways through a tile by it: clear values for a tile nothing can show in, a
straight path for a tile with one face and no sphere, the whole kernel for the rest.  Every sequence here is rendered in two fresh
contexts that differ in RWR_TILE_CLASS alone (=0: the kernel ignores the words), given the same calls: every plane of every frame
must be the same bytes in both — no tolerance, both sides run the same functions.  The class words themselves are read back
(rwr_debug_tile_classes) and compared with a model built from the *other* context's debug counts and object ids.

The contexts run with RWR_FUSED_SETUP=0, so that these small frames take the two launches per frame a 1080p frame takes, and
RWR_AUTO_BVH_FACE_PX=0, so that cube.obj's small faces stay in the (binned) two-pixel kernel."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# an odd width (a lane's second pixel off the frame), widths / heights that are no multiples of 64 / 8, one and several workgroups
SIZES = [(1, 1), (2, 1), (63, 7), (65, 9), (129, 17), (130, 16), (256, 64)]
CAMS = {
    "R": dict(eye=(0, 0, 0), target=(0, 0, -1)),          # the reference camera, inside the mesh: no tile without a face
    "A": dict(eye=(0, 0, 3), target=(0, 0, -1)),          # suzanne from outside: most tiles show nothing
    "B": dict(eye=(0.4, 0.2, 2.6), target=(0, 0, 0)),
}
PLAIN_ENV = dict(RWR_FUSED_SETUP="0", RWR_AUTO_BVH_FACE_PX="0")
FACES, SPHERES = 0x3, 0xff0000


@contextlib.contextmanager
def _pair(rwr, size, n_slots=1, setup=None, env=PLAIN_ENV):
    """(classes on, classes off): two fresh contexts that differ in RWR_TILE_CLASS alone (the knobs are read at creation);
    setup(ctx) uploads the scene."""
    mp = pytest.MonkeyPatch()
    ctxs = []
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        for v in ("1", "0"):
            mp.setenv("RWR_TILE_CLASS", v)
            ctxs.append(rwr.Context(0))
        mp.undo()
        for c in ctxs:
            setup(c)
            c.resize(*size)
            c.set_frames_in_flight(n_slots)
        yield ctxs
    finally:
        mp.undo()
        for c in ctxs:
            c.close()


def _suzanne_scene(rwr, suzanne, spheres=None):
    def setup(c):
        c.upload_model(suzanne)
        c.set_spheres(rwr.make_spheres() if spheres is None else rwr.make_spheres(spheres))
    return setup


def _cam(rwr, size, eye, target):
    return rwr.camera_build_inv_uniform(rwr.make_camera(eye=eye, target=target, aspect=size[0] / size[1]))


def _frame(rwr, on, off, cam_inv, flags=0, rows=None, strips=None, what=None):
    """One frame in both contexts; all planes byte-identical.  Returns the planes of the context with classes."""
    params = rwr.make_params(flags=flags)
    aux = bool(flags & rwr.FLAG_AUX_OUTPUTS)
    got = []
    for c in (on, off):
        c.render(cam_inv, params, rows=rows, strips=strips)
        got.append(c.readback(aux=aux))
    assert set(got[0]) == ({"color", "depth", "obj_id", "hit_t", "color_f32"} if aux else {"color", "depth"})
    for k in got[0]:
        assert np.array_equal(got[0][k].view(np.uint8), got[1][k].view(np.uint8)), (what, flags, rows, strips, k)
    return got[0]


def _differ(a, b):
    return not np.array_equal(a["color"], b["color"])


@pytest.mark.parametrize("n_slots", [1, 2, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_sizes_cameras_and_slots(rwr, suzanne, size, n_slots):
    """Three cameras, the plain form and the two with aux planes, 2 n + 1 frames each: the first n compute their rays (a camera
    the slots have not seen), the others load them from the slots' planes — both forms of the kernel, as rwr_ray_plane_stats
    confirms."""
    aux, dbg = rwr.FLAG_AUX_OUTPUTS, rwr.FLAG_AUX_OUTPUTS | rwr.FLAG_DEBUG_COUNTS
    with _pair(rwr, size, n_slots, _suzanne_scene(rwr, suzanne)) as (on, off):
        builds = served = 0
        for flags in (0, aux, dbg):
            for cam in "RAB":
                cam_inv = _cam(rwr, size, **CAMS[cam])
                for i in range(2 * n_slots + 1):
                    _frame(rwr, on, off, cam_inv, flags, what=(cam, i))
                builds, served = builds + n_slots, served + n_slots + 1   # ... so n_slots frames computed, n_slots + 1 loaded
                assert on.ray_plane_stats() == off.ray_plane_stats() == (builds, served), (flags, cam)


def test_camera_sweep_across_the_spheres(rwr, suzanne):
    """The reference's two spheres in view from twelve poses around them (the mesh is small there: tiles with no face or several,
    with and without a sphere bit), then from the reference camera inside the mesh (tiles with one face), first with the
    reference's spheres and then with eight spheres around the rim of the view, whose rectangles lie over one-face tiles.  Four
    frames per pose on one slot: one computes, three load."""
    size = (320, 180)
    aux = rwr.FLAG_AUX_OUTPUTS
    seen = set()
    sphere_px = 0
    with _pair(rwr, size, 1, _suzanne_scene(rwr, suzanne)) as (on, off):
        poses = []
        for k in range(12):
            a = 2.0 * np.pi * k / 12
            poses.append(((0.5 + 1.6 * np.cos(a), 0.45 + 0.9 * np.sin(a), 1.5 + 0.5 * np.sin(2 * a)), (0.5, 0.45, -3.5)))
        poses.append((CAMS["R"]["eye"], CAMS["R"]["target"]))
        for k, (eye, target) in enumerate(poses):
            cam_inv = _cam(rwr, size, eye, target)
            for flags in (0, aux, aux | rwr.FLAG_DEBUG_COUNTS, aux):
                out = _frame(rwr, on, off, cam_inv, flags, what=k)
            sphere_px += int((out["obj_id"] < -1).sum())
            cls = on.tile_classes()
            assert np.array_equal(cls, off.tile_classes())   # (the setup writes the words whether the kernel looks or not)
            seen |= {(int(c & FACES), bool(c & SPHERES)) for c in np.unique(cls)}
        assert sphere_px > 0
        assert {(0, False), (1, False), (2, False), (0, True), (2, True)} <= seen, seen
        # eight spheres around the rim of the reference camera's view, where the near faces fill whole tiles: their rectangles
        # lie over tiles with one face
        rim = [((x, y, -4.0), 1.2) for x, y in ((-2.5, 1.3), (2.5, 1.3), (-2.5, -1.3), (2.5, -1.3), (-2.8, 0.0), (2.8, 0.0), (0.0, 1.5), (0.0, -1.5))]
        for c in (on, off):
            c.set_spheres(rwr.make_spheres(rim))
        for flags in (0, aux, aux | rwr.FLAG_DEBUG_COUNTS, aux):
            _frame(rwr, on, off, cam_inv, flags, what="large sphere")
        cls = on.tile_classes()
        assert (((cls & FACES) == 1) & ((cls & SPHERES) != 0)).any()


def test_spheres_change_while_the_camera_rests(rwr, suzanne):
    """Other spheres, none, and the first ones again at a camera that never moves: the frames follow, and every change is one new
    k_frame_setup launch (the class words are made from the spheres' rectangles and their count), with none in between."""
    size = (256, 64)
    first = [((0.5, 0.3, 1.5), 0.3), ((0.4, 0.4, -3.0), 0.4)]
    other = [((-0.6, -0.2, 1.0), 0.25)]
    with _pair(rwr, size, 1, _suzanne_scene(rwr, suzanne, first)) as (on, off):
        cam_inv = _cam(rwr, size, **CAMS["A"])
        launches = 0
        frames = []
        for spheres in (first, other, [], first):
            for c in (on, off):
                c.set_spheres(rwr.make_spheres(spheres))
            launches += 1
            for i in range(3):
                got = _frame(rwr, on, off, cam_inv, rwr.FLAG_AUX_OUTPUTS, what=(len(spheres), i))
                assert on.frame_setup_launches() == off.frame_setup_launches() == launches, (spheres, i)
            ids = {int(v) for v in np.unique(got["obj_id"]) if v <= -2}
            assert (ids <= {-2 - s for s in range(len(spheres))}) and bool(ids) == bool(spheres), (spheres, ids)
            cls = on.tile_classes()
            assert bool((cls & SPHERES).any()) == bool(spheres)
            assert not (cls & np.uint32(SPHERES & ~(((1 << len(spheres)) - 1) << 16))).any()   # no bit at or above the sphere count
            frames.append(got)
        assert _differ(frames[0], frames[1]) and _differ(frames[1], frames[2]) and not _differ(frames[0], frames[3])
        assert np.array_equal(frames[0]["depth"], frames[3]["depth"])


@pytest.mark.parametrize("n_slots", [2, 3])
def test_strips_bands_a_moving_camera_and_resize(rwr, suzanne, n_slots):
    size = (130, 24)
    aux = rwr.FLAG_AUX_OUTPUTS
    with _pair(rwr, size, n_slots, _suzanne_scene(rwr, suzanne)) as (on, off):
        cam_inv = _cam(rwr, size, **CAMS["A"])
        reps = 2 * n_slots + 1
        for _ in range(reps):
            whole = _frame(rwr, on, off, cam_inv, aux)
        for _ in range(reps):
            band = _frame(rwr, on, off, cam_inv, aux, rows=(8, 16))
        assert np.array_equal(band["color"][8:16], whole["color"][8:16]) and np.array_equal(band["hit_t"][8:16], whole["hit_t"][8:16])
        for _ in range(reps):
            strip = _frame(rwr, on, off, cam_inv, aux, strips=(1, 3))
        assert np.array_equal(strip["color"][8:16], whole["color"][8:16]) and np.array_equal(strip["depth"][8:16], whole["depth"][8:16])
        # a camera that moves every frame, several frames queued before one is read back
        cams = [_cam(rwr, size, (0.08 * k, 0.03 * k, 2.8 - 0.2 * k), (0, 0, -1)) for k in range(6)]
        for k, c in enumerate(cams):
            _frame(rwr, on, off, c, aux if k % 2 else 0, what=("moving", k))
        queued = []
        for ctx in (on, off):
            for c in cams:
                ctx.render(c, rwr.make_params())
            queued.append(ctx.readback())
        for k in queued[0]:
            assert np.array_equal(queued[0][k].view(np.uint8), queued[1][k].view(np.uint8)), ("queued", k)
        # rwr_resize between frames, and back
        for new in ((65, 9), (256, 64), size):
            for ctx in (on, off):
                ctx.resize(*new)
            c = _cam(rwr, new, **CAMS["B"])
            for i in range(reps):
                got = _frame(rwr, on, off, c, aux if i % 2 else 0, what=("resized", new, i))
            assert on.tile_classes().shape == (2 * ((new[1] + 7) // 8), 2 * ((new[0] + 63) // 64))
        assert got["color"].any()


def _write_two_object_scene(d):
    """The scene of tests/test_multi_material.py: two parts with a material and a texture each."""
    from PIL import Image
    rng = np.random.default_rng(5)
    Image.fromarray(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8), "RGB").save(d / "a.png")
    Image.fromarray(rng.integers(0, 256, (8, 32, 4), dtype=np.uint8), "RGBA").save(d / "b.png")
    (d / "two.mtl").write_text(
        "newmtl red\nKa 0.20 0.02 0.02\nKd 1 1 1\nKs 0.5 0.5 0.5\nmap_Kd a.png\n"
        "newmtl blue\nKa 0.02 0.02 0.30\nKd 1 1 1\nKs 0.1 0.2 0.3\nmap_Kd b.png\n")
    (d / "two.obj").write_text(
        "mtllib two.mtl\n"
        "o left\nv -2 -1 -4\nv 0 -1 -4\nv 0 1 -4\nv -2 1 -4\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\n"
        "usemtl red\nf 1/1 2/2 3/3 4/4\n"
        "o right\nv -0.5 -1 -5\nv 2 -1 -3\nv 2 1 -3\nv -0.5 1 -5\n"
        "usemtl blue\nf 5/1 6/2 7/3\nf 5/1 7/3 8/4\n")


def test_multi_material_scene(rwr, tmp_path):
    """Four faces in two materials: tiles with one face exist, and a frame with several materials shades per pixel."""
    _write_two_object_scene(tmp_path)
    parts = rwr.load_model_parts("two.obj", str(tmp_path))
    size = (120, 72)

    def setup(c):
        c.upload_parts(parts)
        c.set_spheres(rwr.make_spheres([((0.6, 0.5, -3.5), 0.4)]))

    aux = rwr.FLAG_AUX_OUTPUTS
    with _pair(rwr, size, 1, setup) as (on, off):
        cam_inv = _cam(rwr, size, (0.2, 0.1, 0.5), (0, 0, -4))
        for flags in (0, aux, aux | rwr.FLAG_DEBUG_COUNTS, aux):
            got = _frame(rwr, on, off, cam_inv, flags)
        assert {0, 1, 2, 3} <= set(np.unique(got["obj_id"]).tolist())
        assert ((on.tile_classes() & (FACES | SPHERES)) == 1).any()


def test_normal_mapped_frame(rwr, suzanne, cube):
    size = (200, 112)

    def setup(c):
        c.upload_model(suzanne)
        c.set_spheres(rwr.make_spheres())
        c.set_normal_map(0, cube["normal_map"])

    aux = rwr.FLAG_AUX_OUTPUTS
    with _pair(rwr, size, 1, setup) as (on, off):
        cam_inv = _cam(rwr, size, (0.3, 0.2, 2.6), (0, 0, 0))
        plain = _frame(rwr, on, off, cam_inv, aux)
        for flags in (rwr.FLAG_NORMAL_MAP, aux | rwr.FLAG_NORMAL_MAP, aux | rwr.FLAG_NORMAL_MAP | rwr.FLAG_DEBUG_COUNTS, aux | rwr.FLAG_NORMAL_MAP):
            got = _frame(rwr, on, off, cam_inv, flags)
        assert (got["obj_id"] >= 0).any() and _differ(plain, got)
        assert (on.tile_classes() & FACES).any()


def test_binned_scene_has_no_classes(rwr, cube):
    """cube.obj, 428 faces: per-bin face lists, no face sets and no class words — the frames are what they were."""
    size = (129, 17)

    def setup(c):
        c.upload_model(cube)
        c.set_spheres(rwr.make_spheres())

    with _pair(rwr, size, 2, setup) as (on, off):
        for cam in "RRRRRAAAAA":
            got = _frame(rwr, on, off, _cam(rwr, size, **CAMS[cam]), rwr.FLAG_AUX_OUTPUTS if cam == "A" else 0)
        assert (got["obj_id"] >= 0).any()
        for c in (on, off):
            with pytest.raises(rwr.RwrError) as e:
                c.tile_classes()
            assert e.value.code == rwr.ERR_NOT_READY


@pytest.mark.parametrize("cam", ["R", "A"])
@pytest.mark.parametrize("size", [(256, 64), (320, 180)], ids=lambda s: "%dx%d" % s)
def test_class_words_against_the_other_contexts_counts(rwr, suzanne, size, cam):
    """The words of the context with classes against a model from the context WITHOUT them: a tile is "none" iff its listed
    count (debug plane: faces the tile's culling keeps, 0 outside the mesh rectangle) is 0, "one" iff 1, else "more"; every mesh
    pixel of a "one" tile shows the word's face; a tile with no sphere bit has no sphere pixel."""
    w, h = size
    aux = rwr.FLAG_AUX_OUTPUTS
    with _pair(rwr, size, 1, _suzanne_scene(rwr, suzanne, [((0.5, 0.3, 1.5), 0.3), ((0.4, 0.4, -3.0), 0.4)])) as (on, off):
        cam_inv = _cam(rwr, size, **CAMS[cam])
        off.render(cam_inv, rwr.make_params(flags=aux | rwr.FLAG_DEBUG_COUNTS))
        listed = off.readback(aux=True)["obj_id"]
        off.render(cam_inv, rwr.make_params(flags=aux))
        ids = off.readback(aux=True)["obj_id"]
        on.render(cam_inv, rwr.make_params())
        cls = on.tile_classes()
        assert cls.shape == (2 * ((h + 7) // 8), 2 * ((w + 63) // 64)) and cls.dtype == np.uint32
        assert not (cls & ~np.uint32(FACES | 0xff00 | SPHERES)).any()
        counts = {0: 0, 1: 0, 2: 0}
        for ty in range(cls.shape[0]):
            for tx in range(cls.shape[1]):
                tile = (slice(4 * ty, min(h, 4 * ty + 4)), slice(32 * tx, min(w, 32 * tx + 32)))
                n = listed[tile]
                if n.size == 0:
                    continue   # (a tile of the grid's padding: no pixel to ask)
                assert (n == n.flat[0]).all()
                c = int(cls[ty, tx])
                want = min(int(n.flat[0]), 2)
                assert (c & FACES) == want, (ty, tx, c, int(n.flat[0]))
                counts[want] += 1
                t = ids[tile]
                if want == 1:
                    assert (t[t >= 0] == ((c >> 8) & 0xff)).all(), (ty, tx, c)
                else:
                    assert ((c >> 8) & 0xff) == 0
                if not c & SPHERES:
                    assert not (t <= -2).any(), (ty, tx, c)
        # (inside the mesh there are tiles with one face and with more; from outside most hold none)
        assert (counts[1] > 0 and counts[2] > 0) if cam == "R" else (counts[0] > counts[1] + counts[2] > 0), counts
        assert (cls & SPHERES).any() and (cam == "R" or (ids <= -2).any())
