"""Cover words (RWR_TILE_COVER, default on): a frame served from its slot's kept records learns, with the straight path's own tests,
which tiles of class "one face, no sphere" that face covers entirely (every pixel pair hits, wins the depth test, both short forms
in their domain) and leaves one word per tile beside the class words; the slot's later frames with the same records take such a
tile without the tests that could only confirm it.  Every k_frame_setup launch zeroes the words.  The method is that of
test_gpu_tile_class.py: every sequence is rendered in two fresh contexts that differ in RWR_TILE_COVER alone (=0: no frame looks at
the words), given the same calls, and every plane of every frame must be the same bytes in both — no tolerance.  The words are read
back (rwr_debug_tile_cover) and compared with a model built from the *other* context's class words and object ids.

The contexts run with RWR_FUSED_SETUP=0, so that these small frames take the two launches per frame a 1080p frame takes."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLAIN_ENV = dict(RWR_FUSED_SETUP="0", RWR_AUTO_BVH_FACE_PX="0")
FACES, SPHERES = 0x3, 0xff0000
REST = dict(eye=(0, 0, 0), target=(0, 0, -1))   # the reference camera, inside suzanne: most tiles show one face


@contextlib.contextmanager
def _pair(rwr, size, n_slots=1, setup=None, env=PLAIN_ENV):
    """(cover on, cover off): two fresh contexts that differ in RWR_TILE_COVER alone (the knobs are read at creation)."""
    mp = pytest.MonkeyPatch()
    ctxs = []
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        for v in ("1", "0"):
            mp.setenv("RWR_TILE_COVER", v)
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


def _scene(rwr, model, spheres=()):
    def setup(c):
        c.upload_model(model)
        c.set_spheres(rwr.make_spheres(list(spheres)))
    return setup


def _cam(rwr, size, eye, target):
    return rwr.camera_build_inv_uniform(rwr.make_camera(eye=eye, target=target, aspect=size[0] / size[1]))


def _frame(rwr, on, off, cam_inv, flags=0, rows=None, strips=None, what=None):
    """One frame in both contexts; all planes byte-identical.  Returns the planes of the context with cover words."""
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


def _model(rwr, off, cam_inv, size):
    """From the context WITHOUT cover words (its class words and the object ids of an aux frame): `exact`, the tiles with all 128
    pixels in the frame whose class is "one face, no sphere" and whose every pixel shows that face, and `may`, the same rule over
    the in-frame pixels of every tile (a word may only be set there).  Whole-frame launches (tile [ty, tx] = rows
    4 ty .., columns 32 tx ..)."""
    w, h = size
    off.render(cam_inv, rwr.make_params(flags=rwr.FLAG_AUX_OUTPUTS))
    ids = off.readback(aux=True)["obj_id"]
    cls = off.tile_classes()
    exact, may = np.zeros(cls.shape, bool), np.zeros(cls.shape, bool)
    for ty in range(cls.shape[0]):
        for tx in range(cls.shape[1]):
            t = ids[4 * ty:min(h, 4 * ty + 4), 32 * tx:min(w, 32 * tx + 32)]
            c = int(cls[ty, tx])
            if (c & (FACES | SPHERES)) != 1:
                continue
            may[ty, tx] = bool((t == ((c >> 8) & 0xff)).all())   # (a tile of the grid's padding has no pixel to contradict a word)
            exact[ty, tx] = may[ty, tx] and t.size == 128
    return exact, may, cls


def _rest_sequence(rwr, on, off, cam_inv, n_slots, flags_of=lambda i: 0, **kw):
    """3 n frames at rest after something made every slot's records stale, so that each slot goes miss -> learn -> use, with the
    counters that go with it.  Returns the words after the last frame."""
    frames0, _ = on.tile_cover_stats()
    launches0 = on.frame_setup_launches()
    taken = []
    for i in range(3 * n_slots):
        _frame(rwr, on, off, cam_inv, flags_of(i), what=("rest", i), **kw)
        frames, tiles = on.tile_cover_stats()
        assert frames == frames0 + max(0, i + 1 - n_slots), i             # every frame after a slot's first looks at the words
        assert on.frame_setup_launches() == launches0 + min(i + 1, n_slots), i
        words = on.tile_cover()
        if i < n_slots:
            assert not words.any() and tiles == 0, i                      # a frame that made its records: the words are zeroed, none written
        elif i < 2 * n_slots:
            assert tiles == 0, i                                          # the slot's first frame with the flag learns, takes none
        else:
            assert tiles == int(words.sum()), i                           # the third frame on a slot took what the second learnt
        taken.append(tiles)
        assert not (words & ~np.uint32(1)).any()
    assert off.tile_cover_stats() == (0, 0) and not off.tile_cover().any()
    return words, taken


@pytest.mark.parametrize("n_slots", [1, 2, 3])
@pytest.mark.parametrize("size", [(256, 144), (320, 200), (96, 52)], ids=lambda s: "%dx%d" % s)
def test_sizes_and_slots(rwr, suzanne, size, n_slots):
    """suzanne from the origin.  256x144 and 320x200: every lane in the frame, the words are exactly the model's tiles (the CPU
    oracle gives 190 of 288 and 382 of 500 tiles fully one face; those among them whose face set holds that face alone).  96x52: width and rows no multiples of the workgroup — a word
    only where every in-frame pixel shows the face.  3 n frames (six or more for n >= 2; n = 1 runs six), plain, aux and
    debug-count forms in turn, so that what one form learnt the others use."""
    aux = rwr.FLAG_AUX_OUTPUTS
    forms = (0, aux, aux | rwr.FLAG_DEBUG_COUNTS)
    with _pair(rwr, size, n_slots, _scene(rwr, suzanne)) as (on, off):
        cam_inv = _cam(rwr, size, **REST)
        exact, may, cls = _model(rwr, off, cam_inv, size)
        words, taken = _rest_sequence(rwr, on, off, cam_inv, n_slots, lambda i: forms[i % 3])
        if n_slots == 1:
            for i in range(3):
                _frame(rwr, on, off, cam_inv, forms[i], what=("more", i))
                assert on.tile_cover_stats()[1] == int(words.sum())
        assert np.array_equal(on.tile_classes(), cls)
        got = on.tile_cover() == 1
        assert taken[-1] > 0 and got.any()
        assert not (got & ~may).any()
        if size != (96, 52):
            assert np.array_equal(got, exact), (int(got.sum()), int(exact.sum()))
            # (the CPU oracle's count of tiles that show one face throughout; a tile among them whose set holds more faces has no word)
            assert 0 < int(exact.sum()) <= {(256, 144): 190, (320, 200): 382}[size]
        # the debug counts of a covered tile are those of the straight path: one face listed, one tested
        out = _frame(rwr, on, off, cam_inv, aux | rwr.FLAG_DEBUG_COUNTS)
        ty, tx = np.argwhere(got)[0]
        assert (out["obj_id"][4 * ty:4 * ty + 4, 32 * tx:32 * tx + 32] == 1).all() and (out["hit_t"][4 * ty:4 * ty + 4, 32 * tx:32 * tx + 32] == 1.0).all()


def _write_face(d, name, verts):
    """A one-face model with a material and a texture."""
    from PIL import Image
    rng = np.random.default_rng(11)
    Image.fromarray(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8), "RGB").save(d / "t.png")
    (d / "m.mtl").write_text("newmtl m\nKa 0.1 0.1 0.1\nKd 1 1 1\nKs 0.3 0.3 0.3\nmap_Kd t.png\n")
    (d / name).write_text("mtllib m.mtl\n" + "".join("v %r %r %r\n" % v for v in verts) + "vt 0 0\nvt 1 0\nvt 0 1\nusemtl m\nf 1/1 2/2 3/3\n")


# what the face must show: "some" tiles wholly and some partly / nothing (beyond the far plane, 100) / everything, and no word
ONE_FACE = {
    "partly": ([(-2.0, -1.0, -1.0), (2.0, -1.0, -1.0), (0.0, 1.5, -1.0)], "some"),   # (the CPU oracle: 108 tiles wholly, 74 partly)
    "beyond_far": ([(-200.0, -100.0, -150.0), (200.0, -100.0, -150.0), (0.0, 300.0, -150.0)], "nothing"),
    # N = e0 x e1 = (0, 0, 2.4e13), tnum = dot(N, p0 - O) = 1.2e15 > 2^40 (and |ndotd| with it): the compiler's division
    "scaled": ([(-3.0e6, -1.0e6, -50.0), (3.0e6, -1.0e6, -50.0), (0.0, 3.0e6, -50.0)], "no word"),
}


@pytest.mark.parametrize("case", sorted(ONE_FACE))
def test_tiles_that_must_not_be_learnt(rwr, tmp_path, case):
    verts, shows = ONE_FACE[case]
    _write_face(tmp_path, "one.obj", verts)
    model = rwr.load_model_compute("one.obj", str(tmp_path))
    size = (256, 144)
    with _pair(rwr, size, 1, _scene(rwr, model)) as (on, off):
        cam_inv = _cam(rwr, size, **REST)
        exact, may, cls = _model(rwr, off, cam_inv, size)
        one = (cls & (FACES | SPHERES)) == 1
        words, taken = _rest_sequence(rwr, on, off, cam_inv, 1, lambda i: rwr.FLAG_AUX_OUTPUTS if i % 2 else 0)
        got = words == 1
        if shows == "some":
            assert np.array_equal(got, exact) and got.any() and (one & ~got).any()   # (edge tiles: class one, not covered)
            assert taken[-1] == int(got.sum())
        elif shows == "nothing":
            assert one.any() and not exact.any() and not got.any()
        else:
            assert exact.any() and not got.any()   # every pixel of such a tile shows the face, and the short division is out of its domain
            assert taken[-1] == 0


def test_forgetting(rwr, suzanne):
    """With the camera resting, everything that makes the slot's records again clears the words, and they are learnt again."""
    size = (256, 144)
    n = 2
    with _pair(rwr, size, n, _scene(rwr, suzanne)) as (on, off):
        cam_inv = _cam(rwr, size, **REST)
        exact, _, _ = _model(rwr, off, cam_inv, size)
        words, _ = _rest_sequence(rwr, on, off, cam_inv, n)
        assert np.array_equal(words == 1, exact)
        # a sphere moved across covered tiles: their class changes, other words return
        # (in front of the mesh, left and right of the middle: on the CPU oracle the first shows in six tiles one face covers)
        for k, sphere in enumerate([((-0.4, 0.1, -0.5), 0.1), ((0.4, -0.1, -0.5), 0.1)]):
            for c in (on, off):
                c.set_spheres(rwr.make_spheres([sphere]))
            with_sphere, _, cls = _model(rwr, off, cam_inv, size)
            words, taken = _rest_sequence(rwr, on, off, cam_inv, n)
            assert np.array_equal(words == 1, with_sphere) and (exact & ~with_sphere).any() and taken[-1] > 0, k
        for c in (on, off):
            c.set_spheres(rwr.make_spheres([]))
        words, _ = _rest_sequence(rwr, on, off, cam_inv, n)
        assert np.array_equal(words == 1, exact)
        # the same model uploaded again
        for c in (on, off):
            c.upload_model(suzanne)
        words, _ = _rest_sequence(rwr, on, off, cam_inv, n)
        assert np.array_equal(words == 1, exact)
        # a camera step and the step back
        step = _cam(rwr, size, (0.02, 0.0, 0.0), (0.02, 0, -1))
        stepped, _, _ = _model(rwr, off, step, size)
        words, _ = _rest_sequence(rwr, on, off, step, n)
        assert np.array_equal(words == 1, stepped)
        words, _ = _rest_sequence(rwr, on, off, cam_inv, n)
        assert np.array_equal(words == 1, exact)
        # rwr_resize and back
        other = (320, 200)
        for c in (on, off):
            c.resize(*other)
        cam_o = _cam(rwr, other, **REST)
        exact_o, _, _ = _model(rwr, off, cam_o, other)
        words, _ = _rest_sequence(rwr, on, off, cam_o, n)
        assert np.array_equal(words == 1, exact_o)
        for c in (on, off):
            c.resize(*size)
        words, _ = _rest_sequence(rwr, on, off, cam_inv, n)
        assert np.array_equal(words == 1, exact)
        # other rows: a band, every third strip, the whole frame again
        for kw in (dict(rows=(8, 72)), dict(strips=(1, 3)), dict(rows=(16, 144)), dict()):
            words, taken = _rest_sequence(rwr, on, off, cam_inv, n, **kw)
            assert taken[-1] > 0, kw
        assert np.array_equal(words == 1, exact)


def test_without_the_ray_plane(rwr, suzanne):
    """RWR_RAY_PLANE=0: the resting frames compute their rays, and learn and use the words in the kernel's computing form."""
    size = (256, 144)
    aux = rwr.FLAG_AUX_OUTPUTS
    with _pair(rwr, size, 2, _scene(rwr, suzanne), env=dict(PLAIN_ENV, RWR_RAY_PLANE="0")) as (on, off):
        cam_inv = _cam(rwr, size, **REST)
        exact, _, _ = _model(rwr, off, cam_inv, size)
        words, taken = _rest_sequence(rwr, on, off, cam_inv, 2, lambda i: (0, aux, aux | rwr.FLAG_DEBUG_COUNTS)[i % 3])
        assert on.ray_plane_stats() == (0, 0)
        assert np.array_equal(words == 1, exact) and taken[-1] == int(exact.sum()) > 0


def test_setup_cache_off_never_looks(rwr, suzanne):
    size = (256, 144)
    with _pair(rwr, size, 2, _scene(rwr, suzanne), env=dict(PLAIN_ENV, RWR_SETUP_CACHE="0")) as (on, off):
        cam_inv = _cam(rwr, size, **REST)
        for i in range(6):
            _frame(rwr, on, off, cam_inv, rwr.FLAG_AUX_OUTPUTS if i % 2 else 0)
            assert on.tile_cover_stats() == (0, 0) and not on.tile_cover().any()
        assert on.frame_setup_launches() == 6


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


INERT = ["tile_class_off", "binned_cube", "fused", "graph", "multi_material", "normal_map", "one_pixel_per_lane"]


@pytest.mark.parametrize("case", INERT)
def test_inert_elsewhere(rwr, suzanne, cube, tmp_path, case):
    """Frames that do not take the straight path look at no cover word: the counter stays zero, the frames are what they are."""
    size = (256, 144)
    env = dict(PLAIN_ENV)
    flags = [0, rwr.FLAG_AUX_OUTPUTS]
    setup = _scene(rwr, suzanne)
    cam = REST
    if case == "tile_class_off":
        env["RWR_TILE_CLASS"] = "0"
    elif case == "binned_cube":
        setup = _scene(rwr, cube)
    elif case == "fused":
        env["RWR_FUSED_SETUP"] = "1"
        flags = [0]   # (the fused form is the plain frame's)
    elif case == "graph":
        env["RWR_FRAME_GRAPH"] = "1"
        flags = [0]
    elif case == "multi_material":
        _write_two_object_scene(tmp_path)
        parts = rwr.load_model_parts("two.obj", str(tmp_path))

        def setup(c):
            c.upload_parts(parts)
            c.set_spheres(rwr.make_spheres([]))
        cam = dict(eye=(0.2, 0.1, 0.5), target=(0, 0, -4))
    elif case == "normal_map":
        def setup(c):
            c.upload_model(suzanne)
            c.set_spheres(rwr.make_spheres([]))
            c.set_normal_map(0, cube["normal_map"])
        flags = [rwr.FLAG_NORMAL_MAP, rwr.FLAG_NORMAL_MAP | rwr.FLAG_AUX_OUTPUTS]
    elif case == "one_pixel_per_lane":
        env["RWR_ONE_PIXEL_PER_LANE"] = "1"
    with _pair(rwr, size, 2, setup, env=env) as (on, off):
        cam_inv = _cam(rwr, size, **cam)
        shown = False
        for i in range(8):
            got = _frame(rwr, on, off, cam_inv, flags[i % len(flags)], what=(case, i))
            assert on.tile_cover_stats() == (0, 0), (case, i)
            shown |= bool(got["color"].any())
        assert shown
        try:
            assert not on.tile_cover().any()
        except rwr.RwrError as e:
            assert e.code == rwr.ERR_NOT_READY   # (a frame without class words)
