"""The frame kernel's lean resting form (RWR_LEAN_REST, default on; kernels_primary_p2.hip k_primary_p2_lean): a resting camera's
plain frame — rays from the slot's kept plane, cover words, per-tile face sets, one material, colour and depth alone — runs an
entry point of its own without culling records in LDS, without a workgroup barrier and within 80 scalar registers.  Its arithmetic
is the cover form's, so the method is that of test_gpu_tile_cover.py: every sequence is rendered in two fresh contexts that differ
in RWR_LEAN_REST alone (=0: the cover form renders those frames), given the same calls, and colour and depth of every frame must
be the same bytes in both — no tolerance.  rwr_lean_rest_stats keeps the comparison from being vacuous: the count must move in the
"on" context wherever the form is due, and stay 0 in the "off" context and for every frame that is not of the form's kind.

The contexts run with RWR_FUSED_SETUP=0, so that these small frames take the two launches per frame a 1080p frame takes."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLAIN_ENV = dict(RWR_FUSED_SETUP="0", RWR_AUTO_BVH_FACE_PX="0")
FACES, SPHERES = 0x3, 0xff0000
CFG2 = dict(eye=(0, 0, 0), target=(0, 0, -1))    # bench.py cfg2: the reference camera, inside suzanne
CFG2B = dict(eye=(0, 0, 3), target=(0, 0, -1))   # bench.py cfg2b: the mesh in the middle of the frame, nothing around it
ONE_SPHERE = [((-0.4, 0.1, -0.5), 0.1)]          # in front of the mesh, left of the middle (test_gpu_tile_cover.py)


@contextlib.contextmanager
def _pair(rwr, size, n_slots=1, setup=None, env=PLAIN_ENV):
    """(lean on, lean off): two fresh contexts that differ in RWR_LEAN_REST alone (the knobs are read at creation)."""
    mp = pytest.MonkeyPatch()
    ctxs = []
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        for v in ("1", "0"):
            mp.setenv("RWR_LEAN_REST", v)
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


def _scene(rwr, model, spheres=None):
    def setup(c):
        c.upload_model(model)
        c.set_spheres(rwr.make_spheres() if spheres is None else rwr.make_spheres(list(spheres)))
    return setup


def _cam(rwr, size, eye, target):
    return rwr.camera_build_inv_uniform(rwr.make_camera(eye=eye, target=target, aspect=size[0] / size[1]))


def _frame(rwr, on, off, cam_inv, flags=0, rows=None, strips=None, what=None):
    """One frame in both contexts; every plane byte-identical.  Returns the planes of the "on" context."""
    params = rwr.make_params(flags=flags)
    aux = bool(flags & rwr.FLAG_AUX_OUTPUTS)
    got = []
    for c in (on, off):
        c.render(cam_inv, params, rows=rows, strips=strips)
        got.append(c.readback(aux=aux))
    assert {"color", "depth"} <= set(got[0])
    for k in got[0]:
        assert np.array_equal(got[0][k].view(np.uint8), got[1][k].view(np.uint8)), (what, flags, rows, strips, k)
    return got[0]


def _rest(rwr, on, off, cam_inv, n_slots, what, flags=0, **kw):
    """4 n frames at rest: each slot makes its records, learns the cover words, then uses them — with two slots the lean form is
    due from frame 5 on.  Returns how many frames the "on" context launched in the lean form."""
    before = on.lean_rest_stats()
    shown = False
    for i in range(4 * n_slots):
        got = _frame(rwr, on, off, cam_inv, flags, what=(what, i), **kw)
        shown |= bool(got["color"].any())
        assert off.lean_rest_stats() == 0, (what, i)
    assert shown, what
    return on.lean_rest_stats() - before


def _fully_one_face(rwr, off, cam_inv, size):
    """From the context WITHOUT the lean form (its class words and the object ids of an aux frame): the tiles with all 128 pixels in
    the frame whose class is "one face, no sphere" and whose every pixel shows that face — the tiles a resting frame learns as
    covered (test_gpu_tile_cover.py _model) — and the class words.  Whole-frame launches."""
    w, h = size
    off.render(cam_inv, rwr.make_params(flags=rwr.FLAG_AUX_OUTPUTS))
    ids = off.readback(aux=True)["obj_id"]
    cls = off.tile_classes()
    exact = np.zeros(cls.shape, bool)
    for ty in range(cls.shape[0]):
        for tx in range(cls.shape[1]):
            t = ids[4 * ty:min(h, 4 * ty + 4), 32 * tx:min(w, 32 * tx + 32)]
            c = int(cls[ty, tx])
            exact[ty, tx] = (c & (FACES | SPHERES)) == 1 and t.size == 128 and bool((t == ((c >> 8) & 0xff)).all())
    return exact, cls


# name: (size, slots, pose, spheres (None: the reference's two))
MAIN = {
    "64x8": ((64, 8), 2, CFG2, None),             # one workgroup (four tiles of several faces each: none to take as covered)
    "65x9": ((65, 9), 2, CFG2, None),             # odd width: no pair stores on odd rows, partial tiles and workgroups
    "130x20": ((130, 20), 2, CFG2, None),
    "256x144_1slot": ((256, 144), 1, CFG2, None),
    "256x144_2slots": ((256, 144), 2, CFG2, None),
    "256x144_3slots": ((256, 144), 3, CFG2, None),
    "cfg2b_256x144": ((256, 144), 2, CFG2B, None),           # tiles of class "none" around the mesh
    "sphere_256x144": ((256, 144), 2, CFG2, ONE_SPHERE),     # a sphere on screen, across tiles one face would cover
}


@pytest.mark.parametrize("case", sorted(MAIN))
def test_same_bytes_as_the_cover_form(rwr, suzanne, case):
    size, n_slots, pose, spheres = MAIN[case]
    with _pair(rwr, size, n_slots, _scene(rwr, suzanne, spheres)) as (on, off):
        cam_inv = _cam(rwr, size, **pose)
        exact, cls = _fully_one_face(rwr, off, cam_inv, size)
        on.render(cam_inv, rwr.make_params(flags=rwr.FLAG_AUX_OUTPUTS))   # (the same calls in both)
        on.readback(aux=True)
        assert on.lean_rest_stats() == 0   # (a frame with the extra outputs)
        lean = _rest(rwr, on, off, cam_inv, n_slots, case)
        assert lean >= 2 * n_slots, (case, lean)   # every frame behind the slots' record-making and learning ones
        assert np.array_equal(on.tile_classes(), cls)
        # the tiles the lean frames took as covered: what the off context's class words and object ids say they must be
        frames, tiles = on.tile_cover_stats()
        assert tiles == off.tile_cover_stats()[1] >= int(exact.sum()), case
        assert np.array_equal(on.tile_cover(), off.tile_cover())
        one = (cls & (FACES | SPHERES)) == 1
        if pose is CFG2:
            # First the off context's class words: does the pose have a one-face tile at this shape?  It has at every shape but 64x8,
            # whose four tiles hold several faces each (measured: class one in 0 of 4, 6 of 16, 10 of 36 and 142 of 288 tiles; at
            # 65x9 and 130x20 they are tiles of the grid's padding, whose every lane hits all the same).  Then the lean frames took
            # some of them as covered.
            assert one.any() == (case != "64x8"), (case, int(one.sum()))
            assert (tiles > 0) == bool(one.any()), (case, int(one.sum()), int(exact.sum()), tiles)
        if size == (256, 144) and pose is CFG2:
            assert exact.any() and tiles == int(exact.sum())


def test_the_cases_show_every_class(rwr, suzanne):
    """Over MAIN as a whole the class words show tiles of class none, one, more and with a sphere bit: all three ways through a
    tile, and the sphere passes, run in the lean form."""
    seen = set()
    with _pair(rwr, (256, 144), 1, _scene(rwr, suzanne)) as (on, off):
        for case in sorted(MAIN):
            size, _, pose, spheres = MAIN[case]
            off.resize(*size)
            off.set_spheres(rwr.make_spheres() if spheres is None else rwr.make_spheres(list(spheres)))
            off.render(_cam(rwr, size, **pose), rwr.make_params())
            cls = off.tile_classes()
            seen |= {("none", "one", "more")[int(c) & FACES] for c in cls.ravel() if (int(c) & FACES) < 3}
            if (cls & SPHERES).any():
                seen.add("sphere")
    assert seen == {"none", "one", "more", "sphere"}, seen


@pytest.mark.parametrize("rank", [0, 1])
def test_strips_of_two_ranks(rwr, suzanne, rank):
    """row_begin / row_pitch as rwr_render_strips sets them for rank `rank` of two: every second 8-row strip."""
    size = (256, 144)
    with _pair(rwr, size, 2, _scene(rwr, suzanne)) as (on, off):
        cam_inv = _cam(rwr, size, **CFG2)
        assert _rest(rwr, on, off, cam_inv, 2, ("strips", rank), strips=(rank, 2)) >= 4
        assert on.tile_cover_stats()[1] == off.tile_cover_stats()[1] > 0


def test_sequences_that_forget(rwr, suzanne):
    """What makes a slot's records again (test_gpu_tile_cover.py test_forgetting): the frames behind it are the cover form's bytes
    all the way, and the lean form is back once the slots have learnt again."""
    size, n = (256, 144), 2
    with _pair(rwr, size, n, _scene(rwr, suzanne)) as (on, off):
        cam_inv = _cam(rwr, size, **CFG2)
        assert _rest(rwr, on, off, cam_inv, n, "start") >= 2 * n
        step = _cam(rwr, size, (0.02, 0.0, 0.0), (0.02, 0, -1))
        assert _rest(rwr, on, off, step, n, "camera step") >= 2 * n
        assert _rest(rwr, on, off, cam_inv, n, "step back") >= 2 * n
        for k, spheres in enumerate((ONE_SPHERE, [])):
            for c in (on, off):
                c.set_spheres(rwr.make_spheres(spheres))
            assert _rest(rwr, on, off, cam_inv, n, ("set_spheres", k)) >= 2 * n
        for c in (on, off):
            c.upload_model(suzanne)
        assert _rest(rwr, on, off, cam_inv, n, "upload") >= 2 * n
        other = (320, 200)
        for c in (on, off):
            c.resize(*other)
        assert _rest(rwr, on, off, _cam(rwr, other, **CFG2), n, "resize") >= 2 * n
        for c in (on, off):
            c.resize(*size)
        assert _rest(rwr, on, off, cam_inv, n, "resize back") >= 2 * n
        for kw in (dict(rows=(8, 72)), dict(strips=(1, 3)), dict(rows=(16, 144)), dict()):
            assert _rest(rwr, on, off, cam_inv, n, ("rows", kw), **kw) >= 2 * n, kw
        # one frame in three with the extra outputs: those run the cover form, on records and words the lean frames share
        aux = rwr.FLAG_AUX_OUTPUTS
        before = on.lean_rest_stats()
        for i in range(9):
            _frame(rwr, on, off, cam_inv, aux if i % 3 == 2 else 0, what=("mixed", i))
        assert on.lean_rest_stats() - before == 6


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


FALL_BACK = ["binned_cube", "aux_outputs", "two_materials", "normal_map", "ray_plane_off", "tile_cover_off", "tile_lists_off"]


@pytest.mark.parametrize("case", FALL_BACK)
def test_every_other_frame_runs_what_it_ran(rwr, suzanne, cube, tmp_path, case):
    """Frames that are not of the lean form's kind: the count stays 0 in both contexts, the frames are the same bytes."""
    size = (256, 144)
    env = dict(PLAIN_ENV)
    flags = 0
    setup = _scene(rwr, suzanne)
    cam = CFG2
    if case == "binned_cube":   # 428 faces: screen bins, no per-tile sets
        setup = _scene(rwr, cube)
    elif case == "aux_outputs":
        flags = rwr.FLAG_AUX_OUTPUTS
    elif case == "two_materials":
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
        flags = rwr.FLAG_NORMAL_MAP
    elif case == "ray_plane_off":
        env["RWR_RAY_PLANE"] = "0"
    elif case == "tile_cover_off":
        env["RWR_TILE_COVER"] = "0"
    elif case == "tile_lists_off":
        env["RWR_TILE_LISTS"] = "0"
    with _pair(rwr, size, 2, setup, env=env) as (on, off):
        cam_inv = _cam(rwr, size, **cam)
        assert _rest(rwr, on, off, cam_inv, 2, case, flags=flags) == 0
        assert on.lean_rest_stats() == 0 and off.lean_rest_stats() == 0
