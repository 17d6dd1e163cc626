"""While the camera rests, the two-pixel frame kernel loads the normalised ray directions of its pixel pairs from a plane the
frame slot keeps (frame_records.cpp ray_plane_step; k_ray_plane fills it with the frame kernel's own ray function) instead of computing
them.  Every sequence here is rendered in two contexts, the plane on and RWR_RAY_PLANE=0, given the same calls: every plane of
every frame must be the same bytes in both — no tolerance, both sides run the same function — and rwr_ray_plane_stats must show
exactly the builds and the loading frames the sequence implies.

The expected counts come from a model of what the slots are specified to do, not from the library: frames take the slots in
turn; a frame that can use a plane (the reference frame in the two-pixel kernel's culled two-launch form) has the key (camera,
screen, rows); if its slot's plane was built for that key it loads; else if the slot's last such frame had the key, the plane is
built once and the frame loads; otherwise the key is remembered and the frame computes.  Scene changes do not enter the key;
rwr_resize clears every slot's; frames that cannot use a plane (path-traced, fused) pass the slot's key by.

The contexts run with RWR_FUSED_SETUP=0, so that these small frames take the two launches per frame a 1080p frame takes, and
RWR_AUTO_BVH_FACE_PX=0, so that cube.obj's small faces stay in the (binned) two-pixel kernel; one test keeps the default rules."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# an odd width (a lane's second pixel off the frame), widths / heights that are no multiples of 64 / 8, one and several workgroups
SIZES = [(1, 1), (2, 1), (63, 7), (65, 9), (129, 17), (130, 16), (256, 64)]
CAMS = {
    "R": dict(eye=(0, 0, 0), target=(0, 0, -1)),          # the reference camera
    "A": dict(eye=(0, 0, 3), target=(0, 0, -1)),          # suzanne from outside
    "B": dict(eye=(0.4, 0.2, 2.6), target=(0, 0, 0)),
}
PLAIN_ENV = dict(RWR_FUSED_SETUP="0", RWR_AUTO_BVH_FACE_PX="0")


@contextlib.contextmanager
def _pair(rwr, model, size, n_slots=1, env=PLAIN_ENV):
    """(plane on, plane off): two fresh contexts that differ in RWR_RAY_PLANE alone (the knobs are read at creation)."""
    mp = pytest.MonkeyPatch()
    ctxs = []
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        for v in ("1", "0"):
            mp.setenv("RWR_RAY_PLANE", v)
            ctxs.append(rwr.Context(0))
        mp.undo()
        for c in ctxs:
            c.upload_model(model)
            c.set_spheres(rwr.make_spheres())
            c.resize(*size)
            c.set_frames_in_flight(n_slots)
        yield ctxs
    finally:
        mp.undo()
        for c in ctxs:
            c.close()


class _Run:
    """Renders every frame in both contexts, compares all their planes, and keeps the model's counts beside the contexts' own."""

    def __init__(self, rwr, on, off, n_slots, size):
        self.rwr, self.on, self.off, self.n, self.size = rwr, on, off, n_slots, size
        self.keys = [None] * n_slots     # per slot: the key of its last frame that could use a plane
        self.built = [False] * n_slots   # ... and whether the slot's plane holds that key's directions
        self.cur = 0                     # the library takes slot (cur + 1) % n for the next frame, starting from 0
        self.builds = self.served = 0
        self.frames = []

    def resized(self, w, h):
        for c in (self.on, self.off):
            c.resize(w, h)
        self.size = (w, h)
        self.keys = [None] * self.n
        self.built = [False] * self.n

    def frame(self, cam, flags=0, spp=1, bounces=0, rows=None, strips=None, usable=True):
        """usable: the frame can use a plane (False: a path-traced frame, or one the default rules fuse)."""
        rwr = self.rwr
        w, h = self.size
        cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(aspect=w / h, **CAMS[cam]))
        params = rwr.make_params(spp=spp, max_bounces=bounces, flags=flags)
        aux = bool(flags & rwr.FLAG_AUX_OUTPUTS)
        got = []
        for c in (self.on, self.off):
            c.render(cam_inv, params, rows=rows, strips=strips)
            got.append(c.readback(aux=aux))
        assert set(got[0]) == ({"color", "depth", "obj_id", "hit_t", "color_f32"} if aux else {"color", "depth"})
        for k in got[0]:
            assert np.array_equal(got[0][k].view(np.uint8), got[1][k].view(np.uint8)), (len(self.frames), cam, self.size, k)
        # the model
        self.cur = (self.cur + 1) % self.n
        if usable:
            key = (cam, self.size, rows, strips)
            if self.keys[self.cur] == key:
                if not self.built[self.cur]:
                    self.built[self.cur] = True
                    self.builds += 1
                self.served += 1
            else:
                self.keys[self.cur] = key
                self.built[self.cur] = False
        assert self.on.ray_plane_stats() == (self.builds, self.served), (len(self.frames), cam, self.size)
        assert self.off.ray_plane_stats() == (0, 0)
        self.frames.append(got[0])
        return got[0]


def _differ(a, b):
    return not np.array_equal(a["color"], b["color"])


@pytest.mark.parametrize("n_slots", [1, 2, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_six_frames_at_one_camera(rwr, suzanne, size, n_slots):
    """The reference camera, both spheres: every slot computes once, builds once and loads from then on — the plain form for
    six frames, then the form with aux planes for six more (same key: all of them load)."""
    with _pair(rwr, suzanne, size, n_slots) as (on, off):
        run = _Run(rwr, on, off, n_slots, size)
        for _ in range(6):
            run.frame("R")
        assert (run.builds, run.served) == (n_slots, 6 - n_slots)
        for _ in range(6):
            run.frame("R", rwr.FLAG_AUX_OUTPUTS)
        assert (run.builds, run.served) == (n_slots, 12 - n_slots)
        assert not _differ(run.frames[0], run.frames[5]) and not _differ(run.frames[0], run.frames[11])


@pytest.mark.parametrize("n_slots", [1, 2, 3])
@pytest.mark.parametrize("seq", ["AAABBBAAA", "ABABABAB"])
@pytest.mark.parametrize("size", [(65, 9), (256, 64)], ids=lambda s: "%dx%d" % s)
def test_camera_sequences(rwr, suzanne, size, seq, n_slots):
    """suzanne from eye (0, 0, 3) and from a second pose.  A camera that moves every frame builds nothing on one slot; on two
    slots A B A B ... leaves each slot with a camera of its own, at rest."""
    aux = rwr.FLAG_AUX_OUTPUTS
    with _pair(rwr, suzanne, size, n_slots) as (on, off):
        run = _Run(rwr, on, off, n_slots, size)
        for i, cam in enumerate(seq):
            run.frame(cam, aux if i % 2 else 0)
        assert _differ(run.frames[0], run.frames[seq.index("B")])
        want = {("AAABBBAAA", 1): (3, 6), ("AAABBBAAA", 2): (3, 3), ("AAABBBAAA", 3): (0, 0),
                ("ABABABAB", 1): (0, 0), ("ABABABAB", 2): (2, 6), ("ABABABAB", 3): (0, 0)}[(seq, n_slots)]
        assert (run.builds, run.served) == want


@pytest.mark.parametrize("n_slots", [1, 2])
def test_scene_changes_keep_the_plane(rwr, suzanne, cube, n_slots):
    """Other spheres and another mesh at a fixed camera: the frames change, the directions do not — no new build."""
    size = (130, 16)
    with _pair(rwr, suzanne, size, n_slots) as (on, off):
        run = _Run(rwr, on, off, n_slots, size)
        for _ in range(2 * n_slots + 1):
            run.frame("A")
        assert (run.builds, run.served) == (n_slots, n_slots + 1)
        for c in (on, off):
            c.set_spheres(rwr.make_spheres([((0.5, 0.3, 1.5), 0.3), ((-0.6, -0.2, 1.0), 0.25)]))
        spheres = run.frame("A", rwr.FLAG_AUX_OUTPUTS)
        assert _differ(run.frames[0], spheres) and (spheres["obj_id"] <= -2).any()
        for c in (on, off):
            c.upload_model(cube)          # 428 faces: the binned frame
        other = run.frame("A", rwr.FLAG_AUX_OUTPUTS)
        assert _differ(spheres, other)
        run.frame("A")
        for c in (on, off):
            c.upload_model(suzanne)
        assert not _differ(spheres, run.frame("A"))
        assert (run.builds, run.served) == (n_slots, n_slots + 5)


@pytest.mark.parametrize("size", [(65, 9), (129, 17), (256, 64)], ids=lambda s: "%dx%d" % s)
def test_cube_binned(rwr, cube, size):
    """cube.obj (428 faces: per-bin face lists) from the reference camera and from outside, on two slots."""
    with _pair(rwr, cube, size, 2) as (on, off):
        run = _Run(rwr, on, off, 2, size)
        for cam in "RRRRRAAAAA":
            run.frame(cam, rwr.FLAG_AUX_OUTPUTS if cam == "A" else 0)
        assert (run.builds, run.served) == (4, 6)
        assert (run.frames[-1]["obj_id"] >= 0).any()


def test_a_sphere_wins_pixels(rwr, suzanne):
    size = (256, 64)
    with _pair(rwr, suzanne, size) as (on, off):
        for c in (on, off):
            c.set_spheres(rwr.make_spheres([((0.5, 0.3, 1.5), 0.3), ((0.4, 0.4, -3.0), 0.4)]))
        run = _Run(rwr, on, off, 1, size)
        for _ in range(3):
            got = run.frame("A", rwr.FLAG_AUX_OUTPUTS)
        assert (run.builds, run.served) == (1, 2)
        assert (got["obj_id"] <= -2).sum() > 50 and (got["obj_id"] >= 0).sum() > 50


def test_resize_and_back(rwr, suzanne):
    """rwr_resize clears the slots' keys: each size computes and builds again, also the one it comes back to."""
    size = (129, 17)
    with _pair(rwr, suzanne, size, 2) as (on, off):
        run = _Run(rwr, on, off, 2, size)
        for _ in range(5):
            run.frame("A")
        first = run.frames[-1]
        run.resized(256, 64)
        for _ in range(5):
            run.frame("A", rwr.FLAG_AUX_OUTPUTS)
        run.resized(*size)
        for _ in range(5):
            run.frame("A")
        assert not _differ(first, run.frames[-1])
        assert (run.builds, run.served) == (6, 9)


@pytest.mark.parametrize("n_slots", [1, 2])
def test_rows_and_strips(rwr, suzanne, n_slots):
    """The whole frame, rows [8, 16) of its 24, strips 1, 4, ... of its three, the whole frame again: the rows place the grid's
    workgroups, so each is a key of its own (and a plane laid out for its own grid)."""
    size = (130, 24)
    aux = rwr.FLAG_AUX_OUTPUTS
    with _pair(rwr, suzanne, size, n_slots) as (on, off):
        run = _Run(rwr, on, off, n_slots, size)
        reps = 2 * n_slots + 1
        for _ in range(reps):
            whole = run.frame("A", aux)
        for _ in range(reps):
            band = run.frame("A", aux, rows=(8, 16))
        assert np.array_equal(band["color"][8:16], whole["color"][8:16]) and np.array_equal(band["hit_t"][8:16], whole["hit_t"][8:16])
        for _ in range(reps):
            strip = run.frame("A", aux, strips=(1, 3))
        assert np.array_equal(strip["color"][8:16], whole["color"][8:16]) and np.array_equal(strip["depth"][8:16], whole["depth"][8:16])
        for _ in range(reps):
            again = run.frame("A", aux)
        assert not _differ(whole, again) and np.array_equal(whole["depth"], again["depth"])
        assert (run.builds, run.served) == (4 * n_slots, 4 * n_slots + 4)


def test_aux_then_plain(rwr, suzanne):
    """The aux planes are not part of the key: the two forms of the loading kernel share a slot's plane."""
    size = (129, 17)
    with _pair(rwr, suzanne, size) as (on, off):
        run = _Run(rwr, on, off, 1, size)
        for flags in (rwr.FLAG_AUX_OUTPUTS, 0, rwr.FLAG_AUX_OUTPUTS, 0):
            run.frame("A", flags)
        assert (run.builds, run.served) == (1, 3)
        assert not _differ(run.frames[0], run.frames[3]) and np.array_equal(run.frames[0]["depth"], run.frames[3]["depth"])


def test_path_traced_frame_between(rwr, suzanne):
    """A frame of the wavefront integrator uses no plane and leaves the slot's alone."""
    size = (130, 16)
    with _pair(rwr, suzanne, size) as (on, off):
        run = _Run(rwr, on, off, 1, size)
        run.frame("A")
        run.frame("A")
        wf = run.frame("A", spp=4, bounces=1, usable=False)
        back = run.frame("A")
        assert _differ(wf, back) and not _differ(run.frames[1], back)
        run.frame("A", spp=2, usable=False)
        run.frame("B")
        run.frame("A", spp=2, usable=False)
        run.frame("B")
        assert (run.builds, run.served) == (2, 3)


def test_default_rules_fuse_small_frames(rwr, suzanne):
    """With the default rules a small plain frame with frames in flight is ONE fused launch, which computes its rays: no frame
    loads from a plane, none is built.  A frame with aux planes takes the two launches, and its slot's key."""
    size = (256, 64)
    with _pair(rwr, suzanne, size, 2, env={}) as (on, off):
        run = _Run(rwr, on, off, 2, size)
        for _ in range(6):
            run.frame("A", usable=False)
        assert (run.builds, run.served) == (0, 0)
        for flags, usable in ((rwr.FLAG_AUX_OUTPUTS, True), (0, False), (rwr.FLAG_AUX_OUTPUTS, True), (0, False), (rwr.FLAG_AUX_OUTPUTS, True)):
            run.frame("A", flags, usable=usable)   # slots 1 0 1 0 1: slot 1 computes, builds, loads
        assert (run.builds, run.served) == (1, 2)


@pytest.mark.parametrize("size", [(63, 7), (65, 9), (129, 17)], ids=lambda s: "%dx%d" % s)
def test_rays_outside_the_short_normalisation(rwr, orc, suzanne, size):
    """The ray function normalises with a short division when every ray of the wave has all three components in
    [2^-40, 2^40], and with the compiler's otherwise (pixel_pair_ray_dir_tab); k_ray_plane takes the same turn.  At an odd
    width the centre column's x_nds is exactly 0, and for a camera on the z axis looking along it the ray's x component with it:
    the waves that hold that column leave the short form.  The CPU oracle's pixelToRay confirms that these cameras really have
    such rays at these sizes."""
    w, h = size
    for cam in ("R", "A"):
        cam_inv = orc.camera_build_inv_uniform(orc.make_camera(aspect=w / h, **CAMS[cam]))
        _, d, _ = orc.pixel_to_ray(cam_inv, orc.make_screen(w, h), (w - 1) // 2, h // 2)
        assert d[0] == 0.0 and d[2] != 0.0, (cam, d)
    with _pair(rwr, suzanne, size, 2) as (on, off):
        run = _Run(rwr, on, off, 2, size)
        for cam in "RRRRRRAAAAAA":
            run.frame(cam, rwr.FLAG_AUX_OUTPUTS)
        assert (run.builds, run.served) == (4, 8)
