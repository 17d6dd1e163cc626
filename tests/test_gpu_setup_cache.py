"""A frame slot keeps its per-frame records (k_frame_setup: culling records, ray tables, per-tile face sets) while camera,
screen, the call's rows and the scene stand still, and a frame that finds them made launches no setup (frame_records.cpp
launch_records).  Every sequence here is rendered in two contexts, the cache on and RWR_SETUP_CACHE=0: each frame must be the same
bytes in both, and rwr_frame_setup_launches must show exactly the hits and misses the sequence implies.

The expected count comes from a model of what the cache is specified to do, not from the library: frames take the slots in turn;
a slot remembers the key its records were made from; a frame launches the setup unless its key is the slot's.  The key, as far as
these tests vary it: the scene's generation, the camera, the screen, the rows, and whether the launch makes per-tile face sets (the
two-pixel frame kernel of an unbinned, culled scene).  Launches of the wavefront integrator carry per-frame clears and are always
made; the fused frame kernel makes the records itself (no setup launch) and a graph replays its own setup: both leave the slot
without a key.

320x184: 5 x 23 workgroups of the frame kernel, more than one 4x4 tile-list region, a clipped last strip."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 320, 184
EYES = {"A": (0.2, 0.1, 2.4), "B": (-0.3, 0.2, 2.8), "C": (0.0, -0.25, 3.2)}


def _cam(rwr, name, w=W, h=H):
    return rwr.camera_build_inv_uniform(rwr.make_camera(eye=EYES[name], target=(0, 0, 0), aspect=w / h))


@contextlib.contextmanager
def _pair(rwr, model, n_slots=1, **env):
    """(cache on, cache off): two fresh contexts that differ in RWR_SETUP_CACHE alone (the knobs are read at creation)."""
    mp = pytest.MonkeyPatch()
    ctxs = []
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        for v in ("1", "0"):
            mp.setenv("RWR_SETUP_CACHE", v)
            ctxs.append(rwr.Context(0))
        mp.undo()
        for c in ctxs:
            c.upload_model(model)
            c.set_spheres(rwr.make_spheres())
            c.resize(W, H)
            c.set_frames_in_flight(n_slots)
        yield ctxs
    finally:
        mp.undo()
        for c in ctxs:
            c.close()


class _Run:
    """Renders every frame in both contexts, compares them, and keeps the model's launch counts beside the contexts' own."""

    def __init__(self, rwr, on, off, n_slots, lists):
        self.rwr, self.on, self.off, self.n = rwr, on, off, n_slots
        self.lists = lists          # the default frame of this scene and context makes per-tile face sets
        self.keys = [None] * n_slots
        self.cur = 0                # the library takes slot (cur + 1) % n for the next frame, starting from 0
        self.generation = 0
        self.size = (W, H)
        self.want_on = self.want_off = 0
        self.frames = []

    def scene_changed(self):
        self.generation += 1

    def resized(self, w, h):
        self.size = (w, h)

    def frame(self, cam_name, flags=0, spp=1, bounces=0, rows=None, strips=None, kind="setup", lists=None):
        """kind: "setup" (k_frame_setup, cached), "always" (wavefront: always launched), "fused" (no setup launch), "graph"."""
        rwr = self.rwr
        w, h = self.size
        cam = _cam(rwr, cam_name, w, h)
        params = rwr.make_params(spp=spp, max_bounces=bounces, flags=flags)
        aux = bool(flags & rwr.FLAG_AUX_OUTPUTS)
        got = []
        for c in (self.on, self.off):
            c.render(cam, params, rows=rows, strips=strips)
            got.append(c.readback(aux=aux))
        for k in got[0]:
            assert np.array_equal(got[0][k].view(np.uint8), got[1][k].view(np.uint8)), (len(self.frames), cam_name, kind, k)
        # the model
        self.cur = (self.cur + 1) % self.n
        lists = self.lists if lists is None else lists
        key = (self.generation, cam_name, self.size, rows, strips, lists and kind == "setup", kind == "always")
        if kind == "fused":
            self.keys[self.cur] = None
        elif kind == "graph":
            self.keys[self.cur] = None
            self.want_on += 1
            self.want_off += 1
        else:
            if kind == "always" or self.keys[self.cur] != key:
                self.want_on += 1
            self.keys[self.cur] = key
            self.want_off += 1
        have = (self.on.frame_setup_launches(), self.off.frame_setup_launches())
        assert have == (self.want_on, self.want_off), (len(self.frames), cam_name, kind, have)
        self.frames.append(got[0])
        return got[0]


def _differ(a, b):
    return not np.array_equal(a["color"], b["color"])


@pytest.fixture(params=["suzanne", "cube"])
def scene(request, suzanne, cube):
    """suzanne_lowpoly.obj: 111 faces, unbinned, per-tile face sets; cube.obj: 428 faces, binned (never fused, no sets)."""
    return request.param, {"suzanne": suzanne, "cube": cube}[request.param]


def _flags(rwr, name, n_slots):
    # suzanne's plain frame with frames in flight is small enough for the fused launch, which has no setup to cache: with
    # aux planes it takes two launches (and the planes are compared as well)
    return rwr.FLAG_AUX_OUTPUTS if name == "suzanne" and n_slots > 1 else 0


@pytest.mark.parametrize("n_slots", [1, 2, 3])
def test_still_camera_then_change_and_return(rwr, scene, n_slots):
    name, model = scene
    with _pair(rwr, model, n_slots) as (on, off):
        run = _Run(rwr, on, off, n_slots, lists=name == "suzanne")
        for cam in "AAABA":
            run.frame(cam, _flags(rwr, name, n_slots))
        assert _differ(run.frames[2], run.frames[3]) and not _differ(run.frames[2], run.frames[4])
        # one slot: A misses, A A hit, B misses, A misses.  Two: slot 1 sees A A A (one miss), slot 0 sees A B (two).
        # Three: slot 1 sees A B (two), slot 2 sees A A (one), slot 0 sees A (one).
        assert run.want_on == {1: 3, 2: 3, 3: 4}[n_slots] and run.want_off == 5


def test_two_cameras_alive_on_two_slots(rwr, scene):
    name, model = scene
    with _pair(rwr, model, 2) as (on, off):
        run = _Run(rwr, on, off, 2, lists=name == "suzanne")
        for cam in "ABABABAB":
            run.frame(cam, _flags(rwr, name, 2))
        assert _differ(run.frames[6], run.frames[7])
        assert run.want_on == 2 and run.want_off == 8   # each slot misses once and then always hits, with its own key


def test_three_cameras_on_two_slots_always_miss(rwr, scene):
    name, model = scene
    with _pair(rwr, model, 2) as (on, off):
        run = _Run(rwr, on, off, 2, lists=name == "suzanne")
        for cam in "ABCABC":
            run.frame(cam, _flags(rwr, name, 2))
        assert run.want_on == 6 and run.want_off == 6


def test_plain_frames_in_flight_are_fused_and_leave_no_key(rwr, suzanne):
    """suzanne's plain 320x184 frame on two slots takes the fused launch (no k_frame_setup); an aux frame behind it on the same
    slot cannot rely on records from before."""
    with _pair(rwr, suzanne, 2) as (on, off):
        run = _Run(rwr, on, off, 2, lists=True)
        aux = rwr.FLAG_AUX_OUTPUTS
        for cam, flags, kind in (("A", aux, "setup"), ("A", aux, "setup"), ("A", 0, "fused"), ("A", aux, "setup"), ("A", aux, "setup")):
            run.frame(cam, flags, kind=kind)   # slots 1 0 1 0 1: the last frame's slot was written by the fused frame
        assert run.want_on == 3 and run.want_off == 4


def test_scene_and_screen_changes_miss_once(rwr, suzanne, cube):
    with _pair(rwr, suzanne) as (on, off):
        run = _Run(rwr, on, off, 1, lists=True)
        both = (on, off)
        first = run.frame("A")
        run.frame("A")
        assert run.want_on == 1
        # other spheres (the records do not depend on them; the frame does)
        for c in both:
            c.set_spheres(rwr.make_spheres([((-0.8, 0.6, 0.0), 0.3), ((0.9, -0.5, 0.2), 0.25)]))
        run.scene_changed()
        spheres = run.frame("A")
        assert _differ(first, spheres)
        run.frame("A")
        assert run.want_on == 2
        # the other mesh and back
        for c in both:
            c.upload_model(cube)
        run.scene_changed()
        other = run.frame("A", lists=False)
        assert _differ(spheres, other)
        run.frame("A", lists=False)
        for c in both:
            c.upload_model(suzanne)
        run.scene_changed()
        back = run.frame("A")
        assert not _differ(spheres, back)
        run.frame("A")
        assert run.want_on == 4
        # instances (4 x 111 faces: binned) and back
        for c in both:
            c.set_instances(rwr.make_instance_grid(2, 1.5))
        run.scene_changed()
        inst = run.frame("A", lists=False)
        assert _differ(back, inst)
        run.frame("A", lists=False)
        for c in both:
            c.set_instances(None)
        run.scene_changed()
        assert not _differ(back, run.frame("A"))
        run.frame("A")
        assert run.want_on == 6
        # another screen and back
        for c in both:
            c.resize(256, 256)
        run.resized(256, 256)
        run.frame("A")
        run.frame("A")
        for c in both:
            c.resize(W, H)
        run.resized(W, H)
        assert not _differ(back, run.frame("A"))
        run.frame("A")
        assert run.want_on == 8 and run.want_off == 16


def test_launch_geometry_changes_miss(rwr, scene):
    name, model = scene
    with _pair(rwr, model) as (on, off):
        run = _Run(rwr, on, off, 1, lists=name == "suzanne")
        whole = run.frame("A")
        band = run.frame("A", rows=(40, 133))
        assert np.array_equal(band["color"][40:133], whole["color"][40:133])
        run.frame("A", rows=(40, 133))
        run.frame("A")
        assert run.want_on == 3
        for r in (0, 1, 0, 0):
            got = run.frame("A", strips=(r, 2))
            rows = [y for s in range(r, (H + 7) // 8, 2) for y in range(8 * s, min(H, 8 * s + 8))]
            assert np.array_equal(got["color"][rows], whole["color"][rows]) and np.array_equal(got["depth"][rows], whole["depth"][rows])
        assert run.want_on == 6 and run.want_off == 8


def _frame_paths(rwr, run):
    """At one camera on one slot: default, NO_CULL, one pixel per lane, the BVH kernel, aux planes, default again.  The launches of
    the three kernels in the middle make no face sets, so they share one key."""
    default = run.frame("A")
    for flags in (rwr.FLAG_NO_CULL, rwr.FLAG_ONE_PIXEL_PER_LANE, rwr.FLAG_USE_BVH):
        run.frame("A", flags, lists=False)
    assert not _differ(default, run.frame("A", rwr.FLAG_AUX_OUTPUTS))
    assert not _differ(default, run.frame("A"))


def test_frame_paths_with_tile_lists(rwr, suzanne):
    with _pair(rwr, suzanne) as (on, off):
        run = _Run(rwr, on, off, 1, lists=True)
        _frame_paths(rwr, run)
        assert run.want_on == 3 and run.want_off == 6


def test_frame_paths_without_tile_lists(rwr, suzanne):
    with _pair(rwr, suzanne, RWR_TILE_LISTS="0") as (on, off):
        run = _Run(rwr, on, off, 1, lists=False)
        _frame_paths(rwr, run)
        assert run.want_on == 1 and run.want_off == 6


def test_frame_paths_binned(rwr, cube):
    with _pair(rwr, cube) as (on, off):
        run = _Run(rwr, on, off, 1, lists=False)
        _frame_paths(rwr, run)
        assert run.want_on == 1 and run.want_off == 6


@pytest.mark.parametrize("knob,kind", [("RWR_FUSED_SETUP", "fused"), ("RWR_FRAME_GRAPH", "graph")])
def test_fused_and_graph_frames_between_plain_ones(rwr, suzanne, knob, kind):
    """With the knob every plain frame is one fused launch / one graph launch; a frame with aux planes takes the two launches.
    Both forms write the slot's records, so the frame behind them makes them again."""
    with _pair(rwr, suzanne, **{knob: "1"}) as (on, off):
        run = _Run(rwr, on, off, 1, lists=True)
        aux = rwr.FLAG_AUX_OUTPUTS
        first = run.frame("A", kind=kind)
        for flags, k in ((aux, "setup"), (0, kind), (aux, "setup"), (aux, "setup"), (0, kind), (0, kind)):
            assert not _differ(first, run.frame("A", flags, kind=k))
        # setup launches: none by a fused frame, one per graph launch; of the three aux frames the last one hits
        assert (run.want_on, run.want_off) == {"fused": (2, 3), "graph": (6, 7)}[kind]


def test_wavefront_and_back(rwr, suzanne):
    """The integrator's launches also clear its per-tile ray counts and live-tile count: they are made every frame, and the sums
    (here the resolved colour, and the accumulation's running mean) are those of the context without the cache."""
    with _pair(rwr, suzanne) as (on, off):
        run = _Run(rwr, on, off, 1, lists=True)
        acc = rwr.FLAG_ACCUMULATE
        wf = run.frame("A", spp=4, bounces=1, kind="always")
        ref = run.frame("A")
        assert _differ(wf, ref)
        assert not _differ(wf, run.frame("A", spp=4, bounces=1, kind="always"))
        a1 = run.frame("A", acc, spp=2, bounces=1, kind="always")
        a2 = run.frame("A", acc, spp=2, bounces=1, kind="always")
        assert on.accum_samples() == off.accum_samples() == 4 and _differ(a1, a2)
        assert not _differ(ref, run.frame("A"))
        assert not _differ(ref, run.frame("A"))
        assert run.want_on == 6 and run.want_off == 7
