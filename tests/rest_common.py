"""Oracle parity for frames served from a slot's kept state (test infrastructure): a frame slot keeps k_frame_setup's records
while their key stands still (frame_records.cpp launch_records) and, from the third frame at rest, the two-pixel frame kernel loads its
ray directions from a plane the slot keeps (ray_plane_step).  tests/test_gpu_setup_cache.py and tests/test_gpu_ray_plane.py
compare that state with the library itself (on against off); here every frame served from it is compared with the CPU oracle,
at the project's bar: obj_id, hit_t and depth bit for bit, color_f32 within 1e-4.  Used by tests/test_gpu_rest_parity.py (a
fixed list of cases) and tools/fuzz_parity.py --rest (as long as you like).

Slots: the model of what a context's slots are specified to do, written from the specification (include/rwr_hip.h
rwr_frame_setup_launches / rwr_ray_plane_stats, and the docstrings of the _Run classes of the two tests above), not from the
library.  Frames take slots (cur + 1) % n.  A setup launch is made unless the slot's records key — scene generation, camera
bytes, screen, the call's rows, whether the launch makes per-tile face sets, whether it carries the integrator's clears — is the
call's; the integrator's launches are always made.  A frame that can use a plane (the reference frame in the two-pixel kernel's
culled two-launch form, a band that is not empty) has the plane key (camera bytes, screen, rows): it loads when the slot's plane
was built for that key, builds and loads when the slot's last usable frame had the key, and computes otherwise; other frames
pass the slot's plane by.  rwr_resize clears the plane key of every slot and leaves the records keys (the screen is part of
them); rwr_ctx_set_frames_in_flight(n) keeps slots below n as they are, gives up the others with everything they held, and
moves the turn to slot 0 when the current slot is gone.  The model holds for contexts created with RWR_FUSED_SETUP=0 and
RWR_AUTO_BVH_FACE_PX=0 (every whole reference frame of a non-empty scene then takes the two launches of the two-pixel kernel).

Tracked: a context with that model beside it, and a copy of what every slot's targets hold, so that the rows a band or a strip
set did not render can be checked against what the slot's previous frame left there."""
import contextlib
import os

import numpy as np

import fuzz_common

MODEL_ENV = dict(RWR_FUSED_SETUP="0", RWR_AUTO_BVH_FACE_PX="0")
STRIP_ROWS = 8            # include/rwr_hip.h RWR_STRIP_ROWS
FACE_SET_MAX_FACES = 256  # per-tile face sets / one 256-wide batch: scenes above it are binned (RWR_BIN_MIN_FACES' default)
MAX_SLOTS = 3
FLAG_AUX, FLAG_NO_CULL, FLAG_USE_BVH, FLAG_ORTHO_RAYS, FLAG_ONE_PIXEL = 1, 2, 4, 1 << 3, 1 << 17
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")


# ------------------------------------------------------------------------------------------------ calls --
class Call:
    """One render call: the camera uniform, rows = (begin, end) or strips = (first, stride) or neither, flags besides
    FLAG_AUX_OUTPUTS, the integrator's parameters."""

    def __init__(self, cam, rows=None, strips=None, flags=0, spp=1, bounces=0, seed=0):
        self.cam, self.rows, self.strips, self.flags, self.spp, self.bounces, self.seed = cam, rows, strips, flags, spp, bounces, seed

    def band(self, h):
        """(row_begin, row_end, row_pitch) as rwr_render / rwr_render_rows / rwr_render_strips document them."""
        if self.strips is not None:
            return min(STRIP_ROWS * self.strips[0], h), h, STRIP_ROWS * self.strips[1]
        if self.rows is not None:
            return self.rows[0], self.rows[1], STRIP_ROWS
        return 0, h, STRIP_ROWS

    def rendered_rows(self, h):
        b, e, pitch = self.band(h)
        return np.array([y for s in range(b, e, pitch) for y in range(s, min(s + STRIP_ROWS, e))], dtype=np.int64)


def compare(got, want, rows, tag, single_triangles=False):
    """The project's bar on the rows the call rendered; returns the worst colour difference."""
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k][rows].view(np.uint32), want[k][rows].view(np.uint32)), tag + (k,)
    g, w = got["color_f32"][rows], want["color_f32"][rows]
    if g.size == 0:
        return 0.0
    diff = np.abs(g - w)
    if single_triangles:
        # fuzz_common.run's rule for the single-triangle shading (x^32 of an un-normalised dot product): relative above 1
        big = np.abs(w) > 1.0
        with np.errstate(invalid="ignore"):
            rel = np.where(g == w, 0.0, diff / np.maximum(np.abs(w), 1.0))
        assert float(rel[big].max() if big.any() else 0.0) <= 5e-3, tag + ("color_f32 rel",)
        diff = diff[~big]
    d = float(diff.max()) if diff.size else 0.0
    assert d <= 1e-4, tag + ("color_f32", d)
    return d


# ------------------------------------------------------------------------------------------------ the model --
class Slots:
    def __init__(self, n=1, plane=True):
        self.n, self.cur, self.plane = n, 0, plane
        self.rec = [None] * MAX_SLOTS      # records key per slot
        self.pkey = [None] * MAX_SLOTS     # plane key of the slot's last frame that could use a plane
        self.built = [False] * MAX_SLOTS   # the slot's plane holds that key's directions
        self.generation = 0
        self.launches = self.builds = self.served = 0

    def scene_changed(self):
        self.generation += 1

    def resized(self):
        for i in range(self.n):
            self.pkey[i], self.built[i] = None, False

    def set_slots(self, n):
        for i in range(n, MAX_SLOTS):
            self.rec[i], self.pkey[i], self.built[i] = None, None, False
        if self.cur >= n:
            self.cur = 0
        self.n = n

    def frame(self, cam_bytes, size, band, kind, n_faces):
        """kind: "two_pixel" (the reference frame in the two-pixel kernel's culled form), "other" (NO_CULL, one pixel per lane,
        the BVH kernel, single-triangle passes / orthographic rays: the setup without face sets, no plane) or "wavefront".
        Returns (slot, a setup launch is made, "load" / "build" / "compute" / None)."""
        self.cur = (self.cur + 1) % self.n
        s = self.cur
        empty = band[1] <= band[0]
        lists = kind == "two_pixel" and 0 < n_faces <= FACE_SET_MAX_FACES and not empty
        key = (self.generation, cam_bytes, size, band, lists, kind == "wavefront")
        launched = kind == "wavefront" or self.rec[s] != key
        self.rec[s] = key
        self.launches += launched
        action = None
        if kind == "two_pixel" and self.plane and not empty:
            pk = (cam_bytes, size, band)
            if self.pkey[s] == pk:
                action = "load" if self.built[s] else "build"
                self.builds += not self.built[s]
                self.built[s] = True
                self.served += 1
            else:
                self.pkey[s], self.built[s], action = pk, False, "compute"
        return s, bool(launched), action


# ------------------------------------------------------------------------------------------------ a tracked context --
class Tracked:
    """A context, the model of its slots (modelled=False: none — the default rules fuse and choose kernels by rules the model
    does not hold; the counters then need only never fall, and stay zero with the plane off) and what its slots' targets hold."""

    def __init__(self, r, ctx, modelled=True, plane=True):
        self.r, self.ctx, self.modelled, self.plane = r, ctx, modelled, plane
        self.slots = Slots(1, plane)
        self.size = (0, 0)
        self.n_faces = self.n_instances = self.n_triangles = 0
        self.held = [None] * MAX_SLOTS   # per slot: plane name -> what it holds, for the planes that are known
        self.aux_seen = [False] * MAX_SLOTS
        self.counters = (0, 0, 0)
        self.frames = 0
        self.worst = 0.0

    @property
    def n_slots(self):
        return self.slots.n

    def _zeros(self, aux):
        w, h = self.size
        z = {"color": np.zeros((h, w, 4), np.uint8), "depth": np.zeros((h, w), np.float32)}
        if aux:   # planes a slot has never held start zeroed
            z.update(color_f32=np.zeros((h, w, 4), np.float32), obj_id=np.zeros((h, w), np.int32), hit_t=np.zeros((h, w), np.float32))
        return z

    def upload(self, model):
        self.ctx.upload_model(model)
        self.n_faces = len(model["faces"])
        self.slots.scene_changed()

    def set_spheres(self, spheres):
        self.ctx.set_spheres(spheres)
        self.slots.scene_changed()

    def set_instances(self, inst):
        self.ctx.set_instances(inst)
        self.n_instances = 0 if inst is None else len(inst)
        self.slots.scene_changed()

    def set_triangles(self, tris):
        self.ctx.set_triangles(tris)
        self.n_triangles = len(tris)
        self.slots.scene_changed()

    def resize(self, w, h):
        self.ctx.resize(w, h)
        self.size = (w, h)
        self.slots.resized()
        # the targets are cleared; aux planes a slot held before keep bytes of another layout (not known), others start zeroed
        for i in range(self.n_slots):
            self.held[i] = self._zeros(aux=not self.aux_seen[i])

    def set_slots(self, n):
        self.ctx.set_frames_in_flight(n)
        self.slots.set_slots(n)
        for i in range(MAX_SLOTS):
            if i >= n:
                self.held[i], self.aux_seen[i] = None, False
            elif self.held[i] is None and self.size[0]:
                self.held[i] = self._zeros(aux=True)   # a slot taken into use: cleared targets, no planes yet

    def _kind(self, call):
        if call.spp != 1 or call.bounces != 0:
            return "wavefront"
        if self.n_triangles or call.flags & (FLAG_ORTHO_RAYS | FLAG_NO_CULL | FLAG_USE_BVH | FLAG_ONE_PIXEL):
            return "other"
        return "two_pixel"

    def frame(self, call, want, aux=True, tag=(), rgba8=None):
        """Renders the call, reads the frame back and compares it: with aux planes, all of them with the oracle's frame `want`
        on the rows the call rendered; without, the depth with the oracle's and the RGBA8 with `rgba8` (an aux frame's of the same
        call) where given.  Rows the call did not render must hold what the slot held.  Returns (frame, slot, setup launched,
        plane action); the last three are None without a model."""
        r, ctx = self.r, self.ctx
        w, h = self.size
        tag = tag + (self.frames, (w, h), call.rows, call.strips, call.flags, "aux" if aux else "plain")
        params = r.make_params(spp=call.spp, max_bounces=call.bounces, seed=call.seed, flags=call.flags | (FLAG_AUX if aux else 0))
        ctx.render(call.cam, params, rows=call.rows, strips=call.strips)
        got = ctx.readback(aux=aux)
        self.frames += 1
        kind = self._kind(call)
        slot, launched, action = self.slots.frame(call.cam.tobytes(), (w, h), call.band(h), kind, self.n_faces * max(1, self.n_instances))
        rows = call.rendered_rows(h)
        if aux:
            self.worst = max(self.worst, compare(got, want, rows, tag, single_triangles=kind == "other" and bool(self.n_triangles or call.flags & FLAG_ORTHO_RAYS)))
        else:
            assert np.array_equal(got["depth"][rows].view(np.uint32), want["depth"][rows].view(np.uint32)), tag + ("plain depth",)
            if rgba8 is not None:
                assert np.array_equal(got["color"][rows], rgba8[rows]), tag + ("plain rgba8",)
        # the rows outside
        held = self.held[slot]
        outside = np.setdiff1d(np.arange(h), rows)
        if held is not None and outside.size:
            for k in got:
                if k in held:
                    assert np.array_equal(got[k][outside].view(np.uint8), held[k][outside].view(np.uint8)), tag + ("rows outside", k)
        # the counters (behind the comparison: a wrong frame is reported as one)
        have = (ctx.frame_setup_launches(),) + tuple(ctx.ray_plane_stats())
        if self.modelled:
            assert have == (self.slots.launches, self.slots.builds, self.slots.served), tag + (have, (self.slots.launches, self.slots.builds, self.slots.served), slot, launched, action)
        else:
            assert all(a >= b for a, b in zip(have, self.counters)), tag + (have, self.counters)
            assert self.plane or have[1:] == (0, 0), tag + (have,)
            launched = action = None
        self.counters = have
        new = dict(held or {})
        new.update(got)
        self.held[slot] = new
        self.aux_seen[slot] |= aux
        return got, slot, launched, action


def rest(ctx, n_slots, call, want, frames, tag=(), served=None, loaded=False):
    """The rest sequence on a Tracked context with n_slots frames in flight: the same call `frames` times with FLAG_AUX_OUTPUTS,
    every frame compared with the oracle's single frame `want`, then once more without the flag (RGBA8 as the aux frame's, depth
    bits as the oracle's).  served (default: the context has a model and the call is the two-pixel kernel's, frames >= 2 n + 2):
    every slot's last aux frame must then have been a loading frame on kept records.  A slot's building frame counts as one: it
    fills the plane and loads from it.  With 2 n + 2 frames on three slots, slot 0 computes and builds and is not visited again,
    so its last frame is the building one.  loaded: the slots are at rest at this call already, and EVERY aux frame must be a
    pure load (plane built before, no setup launch); a few frames behind a rest of 2 n + 2 compare such a frame on every slot.
    Returns the last aux frame."""
    assert ctx.n_slots == n_slots
    h = ctx.size[1]
    usable = ctx._kind(call) == "two_pixel" and call.band(h)[1] > call.band(h)[0]
    if served is None:
        served = ctx.modelled and ctx.plane and usable and frames >= 2 * n_slots + 2
    last = {}
    got = None
    for i in range(frames):
        got, slot, launched, action = ctx.frame(call, want, aux=True, tag=tag + ("rest", i))
        last[slot] = (launched, action)
        assert not loaded or (launched, action) == (False, "load"), tag + ("rest", i, slot, launched, action)
    if served:
        assert len(last) == n_slots and all(v[0] is False and v[1] in ("build", "load") for v in last.values()), tag + (last,)
    ctx.frame(call, want, aux=False, tag=tag + ("rest", "plain"), rgba8=None if got is None else got["color"])
    return got


@contextlib.contextmanager
def tracked(r, modelled=True, plane=True, mp=None):
    """A fresh context under the model's environment knobs (modelled) or none (the default rules); plane=False: RWR_RAY_PLANE=0.
    The knobs are read at creation.  mp: a pytest.MonkeyPatch (tests); without one os.environ is changed and restored."""
    env = dict(MODEL_ENV) if modelled else {}
    if not plane:
        env["RWR_RAY_PLANE"] = "0"
    saved = {} if mp is not None else {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if mp is not None:
                mp.setenv(k, v)
            else:
                os.environ[k] = v
        ctx = r.Context(0)
    finally:
        if mp is not None:
            mp.undo()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        yield Tracked(r, ctx, modelled, plane)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the cases --
MESHES = (1, 2, 64, 65, 255, 256, 257, 300, 777, 1500, "suzanne", "cube")
FOVY = ((1.0, 15.0), (15.0, 110.0), (110.0, 175.0))
FORCED_SIZES = {3: (1, 1), 7: (2, 1), 13: (131, None), 22: (200, 41)}   # case index -> (w, h); None: drawn
MAX_WORK = 2e7   # w h n_faces, as fuzz_common.run bounds its frames


def _offset(rng):
    """fuzz_common.run's far=True offsets: up to 1e5 on random axes."""
    axes = rng.random(3) < 0.6
    axes[int(rng.integers(0, 3))] = True
    return np.where(axes, rng.choice([-1.0, 1.0], 3) * 10.0 ** rng.uniform(0.0, 5.0, 3), 0.0)


def draw_cases(orc, ref_loader, meshes, seed, n_cases=40):
    """The fixed list: case i takes mesh MESHES[i % 12] (soups with extents and triangle sizes from the fuzz's lists, the two
    real meshes), a field of view from range (i + i // 12) % 3, a third of the cases (a drawn set) moved by the far offsets;
    eye, target, spheres, size and frames in flight drawn as fuzz_common.run draws them.  meshes: {"suzanne": ..., "cube": ...}."""
    rng = np.random.default_rng(seed)
    tex = meshes["suzanne"]["texture"]
    far_set = set(rng.permutation(n_cases)[: (n_cases + 2) // 3].tolist())
    cases = []
    for i in range(n_cases):
        m = MESHES[i % len(MESHES)]
        if isinstance(m, int):
            model = fuzz_common.soup(ref_loader, rng, m, extent=float(rng.choice([0.5, 2.5, 8.0])), tri_size=float(rng.choice([0.02, 0.05, 0.4, 1.5, 6.0])), tex=tex)
        else:
            model = meshes[m]
        n_faces = len(model["faces"])
        fw, fh = FORCED_SIZES.get(i, (None, None))
        while True:
            w = fw or int(rng.integers(1, 260))
            h = fh or int(rng.integers(1, 150))
            if w * h * n_faces <= MAX_WORK:
                break
        far = i in far_set
        offset = _offset(rng) if far else np.zeros(3)
        if far:
            model = fuzz_common._moved(model, offset)
        lo, hi = FOVY[(i + i // len(MESHES)) % 3]
        cam = orc.make_camera(eye=tuple(rng.uniform(-4, 4, 3) * float(rng.choice([0.1, 1.0, 1.0, 6.0])) + offset), target=tuple(rng.uniform(-1, 1, 3) + offset),
                              aspect=w / h, fovy=float(rng.uniform(lo, hi)))
        spheres = orc.make_spheres([(tuple(rng.uniform(-3, 3, 3) + offset), float(rng.uniform(0.05, 1.5))) for _ in range(int(rng.integers(0, 9)))])
        cases.append(dict(name="case%02d" % i, mesh=m, model=model, spheres=spheres, cam=orc.camera_build_inv_uniform(cam), size=(w, h),
                          n_slots=int(rng.integers(1, 4)), far=far, offset=offset))
    return cases


def oracle_frame(orc, cam, size, spheres, model):
    return orc.render_frame(cam, orc.make_screen(*size), spheres, model)


def shows(frame):
    """(mesh pixels, sphere pixels, other pixels) of an oracle frame: obj_id >= 0 a face, <= -2 a sphere, -1 nothing."""
    ids = frame["obj_id"]
    return int((ids >= 0).sum()), int((ids <= -2).sum()), int((ids == -1).sum())


def case_conditions(cases, frames):
    """The conditions on the list's inputs (counts): cases that show the mesh and something else, cases that show a sphere, far
    cases that show the mesh."""
    both = sum(1 for f in frames if shows(f)[0] > 0 and shows(f)[1] + shows(f)[2] > 0)
    sphere = sum(1 for f in frames if shows(f)[1] > 0)
    far_mesh = sum(1 for c, f in zip(cases, frames) if c["far"] and shows(f)[0] > 0)
    return both, sphere, far_mesh


# ------------------------------------------------------------------------------------------------ the smallest changes --
STEP_SIZE = (131, 43)   # an odd width over two workgroup columns; 43 rows: six strips, the last one clipped


def same_size_mesh(ref_loader, rng, model, extent, tri_size):
    """Another mesh with the face and vertex counts of `model` (its material and texture): a soup's faces over its vertices."""
    n_faces, n_verts = len(model["faces"]), len(model["vertices"])
    s = fuzz_common.soup(ref_loader, rng, n_faces, extent, tri_size, model["texture"])
    verts = np.zeros(n_verts, ref_loader.VERTEX_DTYPE)
    k = min(n_verts, 3 * n_faces)
    verts[:k] = s["vertices"][:k]
    s["vertices"] = verts
    s["faces"]["indices"] %= np.uint32(n_verts)
    s["material"] = model["material"]
    return s


def step_scenes(orc, ref_loader, suzanne, seed=7):
    """The three scenes of the smallest-change steps: a soup below the face-set limit, one above it (binned), suzanne; each with
    the mesh that replaces it (same counts), a resting camera and two sphere sets."""
    rng = np.random.default_rng(seed)
    tex = suzanne["texture"]
    w, h = STEP_SIZE
    out = {}
    for name, n in (("soup65", 65), ("soup300", 300), ("suzanne", None)):
        model = suzanne if n is None else fuzz_common.soup(ref_loader, rng, n, extent=2.5, tri_size=0.4, tex=tex)
        other = same_size_mesh(ref_loader, rng, model, 2.5 if n else 1.0, 0.4)
        eye = (0.3, 0.15, 2.0) if n is None else (0.4, 0.3, 3.5)
        spheres = orc.make_spheres([((0.9, 0.5, 0.3), 0.3), ((-0.8, -0.3, 0.3), 0.25)])
        spheres_b = orc.make_spheres([((-0.8, 0.6, 0.0), 0.3), ((0.9, -0.5, 0.2), 0.25), ((0.0, 0.9, 0.5), 0.2)])
        out[name] = dict(name=name, model=model, other=other, eye=eye, spheres=spheres, spheres_b=spheres_b)
    return out


def resting_cam(orc, scene, size):
    return orc.camera_build_inv_uniform(orc.make_camera(eye=scene["eye"], target=(0, 0, 0), aspect=size[0] / size[1]))


def ulp_cams(cam):
    """3c: the camera with one element moved by one float32 ulp, returned as (projection, origin, column): of the projection
    inverse ([0][0]), of the ray origin, of the inverse view matrix's translation column (column-major [3][0]).  The first
    changes the ray directions (a plane kept from the resting camera would show in hit_t), the second the origin alone.
    pixelToRay multiplies the translation column by w = 0, so the third camera's frame is the resting one's (other bytes all
    the same: both keys must miss); the first two cameras change hit_t."""
    a, b, c = cam.copy(), cam.copy(), cam.copy()
    a["proj_inv"][0][0][0] = np.nextafter(a["proj_inv"][0][0][0], np.float32(np.inf))
    b["origin"][0][0] = np.nextafter(b["origin"][0][0], np.float32(np.inf))
    c["viewmodel_inv"][0][3][0] = np.nextafter(c["viewmodel_inv"][0][3][0], np.float32(np.inf))
    return a, b, c


ULP_KEYS = ("3c proj", "3c origin", "3c column")


def ulp_sphere(spheres):
    """3b: the first sphere's radius moved by one float32 ulp."""
    s = spheres.copy()
    s["radius"][0] = np.nextafter(s["radius"][0], np.float32(np.inf))
    return s


PATH_INSTANCES = ((0.0, (0.0, 0.0, 0.0)), (0.7, (1.2, -0.4, -1.0)))   # rotation about y, translation


def path_instances(r_or_orc):
    inst = np.zeros(len(PATH_INSTANCES), dtype=r_or_orc.INSTANCE_DTYPE)
    for i, (a, t) in enumerate(PATH_INSTANCES):
        c_, s_ = np.float32(np.cos(a)), np.float32(np.sin(a))
        m = np.eye(4, dtype=np.float32)
        m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c_, -s_, s_, c_   # column-major m[col][row]
        m[3, :3] = t
        inst["model"][i] = m
    return inst


SINGLE_TRIANGLES = [((-1.5, -1.0, 0.5), (1.0, -1.2, 0.8), (0.2, 1.4, 1.0)), ((0.5, 0.5, 1.8), (1.6, 0.4, 1.2), (1.0, 1.5, 1.5))]


class Oracle:
    """The oracle's frames of a scene's steps, computed once and shared (by the slot counts, by the default-rule runs)."""

    def __init__(self, orc):
        self.orc, self.frames = orc, {}

    def get(self, key, make):
        if key not in self.frames:
            f = make()
            for a in f.values():
                if a is not None:
                    a.setflags(write=False)
            self.frames[key] = f
        return self.frames[key]


def run_steps(ctx, orc, oracle, scene, n_slots, steps="abcdefgh"):
    """Steps 3a-3h on one long-lived Tracked context, each followed by a rest sequence of its own with every frame compared.
    Returns {step: last aux frame}; the oracle's frames stay in `oracle` (keyed by scene and step) for the conditions on them."""
    name = scene["name"]
    w, h = STEP_SIZE
    frames = 2 * n_slots + 2
    scr = lambda size=STEP_SIZE: orc.make_screen(*size)
    cam = resting_cam(orc, scene, STEP_SIZE)
    model, spheres = scene["model"], scene["spheres"]

    def want_of(key, cam_=None, size=STEP_SIZE, spheres_=None, model_=None):
        return oracle.get((name, key), lambda: orc.render_frame(cam if cam_ is None else cam_, scr(size), spheres if spheres_ is None else spheres_,
                                                                model if model_ is None else model_))

    ctx.upload(model); ctx.set_spheres(spheres); ctx.set_instances(None); ctx.set_triangles(orc.make_triangles())
    ctx.resize(w, h); ctx.set_slots(n_slots)
    base = want_of("base")
    call = Call(cam)
    t = (name, n_slots)
    rest(ctx, n_slots, call, base, frames, t + ("base",))
    if "a" in steps:   # the same-size mesh and back: generation alone tells them apart; the plane stays (no build)
        launches, builds = ctx.slots.launches, ctx.slots.builds
        ctx.upload(scene["other"])
        rest(ctx, n_slots, call, want_of("3a", model_=scene["other"]), frames, t + ("3a",))
        ctx.upload(model)
        rest(ctx, n_slots, call, base, frames, t + ("3a back",))
        assert (ctx.slots.launches, ctx.slots.builds) == (launches + 2 * n_slots, builds)   # records remade on every slot, no build
    if "b" in steps:   # one sphere by one ulp of its radius, then all spheres replaced, and back
        s1 = ulp_sphere(spheres)
        ctx.set_spheres(s1)
        rest(ctx, n_slots, call, want_of("3b ulp", spheres_=s1), frames, t + ("3b ulp",))
        ctx.set_spheres(scene["spheres_b"])
        rest(ctx, n_slots, call, want_of("3b all", spheres_=scene["spheres_b"]), frames, t + ("3b all",))
        ctx.set_spheres(spheres)
        rest(ctx, n_slots, call, base, frames, t + ("3b back",))
    if "c" in steps:   # the camera by one ulp, and back: compute, build, load again each time
        for key, c1 in zip(ULP_KEYS, ulp_cams(cam)):
            builds = ctx.slots.builds
            rest(ctx, n_slots, Call(c1), want_of(key, cam_=c1), frames, t + (key,))
            rest(ctx, n_slots, call, base, frames, t + (key + " back",))
            assert not ctx.modelled or ctx.slots.builds == builds + 2 * n_slots
    if "d" in steps:   # rows and strips; a band from a row that is no multiple of 8
        for key, c1 in (("rows 8:16", Call(cam, rows=(8, 16))), ("strips 1,3", Call(cam, strips=(1, 3))), ("whole", call),
                        ("rows 3:21", Call(cam, rows=(3, 21))), ("strips 2,4", Call(cam, strips=(2, 4))), ("rows 40:43", Call(cam, rows=(40, 43))), ("whole", call)):
            rest(ctx, n_slots, c1, base, frames, t + ("3d " + key,))
    if "e" in steps:   # resize to (w + 1, h) and back, and to the same size again
        wide = (w + 1, h)
        cam_w = resting_cam(orc, scene, wide)
        ctx.resize(*wide)
        rest(ctx, n_slots, Call(cam_w), want_of("3e wide", cam_=cam_w, size=wide), frames, t + ("3e wide",))
        ctx.resize(w, h)
        rest(ctx, n_slots, call, base, frames, t + ("3e back",))
        launches, builds = ctx.slots.launches, ctx.slots.builds
        ctx.resize(w, h)   # the records stand (nothing they are made from changed), the planes do not; the targets are cleared
        rest(ctx, n_slots, call, base, frames, t + ("3e same",))
        assert not ctx.modelled or (ctx.slots.launches, ctx.slots.builds) == (launches, builds + n_slots)
        ctx.resize(w, h)   # ... and a band behind it finds cleared rows outside
        rest(ctx, n_slots, Call(cam, rows=(8, 16)), base, frames, t + ("3e same band",))
        rest(ctx, n_slots, call, base, frames, t + ("3e same whole",))
    if "f" in steps:   # frames in flight 1 -> 3 -> 2 -> 1 and back, the camera at rest throughout
        for n in (1, 3, 2, 1, n_slots):
            ctx.set_slots(n)
            rest(ctx, n, call, base, 2 * n + 2, t + ("3f", n))
            rest(ctx, n, Call(cam, strips=(1, 3)), base, 2, t + ("3f strips", n))
            rest(ctx, n, call, base, n, t + ("3f again", n), served=False)
    if "g" in steps:   # other kernels between frames of the resting call: they share the slot's tables and records
        for flags in (FLAG_NO_CULL, FLAG_ONE_PIXEL, FLAG_USE_BVH):
            for i in range(n_slots + 1):
                ctx.frame(Call(cam, flags=flags), base, tag=t + ("3g", flags, i))
                ctx.frame(call, base, tag=t + ("3g rest", flags, i))
            rest(ctx, n_slots, call, base, frames, t + ("3g after", flags))
        inst = path_instances(orc)
        ctx.set_instances(inst)
        pcall = Call(cam, spp=2, bounces=1, seed=5)
        pwant = oracle.get((name, "3g path"), lambda: orc.render_path(cam, scr(), orc.make_params(2, 1, seed=5), spheres, model, instances=inst))
        for i in range(n_slots):
            ctx.frame(pcall, pwant, tag=t + ("3g path", i))
        ctx.set_instances(None)
        for i in range(n_slots + 1):
            ctx.frame(call, base, tag=t + ("3g rest after path", i))
            pwant1 = oracle.get((name, "3g path single"), lambda: orc.render_path(cam, scr(), orc.make_params(2, 1, seed=5), spheres, model))
            ctx.frame(pcall, pwant1, tag=t + ("3g path single", i))
        rest(ctx, n_slots, call, base, frames, t + ("3g after path",))
    if "h" in steps:   # single-triangle passes and orthographic rays between, then the resting call again
        tris = orc.make_triangles(SINGLE_TRIANGLES)
        none = orc.make_triangles()
        for key, tr, ortho in (("3h tris", tris, False), ("3h ortho", none, True), ("3h tris ortho", tris, True)):
            ctx.set_triangles(tr)
            dwant = oracle.get((name, key), lambda: orc.render_frame_ex(cam, scr(), spheres, tr, model, ortho=ortho))
            for i in range(n_slots + 1):
                ctx.frame(Call(cam, flags=FLAG_ORTHO_RAYS if ortho else 0), dwant, tag=t + (key, i))
            ctx.set_triangles(none)
            rest(ctx, n_slots, call, base, frames, t + (key + " after",))
    return base


def step_conditions(orc, oracle, scene):
    """The conditions of 3a and 3c on the oracle's frames alone: the two meshes differ in obj_id; each one-ulp camera differs
    from the resting one in the bits of hit_t in at least one pixel, but for the translation column's (ulp_cams).  Returns the
    four pixel counts: the swap, the projection, the origin, the column."""
    name = scene["name"]
    cam = resting_cam(orc, scene, STEP_SIZE)
    scr = orc.make_screen(*STEP_SIZE)
    base = oracle.get((name, "base"), lambda: orc.render_frame(cam, scr, scene["spheres"], scene["model"]))
    other = oracle.get((name, "3a"), lambda: orc.render_frame(cam, scr, scene["spheres"], scene["other"]))
    counts = [int((base["obj_id"] != other["obj_id"]).sum())]
    for key, c1 in zip(ULP_KEYS, ulp_cams(cam)):
        f = oracle.get((name, key), lambda: orc.render_frame(c1, scr, scene["spheres"], scene["model"]))
        counts.append(int((f["hit_t"].view(np.uint32) != base["hit_t"].view(np.uint32)).sum()))
    return tuple(counts)


def run_default_rules(ctx, orc, case, want, n_frames=6):
    """A case on a context with the default rules (small plain frames with frames in flight fuse, small faces go to the BVH
    kernel): plain and aux frames alternate, every one compared."""
    ctx.upload(case["model"]); ctx.set_spheres(case["spheres"]); ctx.resize(*case["size"]); ctx.set_slots(case["n_slots"])
    call = Call(case["cam"])
    rgba8 = None
    for i in range(n_frames):
        got = ctx.frame(call, want, aux=bool(i % 2), tag=(case["name"], "default", i), rgba8=rgba8)[0]
        if i % 2:
            rgba8 = got["color"]
