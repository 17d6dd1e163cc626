"""The case list for the path tracer's extensions taken together (test infrastructure): deeper paths, shadow rays, sky light,
mirror surfaces, with normal maps, RWR_FLAG_NO_CULL, rotated instances, parts and frames in flight drawn on top.

case(i, ...) is deterministic in i (np.random.default_rng(BASE + i) and nothing else; no clock).  Case i takes combination i % 16 of
{depth > 1, shadows, sky, mirrors}: with N_CASES = 64 every combination occurs four times.  DIRECTED names the hand-built cases,
the list's last entries (listed(j) walks random cases and directed cases as one list).  reference() is mirror_ref.c's frame of a
case, gpu_frame() the product's, compare() the comparison both tests/test_gpu_path_cases.py and tools/fuzz_parity.py --path make;
tests/test_path_cases_host.py asserts with the reference alone that the list exercises what the GPU file relies on."""
import os
import re

import numpy as np

import fuzz_common
import mirror_common
import mirror_ref
import shadow_common
import world_offset_common

HERE = os.path.dirname(os.path.abspath(__file__))
# the colour bar of the deeper paths (the sky and mirror files read the same line): not a tolerance of this file's own
COLOR_TOL = float(re.search(r"^COLOR_TOL\s*=\s*([0-9.eE+-]+)", open(os.path.join(HERE, "test_gpu_multi_bounce.py")).read(), re.M).group(1))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")

BASE = 52000
N_CASES = 64
FACE_COUNTS = (1, 7, 63, 65, 129, 257, 300)      # around the batch edges
MANY_SAMPLES = {11: 33, 15: 65}                  # i % 32 -> spp: a launch group crossed unevenly, under three and four flags
# include/rwr_hip.h
FLAG_AUX_OUTPUTS, FLAG_NO_CULL, FLAG_NORMAL_MAP, FLAG_ACCUMULATE = 1, 2, 1 << 4, 1 << 5
FLAG_MULTI_BOUNCE, FLAG_SHADOWS, FLAG_SKY, FLAG_MIRRORS = 1 << 6, 1 << 7, 1 << 9, 1 << 10
# the schedule tests/test_gpu_fuzz.py forces: every pool traced as packets, launch groups of five samples
FORCED_SCHEDULE = {"RWR_WF_GROUP": "5", "RWR_WF_PACKET_FILL": "0", "RWR_WF_PACKET_EXTENT": "1e30", "RWR_WF_MIN_PACKET_POOLS": "0"}

_cache = {}


# ------------------------------------------------------------------ ingredients --
def _rotation(axis, angle) -> np.ndarray:
    """Rodrigues' formula in float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * (k @ k)


def instances(orc, rotations, translations) -> np.ndarray:
    """Rigid instances: the matrices built in float64 and stored as float32, column-major (m[column][row]) as fuzz_common does."""
    inst = np.zeros(len(rotations), dtype=orc.INSTANCE_DTYPE)
    for k, (r, t) in enumerate(zip(rotations, translations)):
        m = np.eye(4)
        m[:3, :3] = r
        m[:3, 3] = t
        inst["model"][k] = m.T.astype(np.float32)
    return inst


def _reflectance(rng) -> tuple:
    """Per channel: 0, 1 or uniform."""
    return tuple(float((0.0, 1.0, rng.uniform(0.0, 1.0))[int(rng.integers(0, 3))]) for _ in range(3))


def _split(model, ambients=((0.12, 0.03, 0.02), (0.02, 0.04, 0.15))) -> list:
    """A mesh's faces dealt to two parts with materials of their own (both carry every vertex, and the mesh's normal map)."""
    f = model["faces"]
    n = len(f) // 2
    parts = []
    for k, faces in enumerate((f[:n], f[n:])):
        mat = model["material"].copy()
        mat["ambient"] = ambients[k]
        parts.append({"vertices": model["vertices"], "faces": faces.copy(), "material": mat, "texture": model["texture"],
                      "normal_map": model.get("normal_map")})
    return parts


def _quad(ref_loader, tex, corners):
    a, b, c, d = corners
    return shadow_common.triangle_model(ref_loader, [(a, b, c), (a, c, d)], tex)


def _camera(orc, eye, target, w, h, fovy=60.0):
    return orc.camera_build_inv_uniform(orc.make_camera(eye=tuple(eye), target=tuple(target), aspect=w / h, fovy=fovy))


def _finish(orc, c) -> dict:
    c.setdefault("instances", None)
    c.setdefault("fovy", 60.0)
    c.setdefault("seed", 13)
    c.setdefault("extra", 0)
    c.setdefault("sky_colors", (mirror_ref.DEFAULT_ZENITH, mirror_ref.DEFAULT_HORIZON))
    c.setdefault("mirror_parts", {})
    c.setdefault("mirror_spheres", {})
    c.setdefault("frames_in_flight", 1)
    for k in ("multi", "shadows", "sky", "mirrors"):
        c.setdefault(k, False)
    c["multi"] = c["bounces"] > 1
    c["cam_inv"] = _camera(orc, c["eye"], c["target"], c["w"], c["h"], c["fovy"])
    return c


# ------------------------------------------------------------------ the random cases --
def case(i, ref_loader, orc, cube, suzanne) -> dict:
    """Case i: model (one model or a list of parts), spheres, instances, eye / target / fovy (and cam_inv), w, h, spp, bounces,
    seed, the four extension switches (multi, shadows, sky, mirrors) and extra flags, sky_colors, mirror_parts, mirror_spheres,
    frames_in_flight.  Nothing the header refuses is drawn (orthographic rays, the BVH kernel, single triangles)."""
    key = ("case", i)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(BASE + i)
    combo = i % 16
    multi, shadows, sky, mirrors = bool(combo & 1), bool(combo & 2), bool(combo & 4), bool(combo & 8)
    many = MANY_SAMPLES.get(i % 32)
    tex = suzanne["texture"]
    kind = rng.random()
    if many:             # <= 65 faces: a soup
        kind = 0.0
    if kind < 0.45:      # a soup, with a second part of its own texture now and then
        n_faces = int(rng.choice(FACE_COUNTS[:4] if many else FACE_COUNTS))
        few = n_faces <= 7
        model = fuzz_common.soup(ref_loader, rng, n_faces, extent=0.5 if few else float(rng.choice([0.5, 1.2, 2.0])),
                                 tri_size=float(rng.choice([0.8, 1.5] if few else [0.15, 0.4, 1.0])), tex=tex)
        what = f"soup {n_faces}"
        if rng.random() < 0.4 and not many:
            tex2 = rng.integers(0, 256, (int(rng.integers(1, 40)), int(rng.integers(1, 40)), 4), dtype=np.uint8)
            other = fuzz_common.soup(ref_loader, rng, int(rng.integers(1, 200)), extent=1.5, tri_size=0.5, tex=tex2)
            other["material"]["ambient"], other["material"]["specular"] = rng.uniform(0, 0.3, 3), rng.uniform(0, 1, 3)
            model = [model, other]
            what += f" + part of {len(other['faces'])} faces, texture {tex2.shape[1]}x{tex2.shape[0]}"
    elif kind < 0.62:    # the real meshes: exactly shared edges and vertices
        model, what = cube, "cube"
    elif kind < 0.78:
        model, what = suzanne, "suzanne"
    else:
        model, what = _split(cube), "cube halves"
    parts = list(model) if isinstance(model, list) else [model]
    n_faces = sum(len(p["faces"]) for p in parts)
    nmap = bool(rng.random() < 0.3)
    if nmap and what.startswith("soup"):     # a random map (of a size of its own) on the soup's last part
        m = rng.integers(0, 256, (int(rng.integers(1, 40)), int(rng.integers(1, 40)), 4), dtype=np.uint8)
        m[..., 2] |= 0x80                    # mostly outward-pointing normals
        parts[-1]["normal_map"] = m
    no_cull = bool(rng.random() < 0.2)
    spheres = orc.make_spheres([(tuple(rng.uniform(-2.2, 2.2, 3)), float(rng.uniform(0.05, 1.2))) for _ in range(int(rng.integers(0, 9)))])
    inst = None
    if rng.random() < 0.4:
        k = 2 if n_faces >= 300 else int(rng.integers(2, 5))
        inst = instances(orc, [_rotation(rng.normal(size=3), rng.uniform(0, 2 * np.pi)) for _ in range(k)], [rng.uniform(-2.5, 2.5, 3) for _ in range(k)])
    if many:
        w, h = int(rng.integers(5, 25)), int(rng.integers(3, 17))
    else:
        w, h = int(rng.integers(5, 81)), int(rng.integers(3, 57))
    d = rng.normal(size=3)
    eye = d / np.linalg.norm(d) * rng.uniform(2.5, 5.5)
    target = rng.uniform(-0.5, 0.5, 3)
    fovy = float(rng.choice([rng.uniform(35, 80), rng.uniform(35, 80), rng.uniform(15, 35), rng.uniform(80, 120)]))
    spp = many or int(rng.choice([1, 2, 5, 9]))
    bounces = int(rng.choice([2, 3, 8])) if multi else 1
    # mirrors are drawn for every case: without the flag they are set and must do nothing
    mirror_parts = {k: _reflectance(rng) for k in range(len(parts)) if rng.random() < 0.6}
    mirror_spheres = {k: _reflectance(rng) for k in range(len(spheres)) if rng.random() < 0.5}
    if not mirror_parts and not mirror_spheres:
        mirror_parts = {0: _reflectance(rng)}
    c = dict(index=i, what=what, model=model, spheres=spheres, instances=inst, eye=tuple(map(float, eye)), target=tuple(map(float, target)), fovy=fovy,
             w=w, h=h, spp=spp, bounces=bounces, seed=int(rng.integers(0, 1000)), shadows=shadows, sky=sky, mirrors=mirrors,
             extra=(FLAG_NORMAL_MAP if nmap else 0) | (FLAG_NO_CULL if no_cull else 0),
             sky_colors=(tuple(map(float, rng.uniform(0, 2, 3))), tuple(map(float, rng.uniform(0, 2, 3)))),
             mirror_parts=mirror_parts, mirror_spheres=mirror_spheres, frames_in_flight=int(rng.integers(1, 4)))
    _cache[key] = _finish(orc, c)
    return _cache[key]


# ------------------------------------------------------------------ the directed cases --
def inside_mirror_sphere(ref_loader, orc, cube, suzanne) -> dict:
    """The eye inside sphere 0, a mirror of R = 1; sphere 1 outside it; all of it inside the cube, scaled to a closed room, so
    that no path ends before B = 8.  By the header's rule n is the OUTWARD normal at an inside hit: the next ray starts 1e-4
    outside the sphere, its reflection points back in and finds the sphere again, from outside, after ~1e-4 (generation 1, a
    reflection as well), and generation 2 leaves along almost the primary ray's direction into the room."""
    room = world_offset_common.translated(cube, (0.0, 0.0, 0.0), scale=4.0)
    return _finish(orc, dict(what="inside_mirror_sphere", model=room, spheres=orc.make_spheres([((0.0, 0.0, 0.0), 1.0), ((1.9, 0.6, -1.5), 0.7)]),
                             eye=(0.2, 0.1, 0.3), target=(1.0, 0.3, -1.0), fovy=75.0, w=40, h=28, spp=2, bounces=8, shadows=True, sky=True,
                             mirrors=True, mirror_spheres={0: (1.0, 1.0, 1.0)}))


def facing_mirrors(ref_loader, orc, cube, suzanne) -> dict:
    """Two parallel quads 2 apart (x = -1 and x = +1), both mirror parts, a small diffuse cube between them, the eye between them."""
    tex = cube["texture"]
    left = _quad(ref_loader, tex, [(-1.0, -2.0, -3.0), (-1.0, -2.0, 3.0), (-1.0, 2.0, 3.0), (-1.0, 2.0, -3.0)])
    right = _quad(ref_loader, tex, [(1.0, -2.0, -3.0), (1.0, 2.0, -3.0), (1.0, 2.0, 3.0), (1.0, -2.0, 3.0)])
    small = world_offset_common.translated(cube, (0.1, -0.2, -0.6), scale=0.25)
    return _finish(orc, dict(what="facing_mirrors", model=[left, right, small], spheres=orc.make_spheres([]), eye=(0.3, 0.2, 1.6), target=(-1.0, 0.0, -0.2),
                             fovy=70.0, w=48, h=32, spp=3, bounces=8, sky=True, mirrors=True,
                             mirror_parts={0: (1.0, 1.0, 1.0), 1: (0.9, 0.6, 0.3)}))


def black_mirror(ref_loader, orc, cube, suzanne) -> dict:
    """mirror_common's quad_floor (its quad under the cube, its camera, size and samples) with R = (0, 0, 0), B = 1: the reflected
    rays carry nothing and are rays all the same."""
    return _finish(orc, dict(what="black_mirror", model=[mirror_common._quad(ref_loader, cube), cube], spheres=orc.make_spheres([]), eye=(2.4, 1.6, 3.4),
                             target=(0.0, -0.6, 0.0), w=64, h=48, spp=4, bounces=1, sky=True, mirrors=True, mirror_parts={0: (0.0, 0.0, 0.0)}))


def rotated_parts(ref_loader, orc, cube, suzanne) -> dict:
    """The split cube (part 1 a mirror) under three rotated instances, side by side so that each shows in the others' mirror faces."""
    inst = instances(orc, [_rotation(a, t) for a, t in (((1, 1, 0), 0.7), ((0, 1, 1), 2.1), ((1, 0, 1), 4.0))], [(-3.1, 0.0, 0.0), (0.0, 0.2, 0.0), (3.1, -0.1, 0.3)])
    return _finish(orc, dict(what="rotated_parts", model=_split(cube), spheres=orc.make_spheres([((0.0, 2.3, 0.4), 0.6)]), instances=inst, eye=(0.5, 2.5, 8.0),
                             target=(0.0, 0.0, 0.0), fovy=55.0, w=72, h=40, spp=4, bounces=3, shadows=True, sky=True, mirrors=True,
                             mirror_parts={1: (0.6, 1.0, 0.8)}))


def nmap_mirror(ref_loader, orc, cube, suzanne) -> dict:
    """The cube with its normal map and RWR_FLAG_NORMAL_MAP, a second cube beside it (mirror_common._two_parts), part 0 a mirror."""
    parts = [dict(p, normal_map=cube["normal_map"]) for p in mirror_common._two_parts(cube)]
    return _finish(orc, dict(what="nmap_mirror", model=parts, spheres=orc.make_spheres([]), eye=(3.2, 1.9, 3.6), target=(1.2, 0.0, 0.0), w=64, h=48, spp=4,
                             bounces=2, sky=True, mirrors=True, extra=FLAG_NORMAL_MAP, mirror_parts={0: (1.0, 0.5, 0.75)}))


def no_cull_all(ref_loader, orc, cube, suzanne) -> dict:
    """One soup with RWR_FLAG_NO_CULL and all four extension flags."""
    rng = np.random.default_rng(BASE - 1)
    model = fuzz_common.soup(ref_loader, rng, 129, extent=1.2, tri_size=0.4, tex=suzanne["texture"])
    return _finish(orc, dict(what="no_cull_all", model=model, spheres=orc.make_spheres([((0.9, 0.4, 0.6), 0.5), ((-0.8, -0.5, 0.2), 0.35)]), eye=(0.3, 0.5, 3.2),
                             target=(0.0, 0.0, 0.0), w=53, h=37, spp=5, bounces=3, shadows=True, sky=True, mirrors=True, extra=FLAG_NO_CULL,
                             mirror_parts={0: (0.9, 0.6, 0.3)}, mirror_spheres={1: (0.25, 1.0, 0.8)}))


def far_mirror(ref_loader, orc, cube, suzanne) -> dict:
    """world_offset_common's suzanne and a mirror sphere beside it, 1e4 away from the origin on every axis."""
    off = np.asarray(world_offset_common.OFFSETS["1e4"], np.float64)
    model = world_offset_common.translated(suzanne, off)
    spheres = orc.make_spheres([(tuple(np.array([1.7, 0.2, 0.3]) + off), 0.8), (tuple(np.array([-1.6, -0.3, 0.6]) + off), 0.5)])
    return _finish(orc, dict(what="far_mirror", model=model, spheres=spheres, eye=tuple(np.array([0.6, 0.5, 4.0]) + off), target=tuple(np.array([0.2, 0.0, 0.0]) + off),
                             w=60, h=36, spp=2, bounces=2, shadows=True, sky=True, mirrors=True, mirror_spheres={0: (1.0, 0.9, 0.8)}))


def all_sphere_mirrors(ref_loader, orc, cube, suzanne) -> dict:
    """Eight spheres, every one a mirror of its own R, in front of a soup of two parts: the table's records n_parts + k."""
    rng = np.random.default_rng(BASE - 2)
    tex2 = rng.integers(0, 256, (9, 17, 4), dtype=np.uint8)
    back = [fuzz_common.soup(ref_loader, rng, 65, extent=1.6, tri_size=0.7, tex=suzanne["texture"]), fuzz_common.soup(ref_loader, rng, 63, extent=1.6, tri_size=0.7, tex=tex2)]
    for p in back:
        p["vertices"]["position"][:, 2] -= 2.5
    spec = [((-1.8 + 1.2 * (k % 4), -0.6 + 1.2 * (k // 4), 0.4 * (k % 3)), 0.5) for k in range(8)]
    refl = {k: (0.2 + 0.1 * k, 1.0 - 0.1 * k, 0.125 * k) for k in range(8)}
    return _finish(orc, dict(what="all_sphere_mirrors", model=back, spheres=orc.make_spheres(spec), eye=(0.0, 0.0, 4.5), target=(0.0, 0.0, 0.0), w=64, h=40,
                             spp=3, bounces=3, shadows=True, sky=True, mirrors=True, mirror_spheres=refl))


DIRECTED = {f.__name__: f for f in (inside_mirror_sphere, facing_mirrors, black_mirror, rotated_parts, nmap_mirror, no_cull_all, far_mirror,
                                    all_sphere_mirrors)}
N_LISTED = N_CASES + len(DIRECTED)


def directed(name, ref_loader, orc, cube, suzanne) -> dict:
    key = ("directed", name)
    if key not in _cache:
        _cache[key] = dict(DIRECTED[name](ref_loader, orc, cube, suzanne), index=name)
    return _cache[key]


def listed(j, ref_loader, orc, cube, suzanne) -> dict:
    """Entry j of the committed list: the N_CASES random cases, then the directed ones."""
    if j < N_CASES:
        return case(j, ref_loader, orc, cube, suzanne)
    return directed(list(DIRECTED)[j - N_CASES], ref_loader, orc, cube, suzanne)


# ------------------------------------------------------------------ what a case is, in words and in numbers --
def n_parts(c) -> int:
    return len(c["model"]) if isinstance(c["model"], (list, tuple)) else 1


def n_base_faces(c) -> int:
    return sum(len(p["faces"]) for p in (c["model"] if isinstance(c["model"], (list, tuple)) else [c["model"]]))


def flags(c, mirrors=None, extra=None) -> int:
    mirrors = c["mirrors"] if mirrors is None else mirrors
    return (FLAG_AUX_OUTPUTS | (c["extra"] if extra is None else extra) | (FLAG_MULTI_BOUNCE if c["bounces"] > 1 else 0) |
            (FLAG_SHADOWS if c["shadows"] else 0) | (FLAG_SKY if c["sky"] else 0) | (FLAG_MIRRORS if mirrors else 0))


def describe(c) -> str:
    """The drawn parameters: enough to rebuild the case on the CPU from its index and to see what it is."""
    inst = 0 if c["instances"] is None else len(c["instances"])
    return (f"case {c['index']}: {c['what']} ({n_base_faces(c)} faces, {n_parts(c)} parts), {len(c['spheres'])} spheres, {inst} instances, {c['w']}x{c['h']} "
            f"spp {c['spp']} B {c['bounces']} seed {c['seed']} fovy {c['fovy']:.1f} flags 0x{flags(c):x} (shadows {int(c['shadows'])} sky {int(c['sky'])} "
            f"mirrors {int(c['mirrors'])}) sky {c['sky_colors']} mirror parts {c['mirror_parts']} spheres {c['mirror_spheres']} in flight {c['frames_in_flight']}")


def color_bar(c) -> float:
    """COLOR_TOL, scaled by the largest sky component above 1 where the sky is on (tests/test_gpu_sky.py: a sky term's error is
    relative to S, and S lies between the two colours)."""
    return COLOR_TOL * (max(1.0, max(max(k) for k in c["sky_colors"])) if c["sky"] else 1.0)


# ------------------------------------------------------------------ the reference's frame --
def reference(L, orc, c, mirrors=None, first=False, use_sky_ref=False, **over) -> dict:
    """mirror_ref.c's frame of case c (kept for the session; never modified by a test).  over: spp, bounces, extra, mirror_parts."""
    mirrors = c["mirrors"] if mirrors is None else mirrors
    key = ("ref", c["index"], mirrors, first, use_sky_ref, tuple(sorted((k, str(v)) for k, v in over.items())))
    if key not in _cache:
        extra = over.get("extra", c["extra"])
        params = orc.make_params(over.get("spp", c["spp"]), over.get("bounces", c["bounces"]), seed=c["seed"], flags=extra & FLAG_NORMAL_MAP)
        _cache[key] = mirror_ref.render_path(L, orc, c["cam_inv"].view(orc.CAMERA_INV_DTYPE), orc.make_screen(c["w"], c["h"]), params,
                                             c["spheres"].view(orc.SPHERE_DTYPE), c["model"], instances=c["instances"], shadows=c["shadows"],
                                             sky=c["sky_colors"] if c["sky"] else None, first=first, use_sky_ref=use_sky_ref,
                                             mirror_parts=over.get("mirror_parts", c["mirror_parts"]) if mirrors else None,
                                             mirror_spheres=c["mirror_spheres"] if mirrors else None)
    return _cache[key]


def forget(c):
    """Drops what the session keeps of case c (a long walk of the list, tools/fuzz_parity.py --path, keeps nothing)."""
    for key in [k for k in _cache if k[1] == c["index"]]:
        del _cache[key]


# ------------------------------------------------------------------ the product's frame --
def upload(ctx, c):
    """Scene, instances, spheres, size, sky parameters, mirrors, frames in flight.  The mirrors are set whether or not the case
    renders with the flag: without it they must do nothing."""
    if isinstance(c["model"], (list, tuple)):
        ctx.upload_parts(c["model"])
    else:
        ctx.upload_model(c["model"])
    ctx.set_instances(c["instances"])
    ctx.set_spheres(c["spheres"])
    ctx.resize(c["w"], c["h"])
    ctx.sky_set_params(*c["sky_colors"])
    for k in range(mirror_ref.MAX_SPHERES):      # (the sphere attributes outlive rwr_scene_set_spheres: a context used before)
        ctx.set_sphere_mirror(k, None)
    for k, r in c["mirror_parts"].items():
        ctx.set_part_mirror(k, r)
    for k, r in c["mirror_spheres"].items():
        ctx.set_sphere_mirror(k, r)
    ctx.set_frames_in_flight(c["frames_in_flight"])


def frame(ctx, c, params, **kw) -> dict:
    ctx.render(c["cam_inv"], params, **kw)
    out = ctx.readback(aux=True)
    out["stats"] = ctx.last_render_stats()
    out["shadow"] = ctx.last_shadow_stats()
    return out


def gpu_frame(rwr, c, ctx=None) -> dict:
    """The case's frame on a context of its own (whatever RWR_WF_* the environment holds is read when it is made), or on the
    context given: one frame per frame in flight, so that every slot has rendered; all of them must be the same bytes, the last
    is returned."""
    params = rwr.make_params(spp=c["spp"], max_bounces=c["bounces"], seed=c["seed"], flags=flags(c))
    if ctx is None:
        with rwr.Context(0) as own:
            return gpu_frame(rwr, c, own)
    upload(ctx, c)
    frames = [frame(ctx, c, params) for _ in range(c["frames_in_flight"])]
    for f in frames[:-1]:
        same(f, frames[-1], c, "frames in flight")
    return frames[-1]


def same(a, b, c, what, stats=True):
    """All five planes the same bytes, and (stats) both counts of rays."""
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k, describe(c))
    assert not stats or a["stats"] == b["stats"] and a["shadow"] == b["shadow"], (what, a["stats"], b["stats"], a["shadow"], b["shadow"], describe(c))


def compare(got, want, c) -> float:
    """The product's frame of case c against the reference's: sample-0 planes bit for bit, the ray and shadow-ray counts equal,
    RGBA8 within one code, float colour within color_bar(c).  Returns the colour error."""
    tag = describe(c)
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (k, tag)
    assert got["stats"] == (c["w"] * c["h"] * c["spp"], want["rays"]), (got["stats"], want["rays"], want["gen_rays"].tolist(), tag)
    assert got["shadow"] == ((want["shadow_rays"], want["occluded"]) if c["shadows"] else (0, 0)), (got["shadow"], want["shadow_rays"], want["occluded"], tag)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, ("rgba8", tag)
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    bar = color_bar(c)
    assert err <= bar, (err, bar, tag)
    return err


# ------------------------------------------------------------------ further contexts: schedules, accumulation, splits --
class environment:
    """The given variables set while a context is made and used (the RWR_WF_* tunables are read when a context is created), the
    old values back afterwards."""

    def __init__(self, values):
        self.values = dict(values)

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.values}
        os.environ.update(self.values)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# Chosen from the list (tests/test_path_cases_host.py asserts what they were chosen for): four cases of spp >= 2 for "K frames of
# s samples are one frame of K s" - mirrors on rotated instances (29, 58, 44) and two mirror parts at B = 3 with shadows (59) - and
# two cases for strips of two ranks, both ranks owning rows.
ACCUMULATION = (29, 58, 44, 59)
SPLITS = (29, 59)


def accumulation_steps(c) -> tuple:
    """(K, s) with K s = the case's spp."""
    return {2: (2, 1), 5: (5, 1), 9: (3, 3)}[c["spp"]]


def accumulated_frame(rwr, c) -> dict:
    """K frames of s samples with RWR_FLAG_ACCUMULATE on a context of its own; the last frame shown (its counts are that frame's
    s samples alone)."""
    k, s = accumulation_steps(c)
    params = rwr.make_params(spp=s, max_bounces=c["bounces"], seed=c["seed"], flags=flags(c) | FLAG_ACCUMULATE)
    with rwr.Context(0) as ctx:
        upload(ctx, c)
        ctx.accum_reset()
        for n in range(1, k + 1):
            out = frame(ctx, c, params)
            assert ctx.accum_samples() == n * s, (n, s, describe(c))
    return out


def strips_frame(rwr, c, ranks=2) -> tuple:
    """The frame assembled from strips of `ranks` ranks, each rendered alone and deposited through the loopback: (the planes put
    together row by row with the summed counts, the gathered RGBA8 frame)."""
    c = dict(c, frames_in_flight=1)
    params = rwr.make_params(spp=c["spp"], max_bounces=c["bounces"], seed=c["seed"], flags=flags(c))
    with rwr.Context(0) as ctx:
        upload(ctx, c)
        asm, rays, shadow = None, 0, [0, 0]
        for r in range(ranks):
            part = frame(ctx, c, params, strips=(r, ranks))
            if asm is None:
                asm = {k: np.zeros_like(part[k]) for k in PLANES}
            rows = [y for y in range(c["h"]) if (y // 8) % ranks == r]
            for k in PLANES:
                asm[k][rows] = part[k][rows]
            rays += part["stats"][1]
            shadow[0] += part["shadow"][0]
            shadow[1] += part["shadow"][1]
            ctx.dist_loopback_deposit(r, ranks, True)
        ctx.dist_loopback_finish(ranks, True)
        gathered = ctx.dist_readback()
    asm["stats"] = (c["w"] * c["h"] * c["spp"], rays)
    asm["shadow"] = tuple(shadow)
    return asm, gathered
