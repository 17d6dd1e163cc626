"""The case list for glass taken with the other path extensions (test infrastructure): tests/path_cases.py's random cases beyond
its committed 64, with glass surfaces drawn on top, and the directed cases that pin one rule of RWR_FLAG_GLASS each.

glass_case(g, ...) is deterministic in g alone: it is path_cases.case(path_cases.N_CASES + g) - so case g has combination g % 16 of
{depth > 1, shadows, sky, mirrors} - plus what np.random.default_rng(GLASS_BASE + g), a generator of its own, draws: every part and
every sphere is glass with probability 1/2 (at least one surface is; a glass surface is taken out of the case's mirrors: a surface
has one model), of an index from {1, 1.33, 1.5, 2.4, 4, uniform in [1, 4]} and a tint per channel from {0, 1, uniform}.
RWR_FLAG_GLASS is on unless g // 16 == 3: with N_GLASS_CASES = 64 every combination of the other four occurs three times with the
flag and once with glass surfaces set and the flag off, where glass must do nothing.  DIRECTED names the hand-built cases.
reference() is glass_ref.c's frame of a case, gpu_frame() the product's, compare() the comparison both
tests/test_gpu_glass_cases.py and tools/fuzz_parity.py --path --glass make; tests/test_glass_cases_host.py asserts with the
reference alone that the list exercises what the GPU file relies on."""
import numpy as np

import fuzz_common
import glass_common
import glass_ref
import mirror_common
import path_cases as pc
import world_offset_common

GLASS_BASE = 91000
N_GLASS_CASES = 64
FLAG_GLASS = 1 << 11                      # include/rwr_hip.h
IORS = (1.0, 1.33, 1.5, 2.4, 4.0)         # the range's edges and the common values (water, crown glass, diamond)
PLANES = pc.PLANES

_cache = {}


# ------------------------------------------------------------------ the random cases --
def _ior(rng) -> float:
    k = int(rng.integers(0, len(IORS) + 1))
    return float(IORS[k]) if k < len(IORS) else float(rng.uniform(1.0, 4.0))


def _glass(rng) -> tuple:
    return (_ior(rng), pc._reflectance(rng))


def glass_case(g, ref_loader, orc, cube, suzanne) -> dict:
    """Case g: path_cases' case N_CASES + g (a copy; the case itself is left as it is) with glass (the switch), glass_parts and
    glass_spheres ({index: (ior, tint)}), and its mirror dictionaries without the surfaces that became glass."""
    key = ("case", g)
    if key in _cache:
        return _cache[key]
    base = pc.case(pc.N_CASES + g, ref_loader, orc, cube, suzanne)
    rng = np.random.default_rng(GLASS_BASE + g)
    n_p, n_s = pc.n_parts(base), len(base["spheres"])
    glass_parts = {k: _glass(rng) for k in range(n_p) if rng.random() < 0.5}
    glass_spheres = {k: _glass(rng) for k in range(n_s) if rng.random() < 0.5}
    if not glass_parts and not glass_spheres:
        k = int(rng.integers(0, n_p + n_s))
        if k < n_p:
            glass_parts = {k: _glass(rng)}
        else:
            glass_spheres = {k - n_p: _glass(rng)}
    c = dict(base, index=f"glass {g}", g=g, glass=g // 16 != 3, glass_parts=glass_parts, glass_spheres=glass_spheres,
             mirror_parts={k: r for k, r in base["mirror_parts"].items() if k not in glass_parts},
             mirror_spheres={k: r for k, r in base["mirror_spheres"].items() if k not in glass_spheres})
    _cache[key] = c
    return c


# ------------------------------------------------------------------ the directed cases --
def _finish(orc, c) -> dict:
    c.setdefault("glass", True)
    c.setdefault("glass_parts", {})
    c.setdefault("glass_spheres", {})
    return pc._finish(orc, c)


def back_face_pane(ref_loader, orc, cube, suzanne) -> dict:
    """Which side a face is seen from at h0, on open geometry.  Two quads in the plane z = 0, both glass of ior 1.5, max_bounces 1:
    part 0 (x < 0) turns its back to the eye, part 1 (x > 0) its front.  Every glass event is an h0 event.  Through the back face
    a ray leaves glass it never entered (entering = 0 from the stored N.D, e = eta): past the critical angle of 41.8 degrees, which
    the eye at z = 1.2 sees for |x| > 1.07, it reflects totally.  The front-facing twin is seen at the same angles and gives
    Fresnel reflections and transmissions alone.  A diffuse cube stands behind both."""
    tex = cube["texture"]
    back = pc._quad(ref_loader, tex, [(-3.0, -1.2, 0.0), (-3.0, 1.2, 0.0), (-0.1, 1.2, 0.0), (-0.1, -1.2, 0.0)])      # normal -z
    front = pc._quad(ref_loader, tex, [(0.1, -1.2, 0.0), (3.0, -1.2, 0.0), (3.0, 1.2, 0.0), (0.1, 1.2, 0.0)])         # normal +z
    behind = world_offset_common.translated(cube, (0.0, 0.0, -2.5), scale=1.0)
    return _finish(orc, dict(what="back_face_pane", model=[back, front, behind], spheres=orc.make_spheres([]), eye=(0.0, 0.2, 1.2), target=(0.0, 0.0, 0.0),
                             fovy=90.0, w=71, h=47, spp=3, bounces=1, sky=True, glass_parts={0: (1.5, (1.0, 1.0, 1.0)), 1: (1.5, (1.0, 1.0, 1.0))}))


def soup_glass_all(ref_loader, orc, cube, suzanne) -> dict:
    """Entering against leaving on a soup: 129 unconnected triangles, glass, seen from either side at h0 and at every bounce hit,
    with RWR_FLAG_NO_CULL and all five extension flags, B = 3; two spheres, of which sphere 1 is a mirror."""
    rng = np.random.default_rng(GLASS_BASE - 1)
    model = fuzz_common.soup(ref_loader, rng, 129, extent=1.2, tri_size=0.4, tex=suzanne["texture"])
    return _finish(orc, dict(what="soup_glass_all", model=model, spheres=orc.make_spheres([((0.9, 0.4, 0.6), 0.5), ((-0.8, -0.5, 0.2), 0.35)]), eye=(0.3, 0.5, 3.2),
                             target=(0.0, 0.0, 0.0), w=53, h=37, spp=5, bounces=3, shadows=True, sky=True, mirrors=True, extra=pc.FLAG_NO_CULL,
                             glass_parts={0: (1.5, (0.9, 1.0, 0.8))}, mirror_spheres={1: (0.25, 1.0, 0.8)}))


def nmap_glass(ref_loader, orc, cube, suzanne) -> dict:
    """Normal maps shade and never steer: the two-part cube scene of path_cases.nmap_mirror with part 0 glass and
    RWR_FLAG_NORMAL_MAP; n of the glass rule is the HitRecord normal, so events and rays are those of the frame without the map."""
    c = dict(pc.nmap_mirror(ref_loader, orc, cube, suzanne), what="nmap_glass", w=61, h=45, mirror_parts={}, mirrors=False)
    return _finish(orc, dict(c, glass_parts={0: (1.5, (1.0, 0.5, 0.75))}))


ALL_SPHERE_IORS = (1.0, 1.33, 1.5, 2.4, 4.0, 1.1, 2.0, 3.0)


def _all_sphere_glass(bounces):
    def build(ref_loader, orc, cube, suzanne) -> dict:
        c = dict(pc.all_sphere_mirrors(ref_loader, orc, cube, suzanne), what=f"all_sphere_glass_b{bounces}", w=63, h=41, bounces=bounces, mirror_spheres={})
        glass = {k: (ALL_SPHERE_IORS[k], (0.2 + 0.1 * k, 1.0 - 0.1 * k, 0.125 * k)) for k in range(8)}
        return _finish(orc, dict(c, glass_spheres=glass, mirror_parts={1: (0.9, 0.7, 0.5)}))
    build.__name__ = f"all_sphere_glass_b{bounces}"
    build.__doc__ = """The table's records n_parts + k: eight spheres, each glass of an index and a tint of its own, in front of a soup of two
    parts whose part 1 is a mirror (record 1; the spheres' records begin at 2).  Rendered at B = 1, where every event is an h0 event
    on a sphere, and at B = 3."""
    return build


def nested_spheres(ref_loader, orc, cube, suzanne) -> dict:
    """The rule without a stack: glass sphere 1 (ior 2.4) wholly inside glass sphere 0 (ior 1.5), the eye outside, a diffuse cube
    behind, B = 8.  Each boundary is decided by its own n.Dh and its own eta against 1 (entering the inner sphere from inside the
    outer one is e = 1 / 2.4, not 1.5 / 2.4): no physics of nested dielectrics, but the defined rule, and both sides follow it.
    A path through both spheres transmits four times."""
    behind = world_offset_common.translated(cube, (0.0, 0.0, -3.0), scale=1.5)
    return _finish(orc, dict(what="nested_spheres", model=behind, spheres=orc.make_spheres([((0.0, 0.0, 0.0), 1.0), ((0.15, 0.05, 0.1), 0.55)]),
                             eye=(0.3, 0.4, 3.4), target=(0.0, 0.0, 0.0), fovy=50.0, w=59, h=43, spp=3, bounces=8, sky=True,
                             glass_spheres={0: (1.5, (0.95, 1.0, 0.9)), 1: (2.4, (1.0, 0.9, 0.95))}))


def twin_spheres(ref_loader, orc, cube, suzanne) -> dict:
    """The nearest-hit rule's order at an exact tie: spheres 0 (glass) and 1 (a mirror) have the same centre and radius, so every hit
    on them, at h0 and at every bounce hit, ties in t, and the order decides which model acts.  The cube stands beside them."""
    twin = ((-0.4, 0.0, 0.0), 0.9)
    aside = world_offset_common.translated(cube, (1.6, -0.2, -0.5), scale=0.6)
    return _finish(orc, dict(what="twin_spheres", model=aside, spheres=orc.make_spheres([twin, twin]), eye=(0.4, 0.5, 3.6), target=(0.2, 0.0, 0.0),
                             w=57, h=39, spp=4, bounces=4, sky=True, mirrors=True, glass_spheres={0: (1.5, (1.0, 0.9, 0.8))},
                             mirror_spheres={1: (0.8, 0.9, 1.0)}))


def glass_between_mirrors(ref_loader, orc, cube, suzanne) -> dict:
    """The RNG dimension 2 + 16 (k - 1) of a Fresnel decision that follows mirror generations: path_cases.facing_mirrors with a glass
    quad (ior 1.33, tinted, its front to the eye) standing between the two mirror quads, B = 8: paths cross the pane at every
    generation up to the eighth, from both sides."""
    c = pc.facing_mirrors(ref_loader, orc, cube, suzanne)
    pane = pc._quad(ref_loader, cube["texture"], [(-0.4, -2.0, -3.0), (-0.4, 2.0, -3.0), (-0.4, 2.0, 3.0), (-0.4, -2.0, 3.0)])     # normal +x
    return _finish(orc, dict(c, what="glass_between_mirrors", model=list(c["model"]) + [pane], glass_parts={3: (1.33, (0.9, 0.8, 1.0))}))


def bright_sky_tint(ref_loader, orc, cube, suzanne) -> dict:
    """A tint <= 1 multiplied through a sky brighter than 1: a glass sphere of tint (1, 0.5, 0) over a floor quad (mirror_common's)
    under a sky with components up to 2, B = 4."""
    return _finish(orc, dict(what="bright_sky_tint", model=mirror_common._quad(ref_loader, cube), spheres=orc.make_spheres([((0.0, 0.1, 0.0), 0.9)]),
                             eye=(2.4, 1.6, 3.4), target=(0.0, -0.3, 0.0), w=67, h=45, spp=4, bounces=4, sky=True,
                             sky_colors=((2.0, 1.5, 0.5), (1.0, 2.0, 1.75)), glass_spheres={0: (1.5, (1.0, 0.5, 0.0))}))


def ior_four_room(ref_loader, orc, cube, suzanne) -> dict:
    """The range's upper edge: the closed glass cube of glass_common's cube_room at ior 4.0 (critical angle 14.5 degrees), B = 8,
    with the eye inside the glass: every h0 is a back face, and a path leaves only within 14.5 degrees of a face's normal (seen from
    outside, refraction would bend every ray to within that angle of the opposite face's normal, and most would leave at once).
    Almost every hit reflects totally, and a reflection in a cube keeps the angles to all three axes: such a path stays inside for
    all eight generations."""
    room = world_offset_common.translated(cube, (0.0, 0.0, 0.0), scale=4.0)
    return _finish(orc, dict(what="ior_four_room", model=[cube, room], spheres=orc.make_spheres([]), eye=(0.35, 0.2, 0.55), target=(-1.0, -0.5, -1.0),
                             fovy=75.0, w=70, h=46, spp=2, bounces=8, sky=True, glass_parts={0: (4.0, glass_common.CLEAR)}))


DIRECTED = {f.__name__: f for f in (back_face_pane, soup_glass_all, nmap_glass, _all_sphere_glass(1), _all_sphere_glass(3), nested_spheres, twin_spheres,
                                    glass_between_mirrors, bright_sky_tint, ior_four_room)}


def directed(name, ref_loader, orc, cube, suzanne) -> dict:
    key = ("directed", name)
    if key not in _cache:
        _cache[key] = dict(DIRECTED[name](ref_loader, orc, cube, suzanne), index=name)
    return _cache[key]


# ------------------------------------------------------------------ what a case is, in words and in numbers --
def flags(c, glass=None) -> int:
    glass = c["glass"] if glass is None else glass
    return pc.flags(c) | (FLAG_GLASS if glass else 0)


def describe(c) -> str:
    return f"{pc.describe(c)} glass {int(c['glass'])} (flags 0x{flags(c):x}) parts {c['glass_parts']} spheres {c['glass_spheres']}"


def glass_part_of_face(c) -> np.ndarray:
    """For every base face, whether its part is glass."""
    parts = c["model"] if isinstance(c["model"], (list, tuple)) else [c["model"]]
    return np.concatenate([np.full(len(p["faces"]), k in c["glass_parts"]) for k, p in enumerate(parts)])


def on_glass(c, obj_id) -> np.ndarray:
    """Whether the surface of an object id plane (a face index, -2 - sphere, -1 nothing) is one of the case's glass surfaces."""
    of_face = glass_part_of_face(c)
    out = np.zeros(obj_id.shape, bool)
    faces = obj_id >= 0
    out[faces] = of_face[obj_id[faces] % len(of_face)]
    for k in c["glass_spheres"]:
        out |= obj_id == -2 - k
    return out


# ------------------------------------------------------------------ the reference's frame --
def reference(L, orc, c, glass=None, first=False, **over) -> dict:
    """glass_ref.c's frame of case c (kept for the session; never modified by a test).  glass: render the glass surfaces (the case's
    switch when None).  over: spp, bounces, extra, glass_parts, glass_spheres, mirror_parts, mirror_spheres, thr_unorm16."""
    glass = c["glass"] if glass is None else glass
    key = ("ref", c["index"], glass, first, tuple(sorted((k, str(v)) for k, v in over.items())))
    if key not in _cache:
        extra = over.get("extra", c["extra"])
        params = orc.make_params(over.get("spp", c["spp"]), over.get("bounces", c["bounces"]), seed=c["seed"], flags=extra & pc.FLAG_NORMAL_MAP)
        _cache[key] = glass_ref.render_path(L, orc, c["cam_inv"].view(orc.CAMERA_INV_DTYPE), orc.make_screen(c["w"], c["h"]), params,
                                            c["spheres"].view(orc.SPHERE_DTYPE), c["model"], instances=c["instances"], shadows=c["shadows"],
                                            sky=c["sky_colors"] if c["sky"] else None, first=first,
                                            mirror_parts=over.get("mirror_parts", c["mirror_parts"]) if c["mirrors"] else None,
                                            mirror_spheres=over.get("mirror_spheres", c["mirror_spheres"]) if c["mirrors"] else None,
                                            glass_parts=over.get("glass_parts", c["glass_parts"]) if glass else None,
                                            glass_spheres=over.get("glass_spheres", c["glass_spheres"]) if glass else None,
                                            thr_unorm16=over.get("thr_unorm16", False))
    return _cache[key]


def forget(c):
    """Drops what the session keeps of case c, and of the path case under it (tools/fuzz_parity.py --path --glass keeps nothing)."""
    for key in [k for k in _cache if k[1] == c["index"] or k == ("case", c.get("g"))]:
        del _cache[key]
    if "g" in c:
        pc._cache.pop(("case", pc.N_CASES + c["g"]), None)


# ------------------------------------------------------------------ the product's frame --
def upload(ctx, c, glass=True):
    """path_cases.upload, with both models cleared on all RWR_MAX_SPHERES sphere slots before (the sphere attributes outlive
    rwr_scene_set_spheres) and the case's glass surfaces set after (glass=False: no glass setter is called at all).  The glass is
    set whether or not the case renders with the flag: without it it must do nothing."""
    if glass:
        for k in range(glass_ref.MAX_SPHERES):
            ctx.set_sphere_glass(k, 1.5, None)
    pc.upload(ctx, c)
    if glass:
        for k, (ior, tint) in c["glass_parts"].items():
            ctx.set_part_glass(k, ior, tint)
        for k, (ior, tint) in c["glass_spheres"].items():
            ctx.set_sphere_glass(k, ior, tint)


def frame(ctx, c, params, **kw) -> dict:
    out = pc.frame(ctx, c, params, **kw)
    out["glass"] = ctx.last_glass_stats()
    return out


def _params(rwr, c, spp=None, extra=0):
    return rwr.make_params(spp=c["spp"] if spp is None else spp, max_bounces=c["bounces"], seed=c["seed"], flags=flags(c) | extra)


def gpu_frame(rwr, c, ctx=None, glass=True) -> dict:
    """The case's frame on a context of its own (whatever RWR_WF_* the environment holds is read when it is made), or on the
    context given: one frame per frame in flight, so that every slot has rendered; all of them must be the same bytes and counts,
    the last is returned.  glass=False: a context on which no glass setter is called."""
    if ctx is None:
        with rwr.Context(0) as own:
            return gpu_frame(rwr, c, own, glass)
    upload(ctx, c, glass)
    params = _params(rwr, c)
    frames = [frame(ctx, c, params) for _ in range(c["frames_in_flight"])]
    for f in frames[:-1]:
        same(f, frames[-1], c, "frames in flight")
    return frames[-1]


def same(a, b, c, what, stats=True):
    """All five planes the same bytes, and (stats) the counts of rays, of shadow rays and of glass events."""
    pc.same(a, b, c, (what, describe(c)), stats)
    assert not stats or a["glass"] == b["glass"], (what, a["glass"], b["glass"], describe(c))


def compare(got, want, c) -> float:
    """path_cases.compare (sample-0 planes bit for bit, the ray and shadow-ray counts equal, RGBA8 within one code, float colour
    within path_cases.color_bar(c)), and the three event counts equal the reference's: (0, 0, 0) where the flag is off.  Returns the
    colour error."""
    try:
        err = pc.compare(got, want, c)
    except AssertionError as e:
        raise AssertionError(f"{e} | {describe(c)} | events {got['glass']} reference {want['events']}") from e
    assert got["glass"] == (want["events"] if c["glass"] else (0, 0, 0)), (got["glass"], want["events"], want["gen_glass"].tolist(), describe(c))
    return err


# ------------------------------------------------------------------ further contexts: accumulation, splits --
# Chosen from the list (tests/test_glass_cases_host.py asserts what they were chosen for): four flag-on cases of spp >= 2 for
# "K frames of s samples are one frame of K s" - glass on rotated instances (5, 13, 41), at B = 2, 8, 3 and 3, beside mirrors that
# reflect (13, 41, 31) - two cases for strips of two ranks, both ranks owning rows (41 on instances, 9 at B = 8, both with mirrors),
# and the block of eight rendered again with the wide per-lane kernel (cases 24 ... 31: all trace glass events, and six of them
# are the cube or its halves without a normal map, two of those under two instances - 856 world faces, as many as glass_common's
# cube_room, whose BVH tests/test_gpu_glass.py finds too large for a copy per 256-thread workgroup, so that the switch decides).
ACCUMULATION = (5, 13, 41, 31)
SPLITS = (41, 9)
WIDE_LANE_BLOCK = 3
# tests/test_gpu_glass.py's schedule that leaves every pool to the per-lane kernels, the wide one asked for
WIDE_LANE_ALONE = {"RWR_WF_GROUP": "5", "RWR_WF_PACKET_RAYS": "0", "RWR_WF_MIN_PACKET_POOLS": "100000", "RWR_WF_WIDE_LANE": "1", "RWR_WF_STATS": "1"}


# Cases of the walk beyond the committed list (tools/fuzz_parity.py --path --glass) whose colour misses the bar against the plain
# reference with every integer equal: compared against glass_ref.c's thr_unorm16 frame instead, at the unchanged bar.
# Both are the cube as glass of a high index at B = 8 with a tint channel just below 1 and local terms of 7 to 10.
ROUNDED_THROUGHPUT = (1145, 7953)


def compare_rounded(got, L, orc, c) -> tuple:
    """For a case of ROUNDED_THROUGHPUT: every integer equals the plain reference's (and the rounding moves none of them), and the
    frame is held by compare, bar unchanged, to the reference that rounds the throughput as the ray record does.  Returns (the
    colour error against that reference, the one against the plain reference)."""
    plain, rounded = reference(L, orc, c), reference(L, orc, c, thr_unorm16=True)
    for k in ("obj_id", "hit_t", "depth"):
        assert got[k].tobytes() == plain[k].tobytes(), (k, describe(c))
    assert got["stats"][1] == plain["rays"] == rounded["rays"] and got["glass"] == plain["events"] == rounded["events"], describe(c)
    against_plain = float(np.abs(got["color_f32"] - plain["color_f32"]).max())
    return compare(got, rounded, c), against_plain


def accumulated_frame(rwr, c) -> dict:
    """K frames of s samples with RWR_FLAG_ACCUMULATE on a context of its own: the last frame shown, with the K frames' event
    counts summed (an accumulating frame counts its own samples)."""
    k, s = pc.accumulation_steps(c)
    params = _params(rwr, c, spp=s, extra=pc.FLAG_ACCUMULATE)
    events = np.zeros(3, np.int64)
    with rwr.Context(0) as ctx:
        upload(ctx, c)
        ctx.accum_reset()
        for n in range(1, k + 1):
            out = frame(ctx, c, params)
            assert ctx.accum_samples() == n * s, (n, s, describe(c))
            events += np.asarray(out["glass"])
    out["glass"] = tuple(events.tolist())
    return out


def strips_frame(rwr, c, ranks=2) -> tuple:
    """The frame assembled from strips of `ranks` ranks, each rendered alone and deposited through the loopback: (the planes put
    together row by row with the summed counts, the gathered RGBA8 frame)."""
    c = dict(c, frames_in_flight=1)
    params = _params(rwr, c)
    with rwr.Context(0) as ctx:
        upload(ctx, c)
        asm, rays, shadow, events = None, 0, np.zeros(2, np.int64), np.zeros(3, np.int64)
        for r in range(ranks):
            part = frame(ctx, c, params, strips=(r, ranks))
            if asm is None:
                asm = {k: np.zeros_like(part[k]) for k in PLANES}
            rows = [y for y in range(c["h"]) if (y // 8) % ranks == r]
            for k in PLANES:
                asm[k][rows] = part[k][rows]
            rays += part["stats"][1]
            shadow += np.asarray(part["shadow"])
            events += np.asarray(part["glass"])
            ctx.dist_loopback_deposit(r, ranks, True)
        ctx.dist_loopback_finish(ranks, True)
        gathered = ctx.dist_readback()
    asm["stats"] = (c["w"] * c["h"] * c["spp"], rays)
    asm["shadow"] = tuple(shadow.tolist())
    asm["glass"] = tuple(events.tolist())
    return asm, gathered
