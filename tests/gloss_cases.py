"""The case list for glossy surfaces taken with the other path extensions (test infrastructure): tests/glass_cases.py's random
cases beyond its committed 64, with glossy surfaces drawn on top, and the directed cases that pin one rule of RWR_FLAG_GLOSSY each.

gloss_case(q, ...) is deterministic in q alone: it is glass_cases.glass_case(N_GLASS_CASES + q) as a copy - so case q has
combination q % 16 of {depth > 1, shadows, sky, mirrors} - with its glass switch set to bool(q & 16), so that q % 32 runs through
all 32 combinations of the five older switches, plus what np.random.default_rng(GLOSS_BASE + q), a generator of its own, draws:
every part and every sphere is glossy with probability P_GLOSS (at least one surface is; a glossy surface is taken out of the
case's mirror and glass dictionaries: a surface has one model), of a roughness from {2^-10, 0.05, 0.25, 0.5, 1, uniform in
[2^-10, 1]} and a reflectance per channel from {0, 1, uniform}.  RWR_FLAG_GLOSSY is on unless (q // 32) % 3 == 2: with
N_GLOSS_CASES = 96 every combination occurs twice with the flag and once with glossy surfaces set and the flag off, where gloss
must do nothing.  DIRECTED names the hand-built cases.  reference() is gloss_ref.c's frame of a case, gpu_frame() the product's,
compare() the comparison both tests/test_gpu_gloss_cases.py and tools/fuzz_parity.py --path --gloss make;
tests/test_gloss_cases_host.py asserts with the reference alone that the list exercises what the GPU file relies on.  The colour bar
is path_cases.color_bar: this file has no tolerance of its own."""
import numpy as np

import fuzz_common
import glass_cases as gc
import gloss_ref
import mirror_common
import path_cases as pc

GLOSS_BASE = 140000
N_GLOSS_CASES = 96
P_GLOSS = 0.5
FLAG_GLOSSY = 1 << 13                             # include/rwr_hip.h
ROUGHNESSES = (2.0 ** -10, 0.05, 0.25, 0.5, 1.0)  # the range's edges and values between them
PLANES = pc.PLANES

_cache = {}


# ------------------------------------------------------------------ the random cases --
def _roughness(rng) -> float:
    k = int(rng.integers(0, len(ROUGHNESSES) + 1))
    return float(ROUGHNESSES[k]) if k < len(ROUGHNESSES) else float(rng.uniform(2.0 ** -10, 1.0))


def _gloss(rng) -> tuple:
    return (_roughness(rng), pc._reflectance(rng))


def _without(items, taken) -> dict:
    return {k: v for k, v in items.items() if k not in taken}


def gloss_case(q, ref_loader, orc, cube, suzanne) -> dict:
    """Case q: glass_cases' case N_GLASS_CASES + q (a copy; the case itself is left as it is) with its glass switch overridden,
    gloss (the switch), gloss_parts and gloss_spheres ({index: (roughness, reflectance)}), and its mirror and glass dictionaries
    without the surfaces that became glossy."""
    key = ("case", q)
    if key in _cache:
        return _cache[key]
    base = gc.glass_case(gc.N_GLASS_CASES + q, ref_loader, orc, cube, suzanne)
    rng = np.random.default_rng(GLOSS_BASE + q)
    n_p, n_s = pc.n_parts(base), len(base["spheres"])
    gloss_parts = {k: _gloss(rng) for k in range(n_p) if rng.random() < P_GLOSS}
    gloss_spheres = {k: _gloss(rng) for k in range(n_s) if rng.random() < P_GLOSS}
    if not gloss_parts and not gloss_spheres:
        k = int(rng.integers(0, n_p + n_s))
        if k < n_p:
            gloss_parts = {k: _gloss(rng)}
        else:
            gloss_spheres = {k - n_p: _gloss(rng)}
    c = dict(base, index=f"gloss {q}", q=q, glass=bool(q & 16), gloss=(q // 32) % 3 != 2, gloss_parts=gloss_parts, gloss_spheres=gloss_spheres,
             mirror_parts=_without(base["mirror_parts"], gloss_parts), mirror_spheres=_without(base["mirror_spheres"], gloss_spheres),
             glass_parts=_without(base["glass_parts"], gloss_parts), glass_spheres=_without(base["glass_spheres"], gloss_spheres))
    _cache[key] = c
    return c


# ------------------------------------------------------------------ the directed cases --
def _finish(orc, c) -> dict:
    c.setdefault("gloss", True)
    c.setdefault("gloss_parts", {})
    c.setdefault("gloss_spheres", {})
    c.setdefault("glass", bool(c.get("glass_parts") or c.get("glass_spheres")))
    c.setdefault("mirrors", bool(c.get("mirror_parts") or c.get("mirror_spheres")))
    return gc._finish(orc, c)


def back_face_gloss(ref_loader, orc, cube, suzanne) -> dict:
    """n of the rule on open geometry seen from behind: glass_cases.back_face_pane's two quads in the plane z = 0 - part 0 (x < 0)
    turns its back to the eye, part 1 (x > 0) its front - both glossy at rho = 0.5, a diffuse cube behind, the sky on, B = 3.  The
    HitRecord normal of a face is turned towards the ray, so through the back face n points at the eye as it does on the front
    face: Rf and X lie on the eye's side of both quads, S = (Rf + X) / 2 is as long as the cosine of half the angle between them,
    anything in (0, 1], and no ray of either quad goes through it to the cube behind.  A rule that took the face's winding normal
    instead would send part 0's rays into the cube."""
    c = dict(gc.back_face_pane(ref_loader, orc, cube, suzanne), what="back_face_gloss", bounces=3, glass=False, glass_parts={})
    return _finish(orc, dict(c, gloss_parts={0: (0.5, (1.0, 1.0, 1.0)), 1: (0.5, (1.0, 1.0, 1.0))}))


def short_ray_chain(ref_loader, orc, cube, suzanne) -> dict:
    """A ray that is no unit vector through every kind of next hit: a glossy floor (rho = 0.5, so |S| = cos of half the angle
    between Rf and X) under a glass sphere, beside a mirror quad that leans over it, B = 8, sky and shadows on.  The floor's rays
    enter the glass, which normalises them, or are reflected by the mirror, which carries their length on (hit distances and the
    next origin P + t D scale with it) and, leaning, sends them back down to the floor, which normalises them again."""
    floor = mirror_common._quad(ref_loader, cube)
    wall = pc._quad(ref_loader, cube["texture"], [(-1.8, -1.3, -2.5), (-1.8, -1.3, 2.5), (-0.3, 1.2, 2.5), (-0.3, 1.2, -2.5)])      # its underside faces +x, -y
    return _finish(orc, dict(what="short_ray_chain", model=[floor, wall], spheres=orc.make_spheres([((0.1, -0.4, 0.0), 0.85)]), eye=(2.2, 1.4, 3.2),
                             target=(-0.3, -0.7, 0.0), w=67, h=45, spp=3, bounces=8, shadows=True, sky=True,
                             gloss_parts={0: (0.5, (0.9, 0.9, 0.8))}, mirror_parts={1: (1.0, 0.9, 0.8)}, glass_spheres={0: (1.5, (1.0, 1.0, 1.0))}))


def gloss_facing_mirror(ref_loader, orc, cube, suzanne) -> dict:
    """The RNG dimension 2 + 16 (k - 1) of a glossy hit at every generation: path_cases.facing_mirrors with the right quad glossy at
    rho = 2^-10 (the left one stays a mirror), B = 8: paths meet the glossy quad at every generation up to the eighth.  At this rho
    S is Rf moved by about 1e-3 X: a wrong dimension moves the rays by that much, and the counts with them."""
    c = pc.facing_mirrors(ref_loader, orc, cube, suzanne)
    return _finish(orc, dict(c, what="gloss_facing_mirror", mirror_parts={0: c["mirror_parts"][0]}, gloss_parts={1: (2.0 ** -10, c["mirror_parts"][1])}))


def soup_gloss_all(ref_loader, orc, cube, suzanne) -> dict:
    """Every flag at once on a soup: 129 unconnected triangles, glossy, seen from either side at h0 and at every bounce hit, with
    RWR_FLAG_NO_CULL and all six extension flags, B = 3; sphere 0 is glass, sphere 1 a mirror: all three record kinds."""
    rng = np.random.default_rng(GLOSS_BASE - 1)
    model = fuzz_common.soup(ref_loader, rng, 129, extent=1.2, tri_size=0.4, tex=suzanne["texture"])
    return _finish(orc, dict(what="soup_gloss_all", model=model, spheres=orc.make_spheres([((0.9, 0.4, 0.6), 0.5), ((-0.8, -0.5, 0.2), 0.35)]), eye=(0.3, 0.5, 3.2),
                             target=(0.0, 0.0, 0.0), w=53, h=37, spp=5, bounces=3, shadows=True, sky=True, extra=pc.FLAG_NO_CULL,
                             gloss_parts={0: (0.25, (0.9, 1.0, 0.8))}, glass_spheres={0: (1.5, (1.0, 0.9, 0.8))}, mirror_spheres={1: (0.25, 1.0, 0.8)}))


def nmap_gloss(ref_loader, orc, cube, suzanne) -> dict:
    """Normal maps shade and never steer: the two-part cube scene of path_cases.nmap_mirror with part 0 glossy and
    RWR_FLAG_NORMAL_MAP; n of the rule is the HitRecord normal, so the rays and counts are those of the frame without the map."""
    c = dict(pc.nmap_mirror(ref_loader, orc, cube, suzanne), what="nmap_gloss", w=61, h=45, mirror_parts={}, mirrors=False)
    return _finish(orc, dict(c, gloss_parts={0: (0.25, (1.0, 0.5, 0.75))}))


ALL_SPHERE_ROUGHNESSES = (2.0 ** -10, 0.05, 0.25, 0.5, 1.0, 0.01, 0.125, 0.75)


def _all_sphere_gloss(bounces):
    def build(ref_loader, orc, cube, suzanne) -> dict:
        c = dict(pc.all_sphere_mirrors(ref_loader, orc, cube, suzanne), what=f"all_sphere_gloss_b{bounces}", w=63, h=41, bounces=bounces, mirror_spheres={})
        gloss = {k: (ALL_SPHERE_ROUGHNESSES[k], (0.2 + 0.1 * k, 1.0 - 0.1 * k, 0.125 * k)) for k in range(8)}
        return _finish(orc, dict(c, gloss_spheres=gloss, mirror_parts={1: (0.9, 0.7, 0.5)}))
    build.__name__ = f"all_sphere_gloss_b{bounces}"
    build.__doc__ = """The table's records n_parts + k: eight spheres, each glossy of a roughness (both ends of the range among them) and a
    reflectance of its own, in front of a soup of two parts whose part 1 is a mirror (record 1; the spheres' records begin at 2).
    Rendered at B = 1, where every glossy ray leaves an h0 on a sphere and the primary kernel alone applies the rule, and at B = 3."""
    return build


def twin_spheres_gloss(ref_loader, orc, cube, suzanne) -> dict:
    """The nearest-hit rule's order at an exact tie: spheres 0 (glossy) and 1 (a mirror) have the same centre and radius, so every
    hit on them, at h0 and at every bounce hit, ties in t, and the order decides which model acts.  The cube stands beside them."""
    c = dict(gc.twin_spheres(ref_loader, orc, cube, suzanne), what="twin_spheres_gloss", glass=False, glass_spheres={})
    return _finish(orc, dict(c, gloss_spheres={0: (0.25, (1.0, 0.9, 0.8))}))


def bright_sky_gloss(ref_loader, orc, cube, suzanne) -> dict:
    """A reflectance <= 1 multiplied through a sky brighter than 1: a glossy sphere of reflectance (1, 0.5, 0) over a floor quad
    (mirror_common's) under a sky with components up to 2, B = 4."""
    c = dict(gc.bright_sky_tint(ref_loader, orc, cube, suzanne), what="bright_sky_gloss", glass=False, glass_spheres={})
    return _finish(orc, dict(c, gloss_spheres={0: (0.25, (1.0, 0.5, 0.0))}))


def far_gloss(ref_loader, orc, cube, suzanne) -> dict:
    """Far from the origin: path_cases.far_mirror's scene, 1e4 away on every axis, with sphere 0 glossy at rho = 0.25.  There the
    1e-4 n offset of the next origin is below an ulp of P (about 1e-3), so a glossy ray starts on its own surface, and both sides
    must meet the same self-hits."""
    c = dict(pc.far_mirror(ref_loader, orc, cube, suzanne), what="far_gloss", mirrors=False, mirror_spheres={})
    return _finish(orc, dict(c, gloss_spheres={0: (0.25, (1.0, 0.9, 0.8))}))


def rough_one(ref_loader, orc, cube, suzanne) -> dict:
    """rho = 1 sends the diffuse ray exactly: the cube (part 0, diffuse) on a floor quad (part 1, glossy at rho = 1, reflectance
    (0.8, 0.6, 0.9)), B = 3.  om = 0, so every component of S is X's: the rays, and the ray counts of every generation, are those of
    the same case with the flag off; only the throughput differs (R in place of the albedo)."""
    plain = {k: v for k, v in cube.items() if k != "normal_map"}
    return _finish(orc, dict(what="rough_one", model=[plain, mirror_common._quad(ref_loader, cube)], spheres=orc.make_spheres([]), eye=(2.3, 1.5, 3.1),
                             target=(0.0, -0.3, 0.0), w=59, h=43, spp=3, bounces=3, sky=True, gloss_parts={1: (1.0, (0.8, 0.6, 0.9))}))


def last_bit_of_s(ref_loader, orc, cube, suzanne) -> dict:
    """Every S the reference's f32 value, to the last bit: a glossy floor (rho = 0.05) under path_cases.all_sphere_mirrors' eight
    spheres, all of them mirrors of R = 1, and a second glossy quad above them, B = 8.  A mirror sphere of radius 0.5 widens the
    angle between two rays by several times at every reflection, so a last-bit difference in a glossy ray - a contracted fma in
    the blend, a reciprocal square root in place of the division - has grown by orders of magnitude when the path next meets a
    textured quad.  On scratch copies of the reference neither of the two moves a count in any entry of the list, and neither
    moves the colour of any other entry beyond its bar; here they move it by 7.7e-4 and 3.3e-4, several bars."""
    c = pc.all_sphere_mirrors(ref_loader, orc, cube, suzanne)
    floor = mirror_common._quad(ref_loader, cube, y=-1.3, half=3.0)
    roof = pc._quad(ref_loader, cube["texture"], [(-3.0, 1.9, -3.0), (3.0, 1.9, -3.0), (3.0, 1.9, 3.0), (-3.0, 1.9, 3.0)])
    return _finish(orc, dict(what="last_bit_of_s", model=[floor, roof], spheres=c["spheres"], eye=(0.3, 0.4, 4.6), target=(0.0, -0.5, 0.0), w=71, h=47, spp=4,
                             bounces=8, sky=True, gloss_parts={0: (0.05, (1.0, 0.9, 0.8)), 1: (0.05, (0.8, 0.9, 1.0))},
                             mirror_spheres={k: (1.0, 1.0, 1.0) for k in range(8)}))


DIRECTED = {f.__name__: f for f in (back_face_gloss, short_ray_chain, gloss_facing_mirror, soup_gloss_all, nmap_gloss, _all_sphere_gloss(1),
                                    _all_sphere_gloss(3), twin_spheres_gloss, bright_sky_gloss, far_gloss, rough_one, last_bit_of_s)}


def directed(name, ref_loader, orc, cube, suzanne) -> dict:
    key = ("directed", name)
    if key not in _cache:
        _cache[key] = dict(DIRECTED[name](ref_loader, orc, cube, suzanne), index=name)
    return _cache[key]


# ------------------------------------------------------------------ what a case is, in words and in numbers --
def flags(c, gloss=None) -> int:
    gloss = c["gloss"] if gloss is None else gloss
    return gc.flags(c) | (FLAG_GLOSSY if gloss else 0)


def describe(c) -> str:
    return f"{gc.describe(c)} gloss {int(c['gloss'])} (flags 0x{flags(c):x}) parts {c['gloss_parts']} spheres {c['gloss_spheres']}"


def on_gloss(c, obj_id) -> np.ndarray:
    """Whether the surface of an object id plane (a face index, -2 - sphere, -1 nothing) is one of the case's glossy surfaces."""
    return gc.on_glass(dict(c, glass_parts=c["gloss_parts"], glass_spheres=c["gloss_spheres"]), obj_id)


def h0_scatter(L, orc, c) -> list:
    """gloss_ref.scatter on the recorded h0 of every pixel-centre ray that lies on a glossy surface (a case without instances, one
    sample: the centre ray is sample 0's): (pixel, surface - the part or -2 - sphere, P, n, S) with P the hit point in float64."""
    assert c["instances"] is None
    one = reference(L, orc, c, gloss=True, spp=1)
    parts = c["model"] if isinstance(c["model"], (list, tuple)) else [c["model"]]
    scene = orc.concat_parts(list(parts))
    pos, idx = scene["vertices"]["position"], scene["faces"]["indices"]
    part_of = np.concatenate([np.full(len(p["faces"]), k) for k, p in enumerate(parts)])
    cam, screen = c["cam_inv"].view(orc.CAMERA_INV_DTYPE), orc.make_screen(c["w"], c["h"])
    out = []
    for y, x in zip(*np.nonzero(on_gloss(c, one["obj_id"]))):
        o, d, _ = orc.pixel_to_ray(cam, screen, int(x), int(y))
        i = int(one["obj_id"][y, x])
        if i >= 0:
            hit, t, n, _ = orc.triangle_ray_intersect(*[pos[v] for v in idx[i]], o, d)
            surface, rho = int(part_of[i]), c["gloss_parts"][int(part_of[i])][0]
        else:
            s = c["spheres"].view(orc.SPHERE_DTYPE)[-2 - i]
            hit, t, n = orc.sphere_ray_intersect(s["center"], float(s["radius"]), o, d)
            surface, rho = i, c["gloss_spheres"][-2 - i][0]
        assert hit and np.float32(t) == one["hit_t"][y, x], (x, y, t, one["hit_t"][y, x])
        pixel = int(y) * c["w"] + int(x)
        S, _ = gloss_ref.scatter(L, n, d, gloss_ref.roughness_of(rho), pixel, 0, 2, c["seed"])
        out.append((pixel, surface, o.astype(np.float64) + float(t) * d.astype(np.float64), n, S))
    return out


# ------------------------------------------------------------------ the reference's frame --
def reference(L, orc, c, gloss=None, use_glass_ref=False, **over) -> dict:
    """gloss_ref.c's frame of case c (kept for the session; never modified by a test).  gloss: render the glossy surfaces (the
    case's switch when None).  over: spp, bounces, extra, gloss_parts, gloss_spheres, glass_parts, glass_spheres, mirror_parts,
    mirror_spheres, thr_unorm16."""
    gloss = c["gloss"] if gloss is None else gloss
    key = ("ref", c["index"], gloss, use_glass_ref, tuple(sorted((k, str(v)) for k, v in over.items())))
    if key not in _cache:
        extra = over.get("extra", c["extra"])
        params = orc.make_params(over.get("spp", c["spp"]), over.get("bounces", c["bounces"]), seed=c["seed"], flags=extra & pc.FLAG_NORMAL_MAP)
        _cache[key] = gloss_ref.render_path(L, orc, c["cam_inv"].view(orc.CAMERA_INV_DTYPE), orc.make_screen(c["w"], c["h"]), params,
                                            c["spheres"].view(orc.SPHERE_DTYPE), c["model"], instances=c["instances"], shadows=c["shadows"],
                                            sky=c["sky_colors"] if c["sky"] else None,
                                            mirror_parts=over.get("mirror_parts", c["mirror_parts"]) if c["mirrors"] else None,
                                            mirror_spheres=over.get("mirror_spheres", c["mirror_spheres"]) if c["mirrors"] else None,
                                            glass_parts=over.get("glass_parts", c["glass_parts"]) if c["glass"] else None,
                                            glass_spheres=over.get("glass_spheres", c["glass_spheres"]) if c["glass"] else None,
                                            gloss_parts=over.get("gloss_parts", c["gloss_parts"]) if gloss else None,
                                            gloss_spheres=over.get("gloss_spheres", c["gloss_spheres"]) if gloss else None,
                                            use_glass_ref=use_glass_ref, thr_unorm16=over.get("thr_unorm16", False))
    return _cache[key]


def forget(c):
    """Drops what the session keeps of case c, and of the glass and path cases under it (tools/fuzz_parity.py --path --gloss keeps
    nothing)."""
    for key in [k for k in _cache if k[1] == c["index"] or k == ("case", c.get("q"))]:
        del _cache[key]
    if "q" in c:
        gc.forget(dict(c, index=f"glass {c['g']}"))


# ------------------------------------------------------------------ the product's frame --
def upload(ctx, c, gloss=True):
    """glass_cases.upload, with all three models cleared on all RWR_MAX_SPHERES sphere slots before (the sphere attributes outlive
    rwr_scene_set_spheres) and the case's glossy surfaces set after (gloss=False: no gloss setter is called at all).  The gloss is
    set whether or not the case renders with the flag: without it it must do nothing."""
    if gloss:
        for k in range(gloss_ref.MAX_SPHERES):
            ctx.set_sphere_gloss(k, 0.5, None)
    gc.upload(ctx, c)
    if gloss:
        for k, (rough, refl) in c["gloss_parts"].items():
            ctx.set_part_gloss(k, rough, refl)
        for k, (rough, refl) in c["gloss_spheres"].items():
            ctx.set_sphere_gloss(k, rough, refl)


def frame(ctx, c, params, **kw) -> dict:
    out = gc.frame(ctx, c, params, **kw)
    out["glossy"] = ctx.last_gloss_stats()
    return out


def _params(rwr, c, spp=None, extra=0, gloss=None):
    return rwr.make_params(spp=c["spp"] if spp is None else spp, max_bounces=c["bounces"], seed=c["seed"], flags=flags(c, gloss) | extra)


def gpu_frame(rwr, c, ctx=None, gloss=True, flag=None) -> dict:
    """The case's frame on a context of its own (whatever RWR_WF_* the environment holds is read when it is made), or on the
    context given: one frame per frame in flight, so that every slot has rendered; all of them must be the same bytes and counts,
    the last is returned.  gloss=False: a context on which no gloss setter is called.  flag: RWR_FLAG_GLOSSY (the case's switch
    when None)."""
    if ctx is None:
        with rwr.Context(0) as own:
            return gpu_frame(rwr, c, own, gloss, flag)
    upload(ctx, c, gloss)
    params = _params(rwr, c, gloss=flag)
    frames = [frame(ctx, c, params) for _ in range(c["frames_in_flight"])]
    for f in frames[:-1]:
        same(f, frames[-1], c, "frames in flight")
    return frames[-1]


def same(a, b, c, what, stats=True):
    """All five planes the same bytes, and (stats) the counts of rays, of shadow rays, of glass events and of glossy rays."""
    gc.same(a, b, c, what, stats)
    assert not stats or a["glossy"] == b["glossy"], (what, a["glossy"], b["glossy"], describe(c))


def compare(got, want, c) -> float:
    """glass_cases.compare (sample-0 planes bit for bit, the ray, shadow-ray and glass event counts equal, RGBA8 within one code,
    float colour within path_cases.color_bar(c)), and the glossy-ray count equals the reference's: 0 where the flag is off.  Returns
    the colour error."""
    try:
        err = gc.compare(got, want, c)
    except AssertionError as e:
        raise AssertionError(f"{e} | {describe(c)} | glossy rays {got['glossy']} reference {want['glossy']}") from e
    assert got["glossy"] == (want["glossy"] if c["gloss"] else 0), (got["glossy"], want["glossy"], want["gen_gloss"].tolist(), describe(c))
    return err


# ------------------------------------------------------------------ further contexts: accumulation, splits --
# Chosen from the list (tests/test_gloss_cases_host.py asserts what they were chosen for): four flag-on cases of spp >= 2 for "K
# frames of s samples are one frame of K s" - a glossy part on rotated instances under a normal map and RWR_FLAG_NO_CULL at B = 8
# (5) and with every flag at B = 3 (63), and two frames with glossy rays, glass events and mirror reflections at B = 8 and 2 (27,
# 57) - two cases for strips of two ranks, glossy surfaces at h0 in both ranks' rows and glossy rays at generation 2 (25 at B = 8
# beside glass, 41 on instances beside mirrors), and the block of eight rendered again with the wide per-lane kernel (cases 24 ...
# 31: the mirror and the glass flag on in all of them, all trace glossy rays, two are the cube under two instances without a
# normal map - 856 world faces, whose BVH tests/test_gpu_glass.py finds too large for a copy per 256-thread workgroup).  The cases
# rendered again under the forced schedule are the first and the last of every block of eight: q % 8 == 0 has none of {depth > 1,
# shadows, sky}, q % 8 == 7 all three.
ACCUMULATION = (5, 27, 63, 57)
SPLITS = (25, 41)
WIDE_LANE_BLOCK = 3
FORCED = (0, 7)
WIDE_LANE_ALONE = gc.WIDE_LANE_ALONE

# Cases whose colour misses the bar against the plain reference with every integer equal: compared against gloss_ref.c's
# thr_unorm16 frame instead, at the unchanged bar, exactly as glass_cases.ROUNDED_THROUGHPUT.  No committed entry is
# one; the walk beyond the list (tools/fuzz_parity.py --path --gloss) met glass_cases' own: gloss case q lies on glass case 64 + q.
ROUNDED_THROUGHPUT = (1081,)


def compare_rounded(got, L, orc, c) -> tuple:
    """For a case of ROUNDED_THROUGHPUT: every integer equals the plain reference's (and the rounding moves none of them), and the
    frame is held by compare, bar unchanged, to the reference that rounds the throughput as the ray record does.  Returns (the
    colour error against that reference, the one against the plain reference)."""
    plain, rounded = reference(L, orc, c), reference(L, orc, c, thr_unorm16=True)
    for k in ("obj_id", "hit_t", "depth"):
        assert got[k].tobytes() == plain[k].tobytes(), (k, describe(c))
    assert got["stats"][1] == plain["rays"] == rounded["rays"] and got["glass"] == plain["events"] == rounded["events"], describe(c)
    assert got["glossy"] == (plain["glossy"] if c["gloss"] else 0) and plain["glossy"] == rounded["glossy"], describe(c)
    against_plain = float(np.abs(got["color_f32"] - plain["color_f32"]).max())
    return compare(got, rounded, c), against_plain


def accumulated_frame(rwr, c) -> dict:
    """K frames of s samples with RWR_FLAG_ACCUMULATE on a context of its own: the last frame shown, with the K frames' glass
    event and glossy-ray counts summed (an accumulating frame counts its own samples)."""
    k, s = pc.accumulation_steps(c)
    params = _params(rwr, c, spp=s, extra=pc.FLAG_ACCUMULATE)
    events, glossy = np.zeros(3, np.int64), 0
    with rwr.Context(0) as ctx:
        upload(ctx, c)
        ctx.accum_reset()
        for n in range(1, k + 1):
            out = frame(ctx, c, params)
            assert ctx.accum_samples() == n * s, (n, s, describe(c))
            events += np.asarray(out["glass"])
            glossy += out["glossy"]
    out["glass"] = tuple(events.tolist())
    out["glossy"] = glossy
    return out


def strips_frame(rwr, c, ranks=2) -> tuple:
    """The frame assembled from strips of `ranks` ranks, each rendered alone and deposited through the loopback: (the planes put
    together row by row with the summed counts, the gathered RGBA8 frame)."""
    c = dict(c, frames_in_flight=1)
    params = _params(rwr, c)
    with rwr.Context(0) as ctx:
        upload(ctx, c)
        asm, rays, shadow, events, glossy = None, 0, np.zeros(2, np.int64), np.zeros(3, np.int64), 0
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
            glossy += part["glossy"]
            ctx.dist_loopback_deposit(r, ranks, True)
        ctx.dist_loopback_finish(ranks, True)
        gathered = ctx.dist_readback()
    asm["stats"] = (c["w"] * c["h"] * c["spp"], rays)
    asm["shadow"] = tuple(shadow.tolist())
    asm["glass"] = tuple(events.tolist())
    asm["glossy"] = glossy
    return asm, gathered
