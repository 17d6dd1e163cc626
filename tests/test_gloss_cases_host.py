"""tests/gloss_cases.py's list, host side: with the CPU reference alone (gloss_ref.c) the conditions the GPU file,
tests/test_gpu_gloss_cases.py, relies on - conditions on the inputs, not measurements: the list is deterministic and stratified,
enough cases have glossy rays in every setting (at generation 1 and after it, beside glass and mirrors, on rotated instances, under
normal maps and RWR_FLAG_NO_CULL, at many samples and at B = 8), every directed case does what it was built for, and the cases
chosen for the further checks trace glossy rays.  If a draw misses a condition the draw is changed (GLOSS_BASE, the probabilities),
not the threshold.  No GPU.  The counts found and the file's total time are printed."""
import time

import numpy as np
import pytest

import glass_cases as gc
import gloss_cases as sc
import gloss_ref
import path_cases as pc

ON = range(64)            # RWR_FLAG_GLOSSY on
OFF = range(64, 96)       # glossy surfaces set, the flag off
COUNTS = ("events", "multi", "deep", "rays", "shadow_rays", "occluded", "sky_terms", "glossy")
GENS = ("gen_rays", "gen_mirror", "gen_glass", "gen_gloss")


@pytest.fixture(scope="module", autouse=True)
def started():
    """When this file's first test began."""
    return time.perf_counter()


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return gloss_ref.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def cases(ref_loader, orc, cube, suzanne):
    return [sc.gloss_case(q, ref_loader, orc, cube, suzanne) for q in range(sc.N_GLOSS_CASES)]


@pytest.fixture(scope="module")
def refs(sref, orc, cases):
    """Every case rendered with its gloss, the flag-off cases too (their own reference, without gloss, is in `plain`)."""
    return [sc.reference(sref, orc, c, gloss=True) for c in cases]


@pytest.fixture(scope="module")
def plain(sref, orc, cases):
    return [sc.reference(sref, orc, c, gloss=False) for c in cases]


def _directed(name, ref_loader, orc, cube, suzanne):
    return sc.directed(name, ref_loader, orc, cube, suzanne)


def _surfaces(c):
    return list(c["gloss_parts"].values()) + list(c["gloss_spheres"].values())


def _same_counts(a, b, what):
    for k in COUNTS:
        assert a[k] == b[k], (k, what)
    for k in GENS:
        assert np.array_equal(a[k], b[k]), (k, what)


def test_the_list_is_deterministic_and_stratified(ref_loader, orc, cube, suzanne, cases):
    assert sc.N_GLOSS_CASES == 96 and len(sc.DIRECTED) == 12
    combos = {}
    for c in cases:
        q = c["q"]
        base = gc.glass_case(gc.N_GLASS_CASES + q, ref_loader, orc, cube, suzanne)
        assert (c["multi"], c["shadows"], c["sky"], c["mirrors"], c["glass"]) == (bool(q & 1), bool(q & 2), bool(q & 4), bool(q & 8), bool(q & 16)), q
        assert c["gloss"] == (q // 32 != 2) and base["glass"] and c["g"] == base["g"] == gc.N_GLASS_CASES + q
        assert sc.flags(c) == pc.flags(base) | (gc.FLAG_GLASS if c["glass"] else 0) | (sc.FLAG_GLOSSY if c["gloss"] else 0)
        combos[(q % 32, c["gloss"])] = combos.get((q % 32, c["gloss"]), 0) + 1
        # at least one glossy surface, every key in range, no surface with two models, and the cases under it untouched
        assert c["gloss_parts"] or c["gloss_spheres"]
        assert all(0 <= k < pc.n_parts(c) for k in c["gloss_parts"]) and all(0 <= k < len(c["spheres"]) for k in c["gloss_spheres"])
        for a, b in (("gloss_parts", "mirror_parts"), ("gloss_parts", "glass_parts"), ("glass_parts", "mirror_parts"),
                     ("gloss_spheres", "mirror_spheres"), ("gloss_spheres", "glass_spheres"), ("glass_spheres", "mirror_spheres")):
            assert not set(c[a]) & set(c[b]), (a, b, q)
        for k in ("mirror_parts", "glass_parts"):
            assert c[k] == {i: v for i, v in base[k].items() if i not in c["gloss_parts"]}, (k, q)
        for k in ("mirror_spheres", "glass_spheres"):
            assert c[k] == {i: v for i, v in base[k].items() if i not in c["gloss_spheres"]}, (k, q)
        assert "gloss_parts" not in base and c is not base and c["cam_inv"] is base["cam_inv"] and c["model"] is base["model"]
        for rough, refl in _surfaces(c):
            assert 2.0 ** -10 <= rough <= 1.0 and len(refl) == 3 and all(0.0 <= v <= 1.0 for v in refl)
    assert combos == {(k, on): (2 if on else 1) for k in range(32) for on in (True, False)}
    # a case is rebuilt from its index alone: the gloss generator is the case's own, the generators under it are not drawn from
    kept = cases[5]
    sc._cache.pop(("case", 5))
    gc._cache.pop(("case", gc.N_GLASS_CASES + 5))
    pc._cache.pop(("case", pc.N_CASES + gc.N_GLASS_CASES + 5))
    again = sc.gloss_case(5, ref_loader, orc, cube, suzanne)
    assert again is not kept and sc.describe(again) == sc.describe(kept)
    assert again["cam_inv"].tobytes() == kept["cam_inv"].tobytes() and again["spheres"].tobytes() == kept["spheres"].tobytes()
    for k in ("gloss_parts", "gloss_spheres", "glass_parts", "glass_spheres", "mirror_parts", "mirror_spheres"):
        assert again[k] == kept[k], k
    sc._cache[("case", 5)] = kept
    # the old lists are what they were: their cases carry no gloss and keep their indices
    assert pc.N_CASES == 64 and gc.N_GLASS_CASES == 64
    assert "gloss_parts" not in pc.case(5, ref_loader, orc, cube, suzanne) and "gloss_parts" not in gc.glass_case(5, ref_loader, orc, cube, suzanne)
    assert gc.glass_case(5, ref_loader, orc, cube, suzanne)["glass"] and not gc.glass_case(48, ref_loader, orc, cube, suzanne)["glass"]
    # every listed roughness and a uniform one occur, and every kind of reflectance
    roughs = {rough for c in cases for rough, _ in _surfaces(c)}
    assert set(sc.ROUGHNESSES) <= roughs and any(v not in sc.ROUGHNESSES for v in roughs)
    refls = {v for c in cases for _, t in _surfaces(c) for v in t}
    assert {0.0, 1.0} <= refls and any(0.0 < v < 1.0 for v in refls)
    # frames no larger than the old lists', and none of the directed ones a multiple of the 64 x 8 tile
    assert all(c["w"] <= 80 and c["h"] <= 56 and c["spp"] <= 65 for c in cases)
    for name in sc.DIRECTED:
        d = _directed(name, ref_loader, orc, cube, suzanne)
        assert d["w"] <= 72 and d["h"] <= 48 and d["spp"] <= 5 and (d["w"] % 64 != 0 or d["h"] % 8 != 0), name
        if name in ("soup_gloss_all", "all_sphere_gloss_b1", "all_sphere_gloss_b3"):
            assert pc.n_base_faces(d) <= 300, name
        assert d["gloss"] and sc.DIRECTED[name].__doc__, name
        assert not set(d["gloss_parts"]) & (set(d["mirror_parts"]) | set(d["glass_parts"])), name
        assert not set(d["gloss_spheres"]) & (set(d["mirror_spheres"]) | set(d["glass_spheres"])), name


@pytest.mark.parametrize("q", (3, 9, 27, 57, 63, 91))
def test_without_gloss_it_is_the_glass_reference(sref, orc, cases, q):
    """gloss_render_path without a glossy record equals glass_render_path in every byte and count: the flag-off cases' reference
    is the frame of a reference that never heard of gloss."""
    c = cases[q]
    got = sc.reference(sref, orc, c, gloss=False)
    want = sc.reference(sref, orc, c, gloss=False, use_glass_ref=True)
    for k in sc.PLANES:
        assert got[k].tobytes() == want[k].tobytes(), (k, sc.describe(c))
    for k in COUNTS[:-1]:
        assert got[k] == want[k], (k, sc.describe(c))
    for k in GENS[:-1]:
        assert np.array_equal(got[k], want[k]), (k, sc.describe(c))
    assert got["glossy"] == 0 and want["rays"] > 0


def test_the_cases_exercise_the_gloss(sref, orc, cases, refs):
    """The minimum number of flag-on cases per condition: each has roughly a factor of two of slack against the draw."""
    on = [(cases[q], refs[q]) for q in ON]
    rays = lambda r: r["glossy"] > 0       # noqa: E731
    parts_alone = {c["q"]: sc.reference(sref, orc, c, gloss_spheres={})["glossy"] if c["gloss_parts"] else 0 for c, r in on}
    spheres_alone = {c["q"]: sc.reference(sref, orc, c, gloss_parts={})["glossy"] if c["gloss_spheres"] else 0 for c, r in on}
    found = {
        "glossy rays": (sum(rays(r) for c, r in on), 30),
        "glossy rays at generation 1 (the primary kernel's)": (sum(r["gen_gloss"][1] > 0 for c, r in on), 30),
        "glossy rays at generations >= 2 (the trace kernels')": (sum(r["gen_gloss"][2:].sum() > 0 for c, r in on), 13),
        "glossy rays and glass events": (sum(rays(r) and sum(r["events"]) > 0 for c, r in on), 8),
        "glossy rays and mirror reflections": (sum(rays(r) and r["gen_mirror"].sum() > 0 for c, r in on), 5),
        "glossy rays, glass events and mirror reflections": (sum(rays(r) and sum(r["events"]) > 0 and r["gen_mirror"].sum() > 0 for c, r in on), 2),
        "glossy rays from parts alone, on rotated instances": (sum(parts_alone[c["q"]] > 0 and c["instances"] is not None for c, r in on), 8),
        "glossy rays from parts alone": (sum(v > 0 for v in parts_alone.values()), 20),
        "glossy rays from spheres alone": (sum(v > 0 for v in spheres_alone.values()), 15),
        "glossy rays under RWR_FLAG_NORMAL_MAP": (sum(rays(r) and bool(c["extra"] & pc.FLAG_NORMAL_MAP) for c, r in on), 7),
        "glossy rays under RWR_FLAG_NO_CULL": (sum(rays(r) and bool(c["extra"] & pc.FLAG_NO_CULL) for c, r in on), 6),
        "glossy rays at 33 or 65 samples": (sum(rays(r) and c["spp"] in (33, 65) for c, r in on), 2),
        "glossy rays at B = 8": (sum(rays(r) and c["bounces"] == 8 for c, r in on), 6),
        "glossy rays at generation 8": (sum(c["bounces"] == 8 and r["gen_gloss"][8] > 0 for c, r in on), 3),
        "glossy rays with shadows": (sum(rays(r) and c["shadows"] for c, r in on), 15),
        "glossy rays with the sky": (sum(rays(r) and c["sky"] for c, r in on), 15),
        "glossy rays with the sky and without shadows (a launch bound of its own)": (sum(rays(r) and c["sky"] and not c["shadows"] and c["bounces"] > 1 for c, r in on), 3),
    }
    for what, (n, least) in found.items():
        print(f"gloss cases with {what}: {n} of {len(on)} (at least {least})")
    print(f"glossy rays of the {len(on)} flag-on cases: {sum(r['glossy'] for c, r in on)}, per generation "
          f"{[int(sum(r['gen_gloss'][k] for c, r in on if len(r['gen_gloss']) > k)) for k in range(1, 9)]}")
    for what, (n, least) in found.items():
        assert n >= least, (what, n, least)
    # the range's edges, exactly, on surfaces of cases that have glossy rays
    for edge in (2.0 ** -10, 1.0):
        assert any(rays(r) and any(rough == edge for rough, _ in _surfaces(c)) for c, r in on), edge
    # on an instance case the glossy part's rays come from later instances too: h0 on a glossy face of instance >= 1
    later = sum(c["instances"] is not None and bool((sc.on_gloss(c, r["obj_id"]) & (r["obj_id"] >= pc.n_base_faces(c))).any()) for c, r in on)
    print(f"gloss cases whose sample-0 plane shows a glossy face of a later instance: {later}")
    assert later >= 5


def test_flag_off_cases_could_fail(cases, refs, plain):
    """Without the flag the reference has no glossy ray; with the flag forced on every one of these cases has some, and its frame
    differs: the switch has something to switch."""
    differ = 0
    for q in OFF:
        assert not cases[q]["gloss"] and plain[q]["glossy"] == 0 and plain[q]["gen_gloss"].sum() == 0
        assert refs[q]["glossy"] > 0, sc.describe(cases[q])
        differ += not np.array_equal(refs[q]["color_f32"], plain[q]["color_f32"])
    print(f"flag-off cases with glossy rays when the flag is forced on: {len(OFF)} of {len(OFF)}; whose frame would differ: {differ} (at least 16)")
    assert differ >= 16


def test_reference_invariants(sref, orc, cases, refs, plain):
    """What makes the counts meaningful: at max_bounces = 1 every sample whose h0 lies on a glossy surface is one glossy ray and
    nothing else is; sample-0 planes and generation 1's ray count do not depend on the gloss; the reflectance steers nothing."""
    h0_rays = 0
    for q in ON:
        c, r = cases[q], refs[q]
        one = sc.reference(sref, orc, c, spp=1, bounces=1)
        n = int(sc.on_gloss(c, one["obj_id"]).sum())
        assert one["glossy"] == n == one["gen_gloss"][1], (one["glossy"], n, sc.describe(c))
        h0_rays += n
        for k in ("obj_id", "hit_t", "depth"):
            assert r[k].tobytes() == plain[q][k].tobytes(), (k, sc.describe(c))
        assert r["gen_rays"][1] == plain[q]["gen_rays"][1]
        black = sc.reference(sref, orc, c, gloss_parts={k: (v, (0.0, 0.0, 0.0)) for k, (v, _) in c["gloss_parts"].items()},
                             gloss_spheres={k: (v, (0.0, 0.0, 0.0)) for k, (v, _) in c["gloss_spheres"].items()})
        _same_counts(black, r, sc.describe(c))
    print(f"samples whose h0 lies on a glossy surface, one per pixel over the 64 flag-on cases: {h0_rays}")
    assert h0_rays > 2000


# ------------------------------------------------------------------ the directed cases --
def _lengths(hits):
    return np.array([np.linalg.norm(S.astype(np.float64)) for _, _, _, _, S in hits])


def test_back_face_gloss(sref, orc, ref_loader, cube, suzanne):
    c = _directed("back_face_gloss", ref_loader, orc, cube, suzanne)
    r = sc.reference(sref, orc, c)
    back = sc.reference(sref, orc, c, gloss_parts={0: c["gloss_parts"][0]})
    front = sc.reference(sref, orc, c, gloss_parts={1: c["gloss_parts"][1]})
    assert c["bounces"] == 3 and c["sky"] and pc.n_parts(c) == 3 and set(c["gloss_parts"]) == {0, 1} and all(v[0] == 0.5 for v in c["gloss_parts"].values())
    assert back["gen_gloss"][1] > 500 and front["gen_gloss"][1] > 500 and back["gen_gloss"][1] + front["gen_gloss"][1] == r["gen_gloss"][1]
    # the rule on the recorded h0 of the centre rays: part 0 is seen from behind (its winding normal is -z and the eye at z > 0), n is
    # turned towards the eye on both parts, S stays on n's side and is shorter than one
    hits = sc.h0_scatter(sref, orc, c)
    eye = np.asarray(c["eye"], np.float64)
    for part in (0, 1):
        mine = [h for h in hits if h[1] == part]
        assert len(mine) > 200
        assert all(float(n.astype(np.float64) @ (eye - P)) > 0 and n[2] == 1.0 for _, _, P, n, _ in mine)
        assert all(float(S.astype(np.float64) @ n.astype(np.float64)) > 0 for _, _, _, n, S in mine)
    ln = _lengths(hits)
    print(f"back_face_gloss: glossy rays per generation {r['gen_gloss'][1:].tolist()} (the back-facing quad alone {back['gen_gloss'][1:].tolist()}); "
          f"|S| of {len(hits)} centre rays from {ln.min():.3f} to {ln.max():.3f}, {int((ln < 0.9).sum())} below 0.9")
    assert ln.max() <= 1.0 + 1e-6 and ln.min() < 0.75 and (ln < 0.9).sum() > 100
    assert r["gen_rays"][2] > 0 and r["sky_terms"] > 0            # the rays go on: into the sky, and from the cube's hits onto the quads' far side


def test_short_ray_chain(sref, orc, ref_loader, cube, suzanne):
    c = _directed("short_ray_chain", ref_loader, orc, cube, suzanne)
    r = sc.reference(sref, orc, c)
    assert c["bounces"] == 8 and c["sky"] and c["shadows"] and c["glass"] and c["mirrors"] and c["gloss_parts"][0][0] == 0.5
    assert list(c["mirror_parts"]) == [1] and list(c["glass_spheres"]) == [0]
    # the floor's generation-1 rays, from the rule on the recorded h0: shorter than one, and where they go next
    hits = [h for h in sc.h0_scatter(sref, orc, c) if h[1] == 0]
    ln = _lengths(hits)
    sphere = c["spheres"].view(orc.SPHERE_DTYPE)[0]
    wall = c["model"][1]
    tris = [[wall["vertices"]["position"][v] for v in f] for f in wall["faces"]["indices"]]
    into_glass = onto_mirror = back_down = 0
    for (_, _, P, n, S), length in zip(hits, ln):
        o = (P + 1e-4 * n.astype(np.float64)).astype(np.float32)
        if length < 0.95:
            into_glass += orc.sphere_ray_intersect(sphere["center"], float(sphere["radius"]), o, S)[0]
            met = [h for h in (orc.triangle_ray_intersect(*t, o, S) for t in tris) if h[0]]
            onto_mirror += bool(met)
            back_down += any(float(S[1] - 2.0 * (m[2] @ S) * m[2][1]) < 0.0 for m in met)       # the mirror's ray, |S| long, points at the floor
    print(f"short_ray_chain: |S| of {len(hits)} floor rays from {ln.min():.3f} to {ln.max():.3f}; of those below 0.95, {into_glass} point into the glass "
          f"sphere and {onto_mirror} onto the mirror, which sends {back_down} back down; glossy rays per generation {r['gen_gloss'][1:].tolist()}, "
          f"glass events {r['gen_glass'][1:].tolist()}, mirror reflections {r['gen_mirror'][1:].tolist()}")
    assert len(hits) > 300 and ln.min() < 0.75 and into_glass >= 10 and onto_mirror >= 20 and back_down >= 20
    # ... and the frame's counts: glass events and mirror reflections in the generations after a glossy one, glossy rays after those
    without = sc.reference(sref, orc, c, gloss=False)
    assert r["gen_glass"][2:].sum() > 0 and r["gen_mirror"][2:].sum() > 0 and r["gen_gloss"][3:].sum() > 0
    assert not np.array_equal(r["gen_glass"][2:], without["gen_glass"][2:]) and not np.array_equal(r["gen_mirror"][2:], without["gen_mirror"][2:])
    assert r["gen_rays"][8] > 0 and 0 < r["occluded"] < r["shadow_rays"] and r["sky_terms"] > 0


def test_gloss_facing_mirror(sref, orc, ref_loader, cube, suzanne):
    c = _directed("gloss_facing_mirror", ref_loader, orc, cube, suzanne)
    r = sc.reference(sref, orc, c)
    print(f"gloss_facing_mirror: glossy rays per generation {r['gen_gloss'][1:].tolist()}, mirror reflections {r['gen_mirror'][1:].tolist()}")
    assert c["bounces"] == 8 and c["gloss_parts"][1][0] == 2.0 ** -10 and set(c["mirror_parts"]) == {0}
    assert r["gen_gloss"][8] > 0 and (r["gen_gloss"][1:] > 0).sum() >= 7 and r["gen_mirror"][7] > 0
    # at this roughness S lies about rho from Rf: a wrong X moves it by that much and no more
    S, rf = gloss_ref.scatter(sref, (0.0, 0.0, 1.0), (0.6, 0.0, -0.8), gloss_ref.roughness_of(2.0 ** -10), pixel=7, sample=1, dim=2 + 16 * 7, seed=c["seed"])
    other, _ = gloss_ref.scatter(sref, (0.0, 0.0, 1.0), (0.6, 0.0, -0.8), gloss_ref.roughness_of(2.0 ** -10), pixel=7, sample=1, dim=3 + 16 * 7, seed=c["seed"])
    assert 1e-5 < float(np.abs(S - other).max()) < 2.5e-3 and float(np.abs(S - rf).max()) < 2.5e-3


def test_soup_gloss_all(sref, orc, ref_loader, cube, suzanne):
    c = _directed("soup_gloss_all", ref_loader, orc, cube, suzanne)
    r = sc.reference(sref, orc, c)
    assert sc.flags(c) == (pc.FLAG_AUX_OUTPUTS | pc.FLAG_NO_CULL | pc.FLAG_MULTI_BOUNCE | pc.FLAG_SHADOWS | pc.FLAG_SKY | pc.FLAG_MIRRORS | gc.FLAG_GLASS |
                           sc.FLAG_GLOSSY)
    assert pc.n_base_faces(c) == 129 and c["bounces"] == 3 and len(c["spheres"]) == 2 and list(c["mirror_spheres"]) == [1] and list(c["glass_spheres"]) == [0]
    assert (r["gen_gloss"][1:] > 0).all() and (r["gen_glass"][1:] > 0).all() and (r["gen_mirror"][1:] > 0).all()
    assert r["sky_terms"] > 0 and 0 < r["occluded"] < r["shadow_rays"]


def test_nmap_gloss(sref, orc, ref_loader, cube, suzanne):
    c = _directed("nmap_gloss", ref_loader, orc, cube, suzanne)
    assert c["extra"] & pc.FLAG_NORMAL_MAP and list(c["gloss_parts"]) == [0] and not c["mirror_parts"] and not c["mirrors"] and not c["glass"]
    r = sc.reference(sref, orc, c)
    flat = sc.reference(sref, orc, c, extra=0)
    _same_counts(r, flat, "normal maps never change n")
    assert r["gen_gloss"][2] > 0 and not np.array_equal(r["color_f32"], flat["color_f32"])


def test_all_sphere_gloss(sref, orc, ref_loader, cube, suzanne):
    one = _directed("all_sphere_gloss_b1", ref_loader, orc, cube, suzanne)
    three = _directed("all_sphere_gloss_b3", ref_loader, orc, cube, suzanne)
    assert one["bounces"] == 1 and three["bounces"] == 3 and sc.describe(dict(one, bounces=3, what="", index="")) == sc.describe(dict(three, what="", index=""))
    assert pc.n_parts(one) == 2 and len(one["spheres"]) == 8 and list(one["mirror_parts"]) == [1]
    roughs = {v[0] for v in one["gloss_spheres"].values()}
    assert len(roughs) == 8 and {2.0 ** -10, 1.0} <= roughs and len({v[1] for v in one["gloss_spheres"].values()}) == 8
    r = sc.reference(sref, orc, one)
    assert {-2 - k for k in range(8)} <= set(np.unique(r["obj_id"]).tolist())                         # every sphere id at h0
    per_sample = sc.reference(sref, orc, one, spp=1)
    assert per_sample["glossy"] == int((per_sample["obj_id"] <= -2).sum()) > 0                        # B = 1: a glossy ray per h0 on a sphere
    assert r["gen_mirror"][1] > 0 and r["glossy"] == r["gen_gloss"][1]
    deep = sc.reference(sref, orc, three)
    assert deep["gen_gloss"][1] == r["gen_gloss"][1] and deep["gen_gloss"][2] > 0 and deep["gen_gloss"][3] > 0 and deep["gen_mirror"][2] > 0


def test_twin_spheres_gloss(sref, orc, ref_loader, cube, suzanne):
    c = _directed("twin_spheres_gloss", ref_loader, orc, cube, suzanne)
    assert c["spheres"][0].tobytes() == c["spheres"][1].tobytes() and list(c["gloss_spheres"]) == [0] and list(c["mirror_spheres"]) == [1] and c["mirrors"]
    r = sc.reference(sref, orc, c)
    swapped = sc.reference(sref, orc, c, gloss_spheres={1: c["gloss_spheres"][0]}, mirror_spheres={0: c["mirror_spheres"][1]})
    print(f"twin_spheres_gloss: glossy rays {r['glossy']}, mirror reflections {int(r['gen_mirror'].sum())}, rays {r['gen_rays'][1:].tolist()}; "
          f"swapped {swapped['glossy']}, {int(swapped['gen_mirror'].sum())}, {swapped['gen_rays'][1:].tolist()}")
    assert r["glossy"] > 0 and r["gen_mirror"].sum() == 0 and swapped["glossy"] == 0 and swapped["gen_mirror"].sum() > 0      # the tie matters
    assert r["rays"] != swapped["rays"]
    assert r["obj_id"].tobytes() == swapped["obj_id"].tobytes() and (r["obj_id"] == -2).any() and not (r["obj_id"] == -3).any()


def test_bright_sky_gloss(sref, orc, ref_loader, cube, suzanne):
    c = _directed("bright_sky_gloss", ref_loader, orc, cube, suzanne)
    r = sc.reference(sref, orc, c)
    assert c["gloss_spheres"][0][1] == (1.0, 0.5, 0.0) and max(max(k) for k in c["sky_colors"]) == 2.0 and c["bounces"] == 4
    assert r["sky_terms"] > 0 and pc.color_bar(c) > pc.COLOR_TOL and r["gen_gloss"][1] > 0 and r["gen_gloss"][2:].sum() > 0
    assert float(r["color_f32"][..., :3].max()) > 1.0                                                 # a colour above 1 does reach the frame


def test_far_gloss(sref, orc, ref_loader, cube, suzanne):
    c = _directed("far_gloss", ref_loader, orc, cube, suzanne)
    r = sc.reference(sref, orc, c)
    centre = c["spheres"].view(orc.SPHERE_DTYPE)[0]["center"]
    assert (np.abs(centre) > 9.9e3).all() and float(np.spacing(np.float32(1e4))) > 2e-4             # 1e-4 n is less than half an ulp of P
    assert c["gloss_spheres"][0][0] == 0.25 and not c["mirrors"] and c["shadows"] and c["sky"]
    hits = sc.h0_scatter(sref, orc, c)
    moved = sum(bool(((P + 1e-4 * n.astype(np.float64)).astype(np.float32) != P.astype(np.float32)).any()) for _, _, P, n, _ in hits)
    print(f"far_gloss: glossy rays per generation {r['gen_gloss'][1:].tolist()}; of {len(hits)} centre-ray hits on the sphere the 1e-4 n offset moves "
          f"the f32 origin of {moved}")
    assert r["gen_gloss"][1] > 0 and r["gen_gloss"][2] > 0 and len(hits) > 20 and moved < len(hits)


def test_rough_one(sref, orc, ref_loader, cube, suzanne):
    c = _directed("rough_one", ref_loader, orc, cube, suzanne)
    on, off = sc.reference(sref, orc, c), sc.reference(sref, orc, c, gloss=False)
    assert c["gloss_parts"] == {1: (1.0, (0.8, 0.6, 0.9))} and pc.n_parts(c) == 2 and c["bounces"] == 3
    print(f"rough_one: rays per generation {on['gen_rays'][1:].tolist()} with the flag, {off['gen_rays'][1:].tolist()} without; glossy {on['gen_gloss'][1:].tolist()}")
    assert np.array_equal(on["gen_rays"], off["gen_rays"]) and on["rays"] == off["rays"] and on["sky_terms"] == off["sky_terms"]
    assert (on["gen_gloss"][1:] > 0).all() and off["glossy"] == 0 and not np.array_equal(on["color_f32"], off["color_f32"])
    for k in ("obj_id", "hit_t", "depth"):
        assert on[k].tobytes() == off[k].tobytes()
    for pixel, _, _, n, S in sc.h0_scatter(sref, orc, c)[::7]:
        X = gloss_ref.bounce_direction(sref, n, pixel, 0, 2, c["seed"])
        assert all(S[i] == X[i] for i in range(3)), pixel


def test_last_bit_of_s(sref, orc, ref_loader, cube, suzanne):
    """The case is as sensitive as it was built to be, shown through an input: the floor's roughness one step of the table's
    2^-23 higher moves S in its last bits, and the frame by more than its bar, with every sample-0 plane unchanged."""
    c = _directed("last_bit_of_s", ref_loader, orc, cube, suzanne)
    r = sc.reference(sref, orc, c)
    assert c["bounces"] == 8 and set(c["gloss_parts"]) == {0, 1} and set(c["mirror_spheres"]) == set(range(8)) and not c["glass"]
    assert (r["gen_mirror"][1:7] > 0).all() and (r["gen_gloss"][1:] > 0).all()
    rho = float(gloss_ref.roughness_of(c["gloss_parts"][0][0]))
    S0, _ = gloss_ref.scatter(sref, (0.0, 1.0, 0.0), (0.6, -0.8, 0.0), np.float32(rho), pixel=11, seed=c["seed"])
    S1, _ = gloss_ref.scatter(sref, (0.0, 1.0, 0.0), (0.6, -0.8, 0.0), np.float32(rho + 2.0 ** -23), pixel=11, seed=c["seed"])
    assert 0.0 < float(np.abs(S1 - S0).max()) <= 2.0 ** -22
    near = sc.reference(sref, orc, c, gloss_parts={0: (rho + 2.0 ** -23, c["gloss_parts"][0][1]), 1: c["gloss_parts"][1]})
    for k in ("obj_id", "hit_t", "depth"):
        assert r[k].tobytes() == near[k].tobytes()
    d = float(np.abs(r["color_f32"] - near["color_f32"]).max())
    print(f"last_bit_of_s: glossy rays per generation {r['gen_gloss'][1:].tolist()}, mirror reflections {r['gen_mirror'][1:].tolist()}; the floor's roughness "
          f"2^-23 higher moves the colour by {d:.3g} ({d / pc.color_bar(c):.1f} bars)")
    assert d > 2.0 * pc.color_bar(c)


# ------------------------------------------------------------------ the further checks --
def test_the_cases_chosen_for_the_further_checks(cases, refs):
    rays = lambda q: refs[q]["glossy"]       # noqa: E731
    acc = [cases[q] for q in sc.ACCUMULATION]
    assert len(set(sc.ACCUMULATION)) == 4
    for c in acc:
        k, s = pc.accumulation_steps(c)
        assert c["gloss"] and k >= 2 and k * s == c["spp"] >= 2 and rays(c["q"]) > 0 and refs[c["q"]]["gen_gloss"][2:].sum() > 0
    assert sum(c["instances"] is not None for c in acc) >= 2 and sum(c["bounces"] == 8 for c in acc) >= 2
    assert sum(sum(refs[c["q"]]["events"]) > 0 and refs[c["q"]]["gen_mirror"].sum() > 0 for c in acc) >= 2
    split = [cases[q] for q in sc.SPLITS]
    assert len(set(sc.SPLITS)) == 2
    for c in split:
        r = refs[c["q"]]
        assert c["gloss"] and c["h"] > 16 and rays(c["q"]) > 0 and r["gen_gloss"][2] > 0
        rows = np.nonzero(sc.on_gloss(c, r["obj_id"]).any(axis=1))[0]
        assert {(int(y) // 8) % 2 for y in rows} == {0, 1}                                            # glossy surfaces at h0 in both ranks' rows
    # the cases rendered under the forced schedule too: the last of every block traces glossy rays (the flag-off ones when it is
    # forced on), the first of all but one flag-on block
    assert sc.FORCED == (0, 7)
    assert all(rays(q) > 0 for q in range(7, 96, 8)) and sum(rays(q) > 0 for q in range(0, 64, 8)) >= 7
    wide = range(8 * sc.WIDE_LANE_BLOCK, 8 * sc.WIDE_LANE_BLOCK + 8)
    assert all(cases[q]["gloss"] and cases[q]["mirrors"] and cases[q]["glass"] and rays(q) > 0 for q in wide)
    # ... and holds scenes as large as the one the wide kernel is known to be chosen for (856 world faces), without a normal map
    big = [q for q in wide if pc.n_base_faces(cases[q]) * (1 if cases[q]["instances"] is None else len(cases[q]["instances"])) >= 856
           and not cases[q]["extra"] & pc.FLAG_NORMAL_MAP]
    assert len(big) >= 2 and any(cases[q]["bounces"] > 1 for q in big), big


def test_the_rounded_reference(sref, orc, ref_loader, cube, suzanne, cases):
    """thr_unorm16 changes no integer on any committed entry (the throughput steers nothing); by how much it moves the colour is
    printed, and an entry whose two references differ by more than its bar is in ROUNDED_THROUGHPUT."""
    listed = list(cases) + [_directed(name, ref_loader, orc, cube, suzanne) for name in sc.DIRECTED]
    worst, worst_ratio, at, moved = 0.0, 0.0, None, 0
    for c in listed:
        a, b = sc.reference(sref, orc, c), sc.reference(sref, orc, c, thr_unorm16=True)
        for k in ("obj_id", "hit_t", "depth"):
            assert a[k].tobytes() == b[k].tobytes(), (k, sc.describe(c))
        _same_counts(a, b, sc.describe(c))
        d = float(np.abs(a["color_f32"] - b["color_f32"]).max())
        moved += d > 0.0
        if d / pc.color_bar(c) >= worst_ratio:
            worst, worst_ratio, at = d, d / pc.color_bar(c), c["index"]
        assert d <= pc.color_bar(c) or c.get("q", c["index"]) in sc.ROUNDED_THROUGHPUT, (d, sc.describe(c))
    print(f"plain against rounded reference over the {len(listed)} committed entries: the colour moves in {moved}, at most {worst:.3g} ({at}, "
          f"{worst_ratio:.2f} of its bar)")
    assert moved > 50
    # the cases of the walk held to the rounded reference: no integer moves there either, and the two references are about a bar apart
    for q in sc.ROUNDED_THROUGHPUT:
        c = sc.gloss_case(q, ref_loader, orc, cube, suzanne)
        a, b = sc.reference(sref, orc, c), sc.reference(sref, orc, c, thr_unorm16=True)
        for k in ("obj_id", "hit_t", "depth"):
            assert a[k].tobytes() == b[k].tobytes(), (k, sc.describe(c))
        _same_counts(a, b, sc.describe(c))
        d = float(np.abs(a["color_f32"] - b["color_f32"]).max())
        print(f"gloss case {q}: plain against rounded reference {d:.3g} ({d / pc.color_bar(c):.2f} of its bar); glossy rays {a['glossy']}, glass events {a['events']}")
        assert d > 0.5 * pc.color_bar(c) and c["gloss"] and c["glass"] and a["glossy"] > 0


def test_total_time(started):
    """Prints what the file took (some 700 reference frames of at most 80 x 56)."""
    print(f"tests/test_gloss_cases_host.py: {time.perf_counter() - started:.1f} s in total")
