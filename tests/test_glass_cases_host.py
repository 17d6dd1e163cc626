"""tests/glass_cases.py's list, host side: with the CPU reference alone (glass_ref.c) the conditions the GPU file,
tests/test_gpu_glass_cases.py, relies on - conditions on the inputs, not measurements: the list is deterministic and stratified,
enough cases have every kind of glass event in every setting (beside mirrors, on rotated instances, under normal maps and
RWR_FLAG_NO_CULL, at many samples and at B = 8), the reference's counts mean what they are taken to mean, every directed case does
what it was built for, and the cases chosen for the further checks trace glass events.  If a draw misses a condition the draw is
changed (GLASS_BASE, the probabilities), not the threshold.  No GPU.  The counts found and the file's total time are printed."""
import time

import numpy as np
import pytest

import glass_cases as gc
import glass_ref
import path_cases as pc

ON = range(48)            # RWR_FLAG_GLASS on
OFF = range(48, 64)       # glass surfaces set, the flag off


@pytest.fixture(scope="module", autouse=True)
def started():
    """When this file's first test began."""
    return time.perf_counter()


@pytest.fixture(scope="module")
def gref(tmp_path_factory):
    return glass_ref.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def cases(ref_loader, orc, cube, suzanne):
    return [gc.glass_case(g, ref_loader, orc, cube, suzanne) for g in range(gc.N_GLASS_CASES)]


@pytest.fixture(scope="module")
def refs(gref, orc, cases):
    """Every case rendered with its glass, the flag-off cases too (their own reference, without glass, is in `plain`)."""
    return [gc.reference(gref, orc, c, glass=True) for c in cases]


@pytest.fixture(scope="module")
def plain(gref, orc, cases):
    return [gc.reference(gref, orc, c, glass=False) for c in cases]


def _directed(name, ref_loader, orc, cube, suzanne):
    return gc.directed(name, ref_loader, orc, cube, suzanne)


def _surfaces(c):
    return list(c["glass_parts"].values()) + list(c["glass_spheres"].values())


def test_the_list_is_deterministic_and_stratified(ref_loader, orc, cube, suzanne, cases):
    assert gc.N_GLASS_CASES == 64 and len(gc.DIRECTED) == 10
    combos = {}
    for c in cases:
        g = c["g"]
        base = pc.case(pc.N_CASES + g, ref_loader, orc, cube, suzanne)
        assert (c["multi"], c["shadows"], c["sky"], c["mirrors"]) == (bool(g & 1), bool(g & 2), bool(g & 4), bool(g & 8)), g
        assert c["glass"] == (g // 16 != 3)
        assert gc.flags(c) == pc.flags(base) | (gc.FLAG_GLASS if c["glass"] else 0)
        combos[(g % 16, c["glass"])] = combos.get((g % 16, c["glass"]), 0) + 1
        # at least one glass surface, every key in range, no surface both mirror and glass, and the case under it untouched
        assert c["glass_parts"] or c["glass_spheres"]
        assert all(0 <= k < pc.n_parts(c) for k in c["glass_parts"]) and all(0 <= k < len(c["spheres"]) for k in c["glass_spheres"])
        assert not set(c["glass_parts"]) & set(c["mirror_parts"]) and not set(c["glass_spheres"]) & set(c["mirror_spheres"])
        assert c["mirror_parts"] == {k: v for k, v in base["mirror_parts"].items() if k not in c["glass_parts"]}
        assert c["mirror_spheres"] == {k: v for k, v in base["mirror_spheres"].items() if k not in c["glass_spheres"]}
        assert "glass_parts" not in base and c["cam_inv"] is base["cam_inv"] and c["model"] is base["model"]
        for ior, tint in _surfaces(c):
            assert 1.0 <= ior <= 4.0 and len(tint) == 3 and all(0.0 <= v <= 1.0 for v in tint)
    assert combos == {(k, on): (3 if on else 1) for k in range(16) for on in (True, False)}
    # a case is rebuilt from its index alone: the glass generator is the case's own, the path case's generator is not drawn from
    kept = cases[5]
    gc._cache.pop(("case", 5))
    pc._cache.pop(("case", pc.N_CASES + 5))
    again = gc.glass_case(5, ref_loader, orc, cube, suzanne)
    assert again is not kept and gc.describe(again) == gc.describe(kept)
    assert again["cam_inv"].tobytes() == kept["cam_inv"].tobytes() and again["spheres"].tobytes() == kept["spheres"].tobytes()
    assert again["glass_parts"] == kept["glass_parts"] and again["glass_spheres"] == kept["glass_spheres"]
    assert again["mirror_parts"] == kept["mirror_parts"] and again["mirror_spheres"] == kept["mirror_spheres"]
    gc._cache[("case", 5)] = kept
    # the old list is what it was: its cases carry no glass and keep their indices
    assert pc.N_CASES == 64 and "glass_parts" not in pc.case(5, ref_loader, orc, cube, suzanne)
    # every kind of index and tint occurs
    iors = {ior for c in cases for ior, _ in _surfaces(c)}
    assert set(gc.IORS) <= iors and any(v not in gc.IORS for v in iors)
    tints = {v for c in cases for _, t in _surfaces(c) for v in t}
    assert {0.0, 1.0} <= tints and any(0.0 < v < 1.0 for v in tints)
    # frames no larger than the old list's, and none of the directed ones a multiple of the 64 x 8 tile
    # (a soup, and the second part drawn beside one, is at most 300 faces; the other models are the two meshes of the resources)
    assert all(c["w"] <= 80 and c["h"] <= 56 for c in cases)
    for c in cases:
        parts = c["model"] if isinstance(c["model"], (list, tuple)) else [c["model"]]
        if c["what"].startswith("soup"):
            assert all(len(p["faces"]) <= 300 for p in parts), gc.describe(c)
        else:
            assert pc.n_base_faces(c) in (len(cube["faces"]), len(suzanne["faces"])), gc.describe(c)
    for name in gc.DIRECTED:
        d = _directed(name, ref_loader, orc, cube, suzanne)
        assert d["w"] <= 72 and d["h"] <= 48 and d["spp"] <= 5 and (d["w"] % 64 != 0 or d["h"] % 8 != 0), name
        if name in ("soup_glass_all", "all_sphere_glass_b1", "all_sphere_glass_b3"):
            assert pc.n_base_faces(d) <= 300, name
        assert gc.DIRECTED[name].__doc__, name


def test_the_cases_exercise_the_glass(gref, orc, cases, refs):
    """The minimum number of flag-on cases per condition: each has roughly a factor of two of slack against the draw."""
    on = [(cases[g], refs[g]) for g in ON]
    ev = lambda r: sum(r["events"])       # noqa: E731
    parts_alone = {c["g"]: sum(gc.reference(gref, orc, c, glass_spheres={})["events"]) for c, r in on}
    spheres_alone = {c["g"]: sum(gc.reference(gref, orc, c, glass_parts={})["events"]) for c, r in on}
    found = {
        "a glass event": (sum(ev(r) > 0 for c, r in on), 36),
        "reflections and transmissions": (sum(r["events"][0] > 0 and r["events"][1] > 0 for c, r in on), 30),
        "total internal reflections": (sum(r["events"][2] > 0 for c, r in on), 12),
        "total internal reflections at max_bounces 1": (sum(r["events"][2] > 0 and c["bounces"] == 1 for c, r in on), 2),
        "paths of two or more transmissions": (sum(r["multi"] > 0 for c, r in on), 12),
        "glass events and mirror reflections": (sum(ev(r) > 0 and r["gen_mirror"].sum() > 0 for c, r in on), 8),
        "events from glass parts alone, on instances": (sum(parts_alone[c["g"]] > 0 and c["instances"] is not None for c, r in on), 6),
        "events from glass parts alone": (sum(v > 0 for v in parts_alone.values()), 20),
        "events from spheres alone": (sum(v > 0 for v in spheres_alone.values()), 20),
        "events under RWR_FLAG_NORMAL_MAP": (sum(ev(r) > 0 and bool(c["extra"] & pc.FLAG_NORMAL_MAP) for c, r in on), 4),
        "events under RWR_FLAG_NO_CULL": (sum(ev(r) > 0 and bool(c["extra"] & pc.FLAG_NO_CULL) for c, r in on), 3),
        "events at 33 or 65 samples": (sum(ev(r) > 0 and c["spp"] in (33, 65) for c, r in on), 2),
        "events at B = 8": (sum(ev(r) > 0 and c["bounces"] == 8 for c, r in on), 5),
    }
    for what, (n, least) in found.items():
        print(f"glass cases with {what}: {n} of {len(on)} (at least {least})")
    for what, (n, least) in found.items():
        assert n >= least, (what, n, least)
    # the range's edges, exactly, on surfaces of cases that have events
    for edge in (1.0, 4.0):
        assert any(ev(r) > 0 and any(ior == edge for ior, _ in _surfaces(c)) for c, r in on), edge
    # on an instance case the glass part's events come from later instances too: h0 on a glass face of instance >= 1
    later = sum(c["instances"] is not None and bool((gc.on_glass(c, r["obj_id"]) & (r["obj_id"] >= pc.n_base_faces(c))).any()) for c, r in on)
    print(f"glass cases whose sample-0 plane shows a glass face of a later instance: {later}")
    assert later >= 3


def test_flag_off_cases_could_fail(cases, refs, plain):
    """Without the flag the reference has no events; rendered with their glass the same cases would differ: 'does nothing' is a claim."""
    differ = 0
    for g in OFF:
        assert not cases[g]["glass"] and plain[g]["events"] == (0, 0, 0) and plain[g]["multi"] == 0 and plain[g]["gen_glass"].sum() == 0
        differ += not np.array_equal(refs[g]["color_f32"], plain[g]["color_f32"])
    print(f"flag-off cases whose frame would differ with the glass on: {differ} of {len(OFF)} (at least 8)")
    assert differ >= 8


def test_reference_invariants(gref, orc, cases, refs, plain):
    """What makes the counts meaningful: at max_bounces = 1 every sample whose h0 lies on glass is one event and nothing else is;
    sample-0 planes and generation 1's ray count do not depend on the glass; the tint steers nothing."""
    h0_events = 0
    for g in ON:
        c, r = cases[g], refs[g]
        one = gc.reference(gref, orc, c, spp=1, bounces=1)
        n = int(gc.on_glass(c, one["obj_id"]).sum())
        assert sum(one["events"]) == n == one["gen_glass"][1], (sum(one["events"]), n, gc.describe(c))
        h0_events += n
        for k in ("obj_id", "hit_t", "depth"):
            assert r[k].tobytes() == plain[g][k].tobytes(), (k, gc.describe(c))
        assert r["gen_rays"][1] == plain[g]["gen_rays"][1] and sum(r["events"]) == r["gen_glass"].sum()
        black = gc.reference(gref, orc, c, glass_parts={k: (i, (0.0, 0.0, 0.0)) for k, (i, _) in c["glass_parts"].items()},
                             glass_spheres={k: (i, (0.0, 0.0, 0.0)) for k, (i, _) in c["glass_spheres"].items()})
        clear = gc.reference(gref, orc, c, glass_parts={k: (i, (1.0, 1.0, 1.0)) for k, (i, _) in c["glass_parts"].items()},
                             glass_spheres={k: (i, (1.0, 1.0, 1.0)) for k, (i, _) in c["glass_spheres"].items()})
        for k in ("events", "multi", "deep", "rays", "shadow_rays", "occluded", "sky_terms"):
            assert black[k] == clear[k] == r[k], (k, gc.describe(c))
        assert np.array_equal(black["gen_rays"], clear["gen_rays"]) and np.array_equal(black["gen_glass"], r["gen_glass"])
    print(f"samples whose h0 lies on glass, one per pixel over the 48 flag-on cases: {h0_events}")
    assert h0_events > 1000


# ------------------------------------------------------------------ the directed cases --
def test_back_face_pane(gref, orc, ref_loader, cube, suzanne):
    c = _directed("back_face_pane", ref_loader, orc, cube, suzanne)
    r = gc.reference(gref, orc, c)
    twin = gc.reference(gref, orc, c, glass_parts={1: c["glass_parts"][1]})
    back = gc.reference(gref, orc, c, glass_parts={0: c["glass_parts"][0]})
    print(f"back_face_pane: events {r['events']}; the back-facing pane alone {back['events']}, the front-facing twin alone {twin['events']}")
    assert c["bounces"] == 1 and pc.n_parts(c) == 3 and c["extra"] == 0
    assert r["events"][2] > 100 and r["events"][0] > 0 and r["events"][1] > 0
    assert twin["events"][2] == 0 and twin["events"][0] > 0 and twin["events"][1] > 0
    assert back["events"][2] == r["events"][2] and back["events"][1] > 0          # the back face both reflects totally and lets rays out
    assert tuple(a + b for a, b in zip(back["events"], twin["events"])) == r["events"]
    ids = set(np.unique(r["obj_id"]).tolist())
    assert {0, 1} & ids and {2, 3} & ids                                            # both panes at h0


def test_soup_glass_all(gref, orc, ref_loader, cube, suzanne):
    c = _directed("soup_glass_all", ref_loader, orc, cube, suzanne)
    r = gc.reference(gref, orc, c)
    assert gc.flags(c) == (pc.FLAG_AUX_OUTPUTS | pc.FLAG_NO_CULL | pc.FLAG_MULTI_BOUNCE | pc.FLAG_SHADOWS | pc.FLAG_SKY | pc.FLAG_MIRRORS | gc.FLAG_GLASS)
    assert pc.n_base_faces(c) == 129 and c["bounces"] == 3 and len(c["spheres"]) == 2 and list(c["mirror_spheres"]) == [1]
    assert all(v > 0 for v in r["events"]) and r["multi"] > 0 and (r["gen_glass"][1:] > 0).all()
    assert r["gen_mirror"].sum() > 0 and r["sky_terms"] > 0 and 0 < r["occluded"] < r["shadow_rays"]
    one = gc.reference(gref, orc, c, spp=1, bounces=1)
    assert one["events"][2] > 0                                                     # a soup triangle seen from behind at h0


def test_nmap_glass(gref, orc, ref_loader, cube, suzanne):
    c = _directed("nmap_glass", ref_loader, orc, cube, suzanne)
    assert c["extra"] & pc.FLAG_NORMAL_MAP and list(c["glass_parts"]) == [0] and not c["mirror_parts"]
    r = gc.reference(gref, orc, c)
    flat = gc.reference(gref, orc, c, extra=0)
    assert sum(r["events"]) > 0 and r["events"] == flat["events"] and r["rays"] == flat["rays"]       # normal maps never change n
    assert np.array_equal(r["gen_rays"], flat["gen_rays"]) and np.array_equal(r["gen_glass"], flat["gen_glass"]) and r["gen_glass"][2] > 0
    assert not np.array_equal(r["color_f32"], flat["color_f32"])


def test_all_sphere_glass(gref, orc, ref_loader, cube, suzanne):
    one = _directed("all_sphere_glass_b1", ref_loader, orc, cube, suzanne)
    three = _directed("all_sphere_glass_b3", ref_loader, orc, cube, suzanne)
    assert one["bounces"] == 1 and three["bounces"] == 3 and gc.describe(dict(one, bounces=3, what="", index="")) == gc.describe(dict(three, what="", index=""))
    assert pc.n_parts(one) == 2 and len(one["spheres"]) == 8 and list(one["mirror_parts"]) == [1]
    assert len({v[0] for v in one["glass_spheres"].values()}) == 8 and len({v[1] for v in one["glass_spheres"].values()}) == 8
    r = gc.reference(gref, orc, one)
    assert {-2 - k for k in range(8)} <= set(np.unique(r["obj_id"]).tolist())                         # every sphere id at h0
    per_sample = gc.reference(gref, orc, one, spp=1)
    assert sum(per_sample["events"]) == int((per_sample["obj_id"] <= -2).sum()) > 0                   # B = 1: an event per h0 on a sphere
    assert r["gen_mirror"][1] > 0 and sum(r["events"]) == r["gen_glass"][1]
    deep = gc.reference(gref, orc, three)
    assert deep["gen_glass"][1] == r["gen_glass"][1] and deep["gen_glass"][2] > 0 and deep["gen_glass"][3] > 0 and deep["multi"] > 0
    assert deep["gen_mirror"][2] > 0                                                                  # the mirror part through the glass


def test_nested_spheres(gref, orc, ref_loader, cube, suzanne):
    c = _directed("nested_spheres", ref_loader, orc, cube, suzanne)
    (c0, r0), (c1, r1) = [(np.asarray(s["center"], np.float64), float(s["radius"])) for s in c["spheres"]]
    assert np.linalg.norm(c1 - c0) + r1 < r0 and np.linalg.norm(np.asarray(c["eye"]) - c0) > r0       # wholly inside; the eye outside
    assert c["glass_spheres"][0][0] != c["glass_spheres"][1][0] and c["bounces"] == 8
    r = gc.reference(gref, orc, c)
    print(f"nested_spheres: events {r['events']}, paths of >= 2 transmissions {r['multi']}, of >= 4 {r['deep']}, per generation {r['gen_glass'][1:].tolist()}")
    assert r["deep"] >= 100 and r["multi"] > r["deep"] and r["gen_glass"][8] > 0


def test_twin_spheres(gref, orc, ref_loader, cube, suzanne):
    c = _directed("twin_spheres", ref_loader, orc, cube, suzanne)
    assert c["spheres"][0].tobytes() == c["spheres"][1].tobytes() and list(c["glass_spheres"]) == [0] and list(c["mirror_spheres"]) == [1]
    r = gc.reference(gref, orc, c)
    swapped = gc.reference(gref, orc, c, glass_spheres={1: c["glass_spheres"][0]}, mirror_spheres={0: c["mirror_spheres"][1]})
    print(f"twin_spheres: events {r['events']}, mirror reflections {int(r['gen_mirror'].sum())}; swapped {swapped['events']}, {int(swapped['gen_mirror'].sum())}")
    assert sum(r["events"]) > 0 and r["events"] != swapped["events"]                                  # the tie matters
    assert r["obj_id"].tobytes() == swapped["obj_id"].tobytes() and (r["obj_id"] == -2).any() and not (r["obj_id"] == -3).any()


def test_glass_between_mirrors(gref, orc, ref_loader, cube, suzanne):
    c = _directed("glass_between_mirrors", ref_loader, orc, cube, suzanne)
    r = gc.reference(gref, orc, c)
    print(f"glass_between_mirrors: glass events per generation {r['gen_glass'][1:].tolist()}, mirror reflections {r['gen_mirror'][1:].tolist()}")
    assert c["bounces"] == 8 and c["glass_parts"][3][0] == 1.33 and set(c["mirror_parts"]) == {0, 1}
    assert (r["gen_glass"][1:] > 0).all() and r["gen_glass"][8] > 0 and (r["gen_mirror"][1:] > 0).all()
    assert r["events"][0] > 0 and r["events"][1] > 0 and r["deep"] > 0


def test_bright_sky_tint(gref, orc, ref_loader, cube, suzanne):
    c = _directed("bright_sky_tint", ref_loader, orc, cube, suzanne)
    r = gc.reference(gref, orc, c)
    assert c["glass_spheres"][0][1] == (1.0, 0.5, 0.0) and max(max(k) for k in c["sky_colors"]) == 2.0
    assert r["sky_terms"] > 0 and pc.color_bar(c) > pc.COLOR_TOL and sum(r["events"]) > 0 and r["multi"] > 0
    assert float(r["color_f32"][..., :3].max()) > 1.0                                                 # a colour above 1 does reach the frame


def test_ior_four_room(gref, orc, ref_loader, cube, suzanne):
    c = _directed("ior_four_room", ref_loader, orc, cube, suzanne)
    r = gc.reference(gref, orc, c)
    n = c["w"] * c["h"] * c["spp"]
    print(f"ior_four_room: events {r['events']}, rays per generation {r['gen_rays'][1:].tolist()}")
    assert c["glass_parts"][0][0] == 4.0 and c["bounces"] == 8
    assert r["events"][2] > r["events"][0] + r["events"][1] > 0
    assert r["gen_rays"][1:].tolist() == [n] * 8                                                      # the room is closed: no path ends early


# ------------------------------------------------------------------ the further checks --
def test_the_cases_chosen_for_the_further_checks(cases, refs):
    ev = lambda g: sum(refs[g]["events"])       # noqa: E731
    acc = [cases[g] for g in gc.ACCUMULATION]
    assert len(set(gc.ACCUMULATION)) == 4
    for c in acc:
        k, s = pc.accumulation_steps(c)
        assert c["glass"] and k >= 2 and k * s == c["spp"] >= 2 and ev(c["g"]) > 0
    assert sum(c["instances"] is not None for c in acc) >= 2 and any(c["bounces"] > 1 for c in acc)
    assert any(c["mirrors"] and refs[c["g"]]["gen_mirror"].sum() > 0 for c in acc)
    split = [cases[g] for g in gc.SPLITS]
    assert len(set(gc.SPLITS)) == 2
    for c in split:
        r = refs[c["g"]]
        assert c["glass"] and c["h"] > 16 and ev(c["g"]) > 0 and r["gen_glass"][2] > 0
        rows = np.nonzero(gc.on_glass(c, r["obj_id"]).any(axis=1))[0]
        assert {(int(y) // 8) % 2 for y in rows} == {0, 1}                                            # glass at h0 in both ranks' rows
    # the eighth cases with the flag on (rendered under the forced schedule too) and the wide-lane block trace glass events
    assert all(ev(g) > 0 for g in range(0, 48, 8))
    wide = range(8 * gc.WIDE_LANE_BLOCK, 8 * gc.WIDE_LANE_BLOCK + 8)
    assert all(cases[g]["glass"] and ev(g) > 0 for g in wide)
    # ... and holds scenes as large as the one the wide kernel is known to be chosen for (856 world faces), without a normal map
    big = [g for g in wide if pc.n_base_faces(cases[g]) * (1 if cases[g]["instances"] is None else len(cases[g]["instances"])) >= 856
           and not cases[g]["extra"] & pc.FLAG_NORMAL_MAP]
    assert len(big) >= 2 and any(cases[g]["bounces"] > 1 for g in big), big


def test_the_rounded_reference(gref, orc, ref_loader, cube, suzanne, cases):
    """thr_unorm16 changes no integer (the throughput steers nothing) and does move the colour; by how much is printed."""
    for c in [cases[g] for g in (9, 13, 37)] + [gc.glass_case(g, ref_loader, orc, cube, suzanne) for g in gc.ROUNDED_THROUGHPUT]:
        plain, rounded = gc.reference(gref, orc, c), gc.reference(gref, orc, c, thr_unorm16=True)
        for k in ("obj_id", "hit_t", "depth"):
            assert plain[k].tobytes() == rounded[k].tobytes()
        for k in ("events", "multi", "deep", "rays", "shadow_rays", "occluded", "sky_terms"):
            assert plain[k] == rounded[k], (k, gc.describe(c))
        d = float(np.abs(plain["color_f32"] - rounded["color_f32"]).max())
        print(f"{c['index']}: plain against rounded reference {d:.3g}")
        assert d > 0.0, gc.describe(c)
    c = gc.glass_case(gc.ROUNDED_THROUGHPUT[0], ref_loader, orc, cube, suzanne)
    assert c["glass"] and c["bounces"] == 8 and 4.0 in {ior for ior, _ in _surfaces(c)}


def test_total_time(started):
    """Prints what the file took (some 350 reference frames of at most 80 x 56: about 10 s on 8 cores)."""
    print(f"tests/test_glass_cases_host.py: {time.perf_counter() - started:.1f} s in total")
