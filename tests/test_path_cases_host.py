"""tests/path_cases.py's list, host side: with the CPU reference alone (mirror_ref.c) the conditions the GPU file,
tests/test_gpu_path_cases.py, relies on - conditions on the inputs, not measurements: enough cases see their mesh, their mirrors
(from h0 and from a bounce hit), shadowed and lit hits, the sky, later instances; every directed case does what it was built for;
and without mirrors the list's reference is sky_ref.c's, byte for byte.  No GPU.  The file's total time is printed."""
import time

import numpy as np
import pytest

import path_cases as pc
import mirror_ref


@pytest.fixture(scope="module", autouse=True)
def started():
    """When this file's first test began."""
    return time.perf_counter()


@pytest.fixture(scope="module")
def mref(tmp_path_factory):
    return mirror_ref.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def cases(ref_loader, orc, cube, suzanne):
    return [pc.case(i, ref_loader, orc, cube, suzanne) for i in range(pc.N_CASES)]


@pytest.fixture(scope="module")
def refs(mref, orc, cases):
    return [pc.reference(mref, orc, c, first=True) for c in cases]


def _directed(name, ref_loader, orc, cube, suzanne):
    return pc.directed(name, ref_loader, orc, cube, suzanne)


def test_the_list_is_deterministic_and_stratified(ref_loader, orc, cube, suzanne, cases):
    assert pc.N_CASES == 64 and len(pc.DIRECTED) == 8 and pc.N_LISTED == 72
    combos = {}
    for c in cases:
        i = c["index"]
        assert (c["multi"], c["shadows"], c["sky"], c["mirrors"]) == (bool(i & 1), bool(i & 2), bool(i & 4), bool(i & 8)), i
        assert (c["bounces"] > 1) == c["multi"] and c["bounces"] in (1, 2, 3, 8)
        assert c["mirror_parts"] or c["mirror_spheres"]
        assert all(k < len(c["spheres"]) for k in c["mirror_spheres"]) and all(k < pc.n_parts(c) for k in c["mirror_parts"])
        assert 5 <= c["w"] <= 80 and 3 <= c["h"] <= 56 and 1 <= c["frames_in_flight"] <= 3
        assert all(0.0 <= v <= 2.0 for k in c["sky_colors"] for v in k)
        combos[i % 16] = combos.get(i % 16, 0) + 1
    assert combos == {k: 4 for k in range(16)}
    # a case is rebuilt from its index alone
    pc._cache.pop(("case", 5))
    again = pc.case(5, ref_loader, orc, cube, suzanne)
    assert again is not cases[5] and pc.describe(again) == pc.describe(cases[5])
    assert again["cam_inv"].tobytes() == cases[5]["cam_inv"].tobytes()
    assert again["spheres"].tobytes() == cases[5]["spheres"].tobytes()
    pc._cache[("case", 5)] = cases[5]
    # sample counts that cross a launch group unevenly, under more than one flag, on small frames of few faces
    for spp in (33, 65):
        many = [c for c in cases if c["spp"] == spp]
        assert len(many) >= 2
        for c in many:
            assert c["w"] <= 24 and c["h"] <= 16 and pc.n_base_faces(c) <= 65 and c["multi"] + c["shadows"] + c["sky"] + c["mirrors"] >= 2
    assert {c["spp"] for c in cases} == {1, 2, 5, 9, 33, 65}
    # the ingredients all occur
    kinds = {c["what"].split(" +")[0] for c in cases}
    assert {"cube", "suzanne", "cube halves"} <= kinds and {f"soup {n}" for n in pc.FACE_COUNTS} <= kinds, kinds
    assert any("+ part" in c["what"] for c in cases)
    assert any(c["extra"] & pc.FLAG_NO_CULL for c in cases) and any(c["extra"] & pc.FLAG_NORMAL_MAP for c in cases)
    assert {len(c["spheres"]) for c in cases} >= {0, 8}
    assert {c["frames_in_flight"] for c in cases} == {1, 2, 3}
    # instances are rigid: rotation about an axis that is no coordinate axis, plus a translation
    for c in cases:
        if c["instances"] is not None:
            assert 2 <= len(c["instances"]) <= (2 if pc.n_base_faces(c) >= 300 else 4)
            for m in c["instances"]["model"]:
                r = m[:3, :3].astype(np.float64)
                assert np.abs(r @ r.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(r) - 1.0) < 1e-6
                assert m[:3, 3].tolist() == [0.0, 0.0, 0.0] and m[3, 3] == 1.0


def test_the_cases_see_their_scenes(cases, refs):
    seen = sum(float((r["obj_id"] != -1).mean()) >= 0.05 for r in refs)
    print(f"cases with >= 5 % of their pixels hit: {seen} of {len(cases)}")
    assert 4 * seen >= 3 * len(cases)


def test_the_cases_exercise_the_mirrors(cases, refs):
    mirror = [(c, r) for c, r in zip(cases, refs) if c["mirrors"]]
    any_gen = sum(r["gen_mirror"].sum() > 0 for c, r in mirror)
    deep = [(c, r) for c, r in mirror if c["bounces"] >= 2]
    second = sum(r["gen_mirror"][2] > 0 for c, r in deep)
    print(f"mirror cases with a reflection: {any_gen} of {len(mirror)}; of those with B >= 2, a reflection off a bounce hit: {second} of {len(deep)}")
    assert len(mirror) == 32 and 4 * any_gen >= 3 * len(mirror)
    assert len(deep) == 16 and 2 * second >= len(deep)
    # both kinds of surface reflect somewhere in the list, and reflected rays find faces, spheres and nothing
    found = set()
    for c, r in mirror:
        f = r["first"].reshape(-1, 8)
        found |= set(np.unique(f[f[:, 7] > 0][:, 6]).tolist())
    assert found == {0.0, 1.0, 2.0}
    # without the flag the reference counts no reflection, whatever mirrors the case carries
    assert all(r["gen_mirror"].sum() == 0 for c, r in zip(cases, refs) if not c["mirrors"])


def test_the_cases_exercise_shadows_and_sky(cases, refs):
    shadow = [(c, r) for c, r in zip(cases, refs) if c["shadows"]]
    mixed = sum(0 < r["occluded"] < r["shadow_rays"] for c, r in shadow)
    print(f"shadow cases with occluded and unoccluded rays: {mixed} of {len(shadow)}")
    assert len(shadow) == 32 and 3 * mixed >= len(shadow)
    for c, r in shadow:
        if (r["obj_id"] != -1).any():
            assert r["shadow_rays"] > 0, pc.describe(c)
    sky = [(c, r) for c, r in zip(cases, refs) if c["sky"]]
    lit = sum(r["sky_terms"] > 0 for c, r in sky)
    print(f"sky cases with a sky term: {lit} of {len(sky)}")
    assert len(sky) == 32 and 4 * lit >= 3 * len(sky)


def test_the_cases_exercise_rotated_instances(cases, refs):
    inst = [(c, r) for c, r in zip(cases, refs) if c["instances"] is not None]
    later = sum(r["obj_id"].max() >= pc.n_base_faces(c) for c, r in inst)
    mirrored = sum(bool(c["mirrors"] and c["mirror_parts"] and r["gen_mirror"].sum() > 0) for c, r in inst)
    shadowed = sum(bool(c["shadows"] and r["occluded"] > 0) for c, r in inst)
    print(f"instance cases: {len(inst)}; showing a later instance: {later}; with a mirror part and reflections: {mirrored}; with occluded shadow rays: {shadowed}")
    assert len(inst) >= 8 and later >= 4 and mirrored >= 3 and shadowed >= 3


def test_inside_mirror_sphere(mref, orc, ref_loader, cube, suzanne):
    c = _directed("inside_mirror_sphere", ref_loader, orc, cube, suzanne)
    r = pc.reference(mref, orc, c, first=True)
    n = c["w"] * c["h"] * c["spp"]
    assert (r["obj_id"] == -2).all()
    assert c["bounces"] == 8 and r["rays"] == n * 8 and r["gen_rays"][1:].tolist() == [n] * 8     # no path ends before B
    # the outward normal against an inside hit: the reflection starts outside the sphere and finds it again at once, from outside
    # (generation 1, a sphere, and a reflection again); generation 2 then leaves into the room
    first = r["first"].reshape(-1, 8)
    assert (first[:, 7] == 1).all() and (first[:, 6] == 2).all()
    assert r["gen_mirror"][1] == n and r["gen_mirror"][2] == n and r["gen_mirror"][3] < n
    assert r["occluded"] == r["shadow_rays"] == n * 9         # (the room is closed: no light reaches any hit)


def test_facing_mirrors(mref, orc, ref_loader, cube, suzanne):
    c = _directed("facing_mirrors", ref_loader, orc, cube, suzanne)
    r = pc.reference(mref, orc, c)
    assert c["bounces"] == 8 and r["gen_mirror"][8] > 0
    assert (r["gen_mirror"][1:] > 0).all() and r["sky_terms"] > 0
    ids = np.unique(r["obj_id"])
    assert {0, 1} & set(ids.tolist()) and {2, 3} & set(ids.tolist()) and ids.max() >= 4          # both quads and the cube in view


def test_black_mirror(mref, orc, ref_loader, cube, suzanne):
    c = _directed("black_mirror", ref_loader, orc, cube, suzanne)
    assert c["bounces"] == 1 and c["mirror_parts"] == {0: (0.0, 0.0, 0.0)}
    r = pc.reference(mref, orc, c, first=True)
    white = pc.reference(mref, orc, c, mirror_parts={0: (1.0, 1.0, 1.0)}, bounces=2)
    flat = pc.reference(mref, orc, c, bounces=0)
    assert r["rays"] == white["gen_rays"][1] > 0 and r["gen_mirror"][1] > 0                      # rays of no throughput are rays
    on_quad = (r["first"][..., 7] == 1).all(axis=2)                                              # every sample's h0 on the quad
    assert on_quad.sum() > 50 and not on_quad.all()
    assert np.array_equal(r["color_f32"][on_quad], flat["color_f32"][on_quad])
    assert not np.array_equal(white["color_f32"][on_quad], flat["color_f32"][on_quad])


def test_rotated_parts(mref, orc, ref_loader, cube, suzanne):
    c = _directed("rotated_parts", ref_loader, orc, cube, suzanne)
    r = pc.reference(mref, orc, c, first=True)
    nb = pc.n_base_faces(c)
    at_h0 = (r["first"][:, :, 0, 7] == 1) & (r["obj_id"] >= 0)        # sample 0 reflected at h0, a mesh face
    off = set(np.unique(r["obj_id"][at_h0] // nb).tolist())
    print(f"rotated_parts: reflections at h0 off instances {sorted(off)}, per generation {r['gen_mirror'][1:].tolist()}")
    assert {1, 2} <= off
    assert (r["obj_id"][at_h0] % nb >= nb // 2).all()                 # the mirror part is part 1: the base face's second half
    assert r["gen_mirror"][2] > 0 and 0 < r["occluded"] < r["shadow_rays"]


def test_nmap_mirror(mref, orc, ref_loader, cube, suzanne):
    c = _directed("nmap_mirror", ref_loader, orc, cube, suzanne)
    assert c["extra"] & pc.FLAG_NORMAL_MAP
    r = pc.reference(mref, orc, c, first=True)
    flat = pc.reference(mref, orc, c, first=True, extra=0)
    assert not np.array_equal(r["color_f32"], flat["color_f32"])
    assert r["first"].tobytes() == flat["first"].tobytes() and r["gen_mirror"][1] > 0 and r["gen_mirror"][2] > 0
    assert r["rays"] == flat["rays"] and np.array_equal(r["gen_rays"], flat["gen_rays"])        # normal maps never change n


def test_the_other_directed_cases(mref, orc, ref_loader, cube, suzanne):
    c = _directed("no_cull_all", ref_loader, orc, cube, suzanne)
    r = pc.reference(mref, orc, c)
    assert pc.flags(c) == (pc.FLAG_AUX_OUTPUTS | pc.FLAG_NO_CULL | pc.FLAG_MULTI_BOUNCE | pc.FLAG_SHADOWS | pc.FLAG_SKY | pc.FLAG_MIRRORS)
    assert r["gen_mirror"][1] > 0 and r["gen_mirror"][2] > 0 and r["sky_terms"] > 0 and 0 < r["occluded"] < r["shadow_rays"]
    c = _directed("far_mirror", ref_loader, orc, cube, suzanne)
    r = pc.reference(mref, orc, c, first=True)
    assert min(c["eye"]) > 9.9e3 and (r["obj_id"] == -2).sum() > 20 and (r["obj_id"] >= 0).sum() > 20
    f = r["first"].reshape(-1, 8)
    assert {0.0, 1.0} <= set(np.unique(f[f[:, 7] > 0][:, 6]).tolist())                           # the mirror sphere shows the mesh and the sky
    assert r["sky_terms"] > 0 and 0 < r["occluded"] < r["shadow_rays"]
    c = _directed("all_sphere_mirrors", ref_loader, orc, cube, suzanne)
    r = pc.reference(mref, orc, c, first=True)
    assert pc.n_parts(c) == 2 and len(c["spheres"]) == 8 and len({v for v in c["mirror_spheres"].values()}) == 8
    at_h0 = r["first"][:, :, 0, 7] == 1
    assert set(np.unique(r["obj_id"][at_h0]).tolist()) == {-2 - k for k in range(8)}             # every sphere reflects at h0 ...
    t0 = r["first"][:, :, 0, 3:6]
    for k, refl in c["mirror_spheres"].items():                                                  # ... with its own record's R: T0 = R
        px = at_h0 & (r["obj_id"] == -2 - k)
        assert np.array_equal(t0[px], np.tile(np.asarray(refl, np.float32), (int(px.sum()), 1))), k
    ids = np.unique(r["obj_id"])
    assert ((ids >= 0) & (ids < 65)).any() and (ids >= 65).any()                                 # both parts in view


def test_without_mirrors_the_reference_is_sky_ref(mref, orc, ref_loader, cube, suzanne):
    """mirror_parts = mirror_spheres = None: mirror_render_path and sky_render_path give the same bytes on every case of the list."""
    for j in range(pc.N_LISTED):
        c = pc.listed(j, ref_loader, orc, cube, suzanne)
        a = pc.reference(mref, orc, c, mirrors=False)
        b = pc.reference(mref, orc, c, mirrors=False, use_sky_ref=True)
        for k in pc.PLANES:
            assert a[k].tobytes() == b[k].tobytes(), (k, pc.describe(c))
        for k in ("rays", "shadow_rays", "occluded", "sky_terms"):
            assert a[k] == b[k], (k, pc.describe(c))
        assert a["gen_mirror"].sum() == 0 and a["gen_rays"].sum() == a["rays"]


def test_the_cases_chosen_for_accumulation_and_splits(cases, refs):
    acc = [cases[i] for i in pc.ACCUMULATION]
    assert len(set(pc.ACCUMULATION)) == 4
    for c in acc:
        k, s = pc.accumulation_steps(c)
        assert k >= 2 and k * s == c["spp"] >= 2 and c["mirrors"] and refs[c["index"]]["gen_mirror"].sum() > 0
    assert sum(c["instances"] is not None for c in acc) >= 3 and any(c["bounces"] > 1 for c in acc) and any(c["shadows"] for c in acc)
    split = [cases[i] for i in pc.SPLITS]
    assert len(set(pc.SPLITS)) == 2
    for c in split:
        assert c["h"] > 16 and c["mirrors"] and refs[c["index"]]["gen_mirror"][2] > 0
    assert any(c["instances"] is not None for c in split)
    # the eighth cases (rendered under the forced schedule too) and the wide-lane block trace bounce rays
    assert all(refs[i]["rays"] > 0 for i in range(0, pc.N_CASES, 8))
    assert sum(refs[i]["rays"] > 0 for i in range(24, 32)) >= 6


def test_total_time(started):
    """Prints what the file took (the references of all 72 entries with and without mirrors: about 13 s on 8 cores)."""
    print(f"tests/test_path_cases_host.py: {time.perf_counter() - started:.1f} s in total")
