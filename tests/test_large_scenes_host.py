"""Scenes beyond the 16-bit traversal stacks, host side (no GPU): the CPU reference alone (soft_shadow_ref.c, brute force over faces)
says that every frame tests/test_gpu_large_scenes.py renders can fail - the face counts lie on the intended side of
lane_lds_plan's limit, faces of index >= 4 096 are seen, the shadow rays are mixed, the lights' size changes answers in both
directions, every generation carries rays, every marked surface model is reached - and csrc/bvh.hpp's build_bvh, called directly
(bvh_host.cpp), returns trees with the invariants the traversal kernels rely on, on these scenes and on the skewed scene whose
SAH tree is rebuilt with median splits.

The coverage bounds are conditions on the inputs; the scenes' shapes, cameras and marks in tests/large_scenes.py were chosen
until the reference met them."""
import numpy as np
import pytest

import bvh_host
import large_scenes as ls
import soft_shadow_ref as ssr

SCENES = tuple(ls.SIZES)


@pytest.fixture(scope="module")
def soft(tmp_path_factory):
    return ssr.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def bvh_lib(tmp_path_factory):
    return bvh_host.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def corners(rwr, orc, ref_loader, suzanne, cube):
    """name -> (n, 9) world-space corners, by the reference's instancing."""
    return {name: ls.world_corners(orc, ls.scene(name, rwr, orc, ref_loader, suzanne, cube)) for name in SCENES}


def test_face_counts_lie_on_the_intended_side_of_the_limit(corners):
    for name in SCENES:
        assert len(corners[name]) == ls.N_FACES[name], name
        assert (len(corners[name]) <= ls.STACK16_MAX_FACES) == (name == "soup_4095"), name
    assert ls.N_FACES["soup_4095"] == ls.STACK16_MAX_FACES and ls.N_FACES["soup_4096"] == ls.STACK16_MAX_FACES + 1
    assert np.array_equal(corners["soup_4095"], corners["soup_4096"][:-1])   # the same soup, one face fewer
    assert ls.N_FACES["cube_grid4"] == 6848 and 13000 <= ls.N_FACES["parts_large"] <= 14400
    assert any(w % 64 or h % 8 for w, h in ls.SIZES.values())   # partial 64 x 8 tiles in at least one scene
    assert all(w <= 96 and h <= 64 for w, h in ls.SIZES.values())
    assert all(f["spp"] <= 5 for f in ls.FRAMES) and all(f["bounces"] in (0, 1, 4) for f in ls.LIMIT + ls.LADDER)
    assert ls.SCHEDULES["bounces"] == ls.SPLITS["bounces"] == 3 and "gloss_parts" in ls.marks(ls.SCHEDULES)


@pytest.mark.parametrize("i", range(len(ls.FRAMES)), ids=[ls.describe(f).replace(" ", "_") for f in ls.FRAMES])
def test_coverage_conditions(soft, rwr, orc, ref_loader, suzanne, cube, i):
    f = ls.FRAMES[i]
    what = ls.describe(f)
    ref = ls.reference(soft, rwr, orc, ref_loader, suzanne, cube, f)
    mesh = ref["obj_id"] >= 0
    w, h = ls.SIZES[f["scene"]]
    assert mesh.sum() >= 0.1 * w * h, (what, int(mesh.sum()))
    assert ref["obj_id"].max() < ls.N_FACES[f["scene"]]
    print(f"{what}: mesh pixels {int(mesh.sum())}, of index >= 4096 {int((ref['obj_id'] >= 4096).sum())}, shadow rays {ref['shadow_rays']} "
          f"occluded {ref['occluded']} to lit {ref['changed_to_lit']} to dark {ref['changed_to_dark']} rays per generation {ref['gen_rays'].tolist()} "
          f"glass {ref['events']} mirror {ref['gen_mirror'].tolist()} glossy {ref['gen_gloss'].tolist()}")
    if ls.N_FACES[f["scene"]] > 4096:   # (a soup of 4 096 faces has no such index: the limit frames differ in its last face instead, below)
        assert (ref["obj_id"] >= 4096).sum() >= 0.05 * mesh.sum(), what
    if f["shadows"]:   # shadow_common.check_class's rule for a mixed scene
        rays, occ = ref["shadow_rays"], ref["occluded"]
        assert rays > 0 and 0.1 <= occ / rays <= 0.9, (what, occ, rays)
    else:
        assert ref["shadow_rays"] == 0
    if f["radii"] is not None:
        rays, lit, dark = ref["shadow_rays"], ref["changed_to_lit"], ref["changed_to_dark"]
        assert lit >= 0.01 * rays and dark >= 0.01 * rays, (what, lit, dark, rays)
        assert lit + dark >= max(20, 0.01 * rays) and lit >= 5 and dark >= 5, (what, lit, dark, rays)   # tests/test_soft_shadows_host.py's condition
    assert np.all(ref["gen_rays"][1:] > 0) and ref["rays"] == ref["gen_rays"].sum(), (what, ref["gen_rays"].tolist())
    if f["sky"]:
        assert ref["sky_terms"] > 0, what
    m = ls.marks(f)
    if "mirror_parts" in m or "mirror_spheres" in m:
        assert np.all(ref["gen_mirror"][1:] > 0), (what, ref["gen_mirror"].tolist())
    else:
        assert ref["gen_mirror"].sum() == 0
    if "glass_parts" in m or "glass_spheres" in m:
        assert all(e > 0 for e in ref["events"]), (what, ref["events"])
    else:
        assert ref["events"] == (0, 0, 0)
    if "gloss_parts" in m or "gloss_spheres" in m:
        assert ref["glossy"] > 0, what
    else:
        assert ref["glossy"] == 0


def test_marks_name_both_ends_of_the_roughness_range_and_every_kind_of_surface():
    assert ls.ROUGH_LOW == 2.0 ** -10 and 0.9 <= ls.ROUGH_HIGH <= 1.0
    for name, variants in ls.MARKS.items():
        for kind in ("mirror", "glass", "gloss"):
            assert set(variants[kind]) == {kind + "_parts", kind + "_spheres"}, (name, kind)
        rough = {r for v in ("gloss", "all") for k in ("gloss_parts", "gloss_spheres") for r, _ in variants[v].get(k, {}).values()}
        assert ls.ROUGH_LOW in rough and ls.ROUGH_HIGH in rough, name
        assert {k.split("_")[0] for k in variants["all"]} == {"mirror", "glass", "gloss"}, name
        surfaces = [(k.split("_")[1], i) for k, d in variants["all"].items() for i in d]
        assert len(surfaces) == len(set(surfaces)), name    # one model per surface


def test_the_limit_frames_differ_in_the_last_face(soft, rwr, orc, ref_loader, suzanne, cube):
    """soup_4096's face 4 095 - the one soup_4095 lacks - is seen at sample 0, so the two frames of every limit pair differ."""
    n = len(ls.LIMIT) // 2
    for a, b in zip(ls.LIMIT[:n], ls.LIMIT[n:]):
        assert (a["scene"], b["scene"]) == ("soup_4095", "soup_4096") and a["radii"] == b["radii"]
        ra, rb = (ls.reference(soft, rwr, orc, ref_loader, suzanne, cube, f) for f in (a, b))
        last = rb["obj_id"] == ls.SOUP_FACES - 1
        assert last.sum() >= 20 and not (ra["obj_id"] == ls.SOUP_FACES - 1).any()
        assert np.array_equal(ra["obj_id"][~last], rb["obj_id"][~last])
        assert ra["color_f32"].tobytes() != rb["color_f32"].tobytes()


@pytest.mark.parametrize("name", SCENES + ("skewed",))
def test_build_bvh(bvh_lib, corners, name):
    """Every face index in exactly one leaf, leaf links that decode to a range inside leaf_faces, faces ascending inside a leaf,
    child boxes that hold every corner below them, inner links below the node count, a depth within kBvhMaxDepth (the skewed scene
    by the median rebuild, the others as the SAH tree), and for soup_4095 links that fit the 15 bits of a 16-bit stack entry."""
    tri = ls.skewed_corners() if name == "skewed" else corners[name]
    bvh = bvh_host.build(bvh_lib, tri)
    got = bvh_host.check(bvh, tri, name)
    print(f"{name}: {len(tri)} faces, {len(bvh['child'])} nodes, depth {bvh['depth']} (SAH {bvh['sah_depth']}), largest leaf link "
          f"{int(got['leaf_links'].max())}, largest inner link {int(got['inner_links'].max())}")
    assert bvh["max_depth"] == 12 and bvh["max_leaf"] == 2
    if name == "skewed":
        assert bvh["sah_depth"] > bvh["max_depth"] >= bvh["depth"]        # rebuilt
    else:
        assert bvh["sah_depth"] == bvh["depth"] <= bvh["max_depth"]       # the SAH tree itself
    if name == "soup_4095":   # what lane_lds_plan's STACK16 relies on
        assert got["leaf_links"].max() < 0x8000 and got["inner_links"].max() < 0x8000 and len(bvh["child"]) <= 0x7fff
    # the largest link a leaf can have: the last face alone in a leaf
    assert got["leaf_links"].max() <= ((len(tri) - 1) << 3)
