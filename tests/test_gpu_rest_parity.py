"""Frames served from a frame slot's kept state — k_frame_setup's records (frame_records.cpp launch_records) and the plane of ray
directions the two-pixel frame kernel loads from (ray_plane_step, k_ray_plane) — compared with the CPU oracle; the helper and
its model of the slots are tests/rest_common.py.  The bar is the project's: obj_id, hit_t and depth bit for bit, color_f32
within 1e-4, a plain frame's RGBA8 equal to the aux frame's.

The list of cases (rest_common.draw_cases, seed 25, 40 cases) was chosen with the oracle alone; test_case_list_inputs asserts
what was found then: 28 of the 40 cases show at least one mesh pixel and at least one other pixel (the condition: 24), 19 show
a sphere pixel (5), 13 of the 14 far cases show the mesh (3).  Of the three scenes of the smallest-change steps (seed 7, 131x43)
the mesh that replaces soup65 / soup300 / suzanne differs from it in the obj_id of 1014 / 3164 / 1041 pixels; moving one
element of the ray origin by one ulp changes the bits of hit_t in 63 / 139 / 31 pixels, one of the projection inverse in
118 / 734 / 74, one of the inverse view matrix's translation column in none (the rays multiply it by 0: a key that must miss
over a frame that must stay)."""
import numpy as np
import pytest

import rest_common as rc

SEED, N_CASES, GROUP = 25, 40, 5
GROUPS = list(range(N_CASES // GROUP))
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(orc, ref_loader, suzanne, cube):
    return rc.draw_cases(orc, ref_loader, {"suzanne": suzanne, "cube": cube}, SEED, N_CASES)


@pytest.fixture(scope="module")
def wants(orc, cases):
    """The oracle's frame of every case, once for the module."""
    out = []
    for c in cases:
        f = rc.oracle_frame(orc, c["cam"], c["size"], c["spheres"], c["model"])
        for a in f.values():
            a.setflags(write=False)
        out.append(f)
    return out


@pytest.fixture(scope="module")
def scenes(orc, ref_loader, suzanne):
    return rc.step_scenes(orc, ref_loader, suzanne)


@pytest.fixture(scope="module")
def step_oracle(orc):
    return rc.Oracle(orc)


def test_case_list_inputs(orc, cases, wants, scenes, step_oracle):
    """No GPU: the conditions on the inputs, with the oracle alone."""
    assert len(cases) == N_CASES and {c["mesh"] for c in cases} == set(rc.MESHES)
    sizes = [c["size"] for c in cases]
    assert (1, 1) in sizes and (2, 1) in sizes and any(w % 2 and w > 64 for w, h in sizes) and any(w > 64 and h > 8 for w, h in sizes)
    assert all(1 <= w <= 259 and 1 <= h <= 149 and w * h * len(c["model"]["faces"]) <= rc.MAX_WORK for c, (w, h) in zip(cases, sizes))
    assert {c["n_slots"] for c in cases} == {1, 2, 3}
    n_far = sum(c["far"] for c in cases)
    assert n_far == (N_CASES + 2) // 3 and all(np.abs(c["offset"]).max() <= 1e5 for c in cases)
    both, sphere, far_mesh = rc.case_conditions(cases, wants)
    print("cases: mesh and other %d, sphere %d, far with mesh %d of %d" % (both, sphere, far_mesh, n_far))
    assert both >= 0.6 * N_CASES and sphere >= 5 and far_mesh >= 3
    for name, scene in scenes.items():
        swap, proj, origin, column = rc.step_conditions(orc, step_oracle, scene)
        print("%s: obj_id differs in %d pixels after the swap; hit_t in %d (translation column), %d (origin), %d (projection)" % (name, swap, column, origin, proj))
        assert len(scene["other"]["faces"]) == len(scene["model"]["faces"]) and len(scene["other"]["vertices"]) == len(scene["model"]["vertices"])
        assert swap >= 1 and origin >= 1 and proj >= 1 and column == 0
    assert len(scenes["soup65"]["model"]["faces"]) <= rc.FACE_SET_MAX_FACES < len(scenes["soup300"]["model"]["faces"])


@gpu
@pytest.mark.parametrize("group", GROUPS)
def test_rest_sequences(rwr, orc, cases, wants, group):
    """Five cases on one modelled context (the state of one case carries into the next): each rests for 2 n + 2 frames, so that
    every slot's last frame loads its rays from the kept plane on kept records (rest_common.rest asserts it from the model, and
    the library's counters against the model after every frame), then for n frames more, each a pure load on kept records.
    Every frame is compared with the oracle."""
    with rc.tracked(rwr, mp=pytest.MonkeyPatch()) as ctx:
        for c, want in list(zip(cases, wants))[GROUP * group: GROUP * (group + 1)]:
            n = c["n_slots"]
            ctx.upload(c["model"]); ctx.set_spheres(c["spheres"]); ctx.resize(*c["size"]); ctx.set_slots(n)
            rc.rest(ctx, n, rc.Call(c["cam"]), want, 2 * n + 2, (c["name"],))
            rc.rest(ctx, n, rc.Call(c["cam"]), want, n, (c["name"], "loads"), loaded=True)   # a pure load on every slot
        assert ctx.slots.served > 0 and ctx.worst <= 1e-4


@gpu
@pytest.mark.parametrize("n_slots", [1, 2, 3])
@pytest.mark.parametrize("scene", ["soup65", "soup300", "suzanne"])
def test_smallest_changes(rwr, orc, scenes, step_oracle, scene, n_slots):
    """Steps 3a-3h of rest_common.run_steps on one long-lived modelled context: a same-size mesh swap (the scene generation
    alone tells the two apart), a sphere by one ulp, the camera by one ulp and back, rows and strips (a band from row 3, a
    clipped last strip), resizes (to the same size too), frames in flight 1 -> 3 -> 2 -> 1, the other frame kernels and the
    integrator between resting frames, single-triangle passes and orthographic rays.  Every frame is compared with the oracle's
    frame of its own inputs.
    Frames in flight, as rwr_ctx_set_frames_in_flight has it: slots below the new count keep what they hold (targets, records,
    plane), the others give everything up and start over when taken into use again, and the turn goes to slot 0 when the slot
    rendered last is gone (the next frame then takes slot 1 % n)."""
    with rc.tracked(rwr, mp=pytest.MonkeyPatch()) as ctx:
        rc.run_steps(ctx, orc, step_oracle, scenes[scene], n_slots)
        assert ctx.worst <= 1e-4


@gpu
@pytest.mark.parametrize("group", GROUPS)
def test_default_rules(rwr, orc, cases, wants, group):
    """The same cases with no knobs set (small plain frames with frames in flight fuse, small faces go to the BVH kernel), plain
    and aux frames alternating, on a context with the plane and on one with RWR_RAY_PLANE=0: no model of the counts (they must
    never fall, and stay zero without the plane); every frame is compared with the oracle."""
    with rc.tracked(rwr, modelled=False, mp=pytest.MonkeyPatch()) as on, rc.tracked(rwr, modelled=False, plane=False, mp=pytest.MonkeyPatch()) as off:
        for c, want in list(zip(cases, wants))[GROUP * group: GROUP * (group + 1)]:
            for ctx in (on, off):
                rc.run_default_rules(ctx, orc, c, want)
        assert off.counters[1:] == (0, 0)
