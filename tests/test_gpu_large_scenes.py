"""The path tracer on scenes beyond the per-lane BVH kernels' 16-bit traversal stacks (csrc/rwr_bvh.h lane_lds_plan: 32-bit stack
entries from 4 096 world faces on), against the tests' CPU reference (soft_shadow_ref.c: the whole stack, brute force over faces).
The scenes and frames are tests/large_scenes.py's; tests/test_large_scenes_host.py asserts with the reference alone that they can
fail.  The bars are the project's own: sample-0 planes bit-exact, RGBA8 within one code, colour within 1e-4 (path_cases.color_bar
for the deeper paths; no sky component here is above 1), every count equal.  rwr_last_traversal_plan says after every frame
which form its stages ran, and the test prints it with the colour error.

  a. at the limit: the soups of 4 095 and 4 096 faces - 16-bit entries for the first, 32-bit for the second, in both stages;
  b. every extension beyond the limit: the plain path at depth 0, 1 and 4, hard and soft shadows, sky, each surface model and all
     three, a normal map - on the instanced cube and on the scene of two parts;
  c. schedules (Z-split, queues, group size, packets forced on and off, frames in flight, culling off, a band) give one frame;
  d. RWR_WF_STACK16=0 on the small scenes the suite already trusts: the forced 32-bit forms give the 16-bit forms' bytes, among
     them the form with the nodelets in LDS and 32-bit entries, which no scene reaches by itself;
  e. rows and strips through the loopback gather, and K frames of s samples against one of K s."""
import os

import numpy as np
import pytest

import large_scenes as ls
import mirror_common
import path_cases as pc
import shadow_common as sc
import soft_shadow_ref as ssr

pytestmark = pytest.mark.gpu
COLOR_TOL = 1e-4   # the project's bar at depth <= 1 (tests/test_gpu_shadows.py, tests/test_gpu_soft_shadows.py)
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
COUNTS = ("stats", "shadow", "glass", "glossy")
# every pool to the per-lane kernels, whatever the pools' size (the frames here have at most twelve tiles - fewer pools than the
# packet kernel is given by default - so this only holds what the defaults do)
LANE_ONLY = {"RWR_WF_PACKET_RAYS": "0", "RWR_WF_MIN_PACKET_POOLS": "100000"}
SWEEP_KEYS = ("RWR_WF_ZSPLIT", "RWR_WF_OVERLAP", "RWR_WF_GROUP", "RWR_WF_PACKET_RAYS", "RWR_WF_MIN_PACKET_POOLS", "RWR_WF_WIDE_LANE")


class unset:
    """path_cases.environment's opposite: the variable is absent while a context is made."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.saved = os.environ.pop(self.name, None)

    def __exit__(self, *exc):
        if self.saved is not None:
            os.environ[self.name] = self.saved


@pytest.fixture(scope="module")
def soft(tmp_path_factory):
    return ssr.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def lane_ctx(rwr):
    """A context whose trace stage runs per lane alone, with lane_lds_plan's own choice of the stack entries."""
    with unset("RWR_WF_STACK16"), pc.environment(LANE_ONLY):
        ctx = rwr.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def stack_pair(rwr):
    """(a context created with RWR_WF_STACK16=0, one created without the variable)."""
    with pc.environment(dict(LANE_ONLY, RWR_WF_STACK16="0")):
        forced = rwr.Context(0)
    with unset("RWR_WF_STACK16"), pc.environment(LANE_ONLY):
        default = rwr.Context(0)
    yield forced, default
    forced.close()
    default.close()


def _flags(rwr, f, scene_flags, extra=0):
    m = f["marks"]
    return (rwr.FLAG_AUX_OUTPUTS | extra | scene_flags | (rwr.FLAG_MULTI_BOUNCE if f["bounces"] > 1 else 0) | (rwr.FLAG_SHADOWS if f["shadows"] else 0) |
            (rwr.FLAG_SOFT_SHADOWS if f["radii"] is not None else 0) | (rwr.FLAG_SKY if f["sky"] else 0) |
            (rwr.FLAG_MIRRORS if "mirror_parts" in m or "mirror_spheres" in m else 0) | (rwr.FLAG_GLASS if "glass_parts" in m or "glass_spheres" in m else 0) |
            (rwr.FLAG_GLOSSY if "gloss_parts" in m or "gloss_spheres" in m else 0))


def _upload(ctx, s, w, h, marks):
    """The scene (an upload makes every part the diffuse surface it is), every sphere slot cleared of all three models (the sphere
    attributes outlive the spheres), then the frame's marks."""
    model, spheres, inst = s[0], s[1], s[2]
    if isinstance(model, (list, tuple)):
        ctx.upload_parts(list(model))
    else:
        ctx.upload_model(model)
    ctx.set_instances(inst)
    ctx.set_spheres(spheres)
    ctx.resize(w, h)
    for k in range(8):
        ctx.set_sphere_gloss(k, 0.5, None)
    for k, r in marks.get("mirror_parts", {}).items():
        ctx.set_part_mirror(k, r)
    for k, r in marks.get("mirror_spheres", {}).items():
        ctx.set_sphere_mirror(k, r)
    for k, (ior, tint) in marks.get("glass_parts", {}).items():
        ctx.set_part_glass(k, ior, tint)
    for k, (ior, tint) in marks.get("glass_spheres", {}).items():
        ctx.set_sphere_glass(k, ior, tint)
    for k, (rough, refl) in marks.get("gloss_parts", {}).items():
        ctx.set_part_gloss(k, rough, refl)
    for k, (rough, refl) in marks.get("gloss_spheres", {}).items():
        ctx.set_sphere_gloss(k, rough, refl)


def _render(rwr, ctx, f, s, cam_inv, w, h, upload=True, extra=0, spp=None, **kw):
    """f: a frame of large_scenes' shape with its marks under "marks"."""
    if upload:
        _upload(ctx, s, w, h, f["marks"])
    ctx.sky_set_params(*ls.SKY)
    if f["radii"] is not None:
        ctx.shadow_set_params(*f["radii"])
    ctx.render(cam_inv.view(rwr.CAMERA_INV_DTYPE), rwr.make_params(spp=spp or f["spp"], max_bounces=f["bounces"], seed=f["seed"], flags=_flags(rwr, f, s[5], extra)), **kw)
    out = ctx.readback(aux=True)
    out["stats"] = ctx.last_render_stats()
    out["shadow"] = ctx.last_shadow_stats()
    out["glass"] = ctx.last_glass_stats()
    out["glossy"] = ctx.last_gloss_stats()
    out["plan"] = ctx.last_traversal_plan()
    return out


def _same(a, b, what, counts=True):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    for k in COUNTS if counts else ():
        assert a[k] == b[k], (what, k, a[k], b[k])


def _check_plan(got, f, stack16, what):
    """Each stage the frame has launched per lane, with the entries expected; a stage it lacks reports nothing at all."""
    for stage, present in (("trace", f["bounces"] > 0), ("shadow", f["shadows"])):
        p = got["plan"][stage]
        if present:
            assert p["launches"] > 0 and p["stack16"] == int(stack16), (what, stage, p)
            assert not p["wide"] or (p["stack16"] and p["nodes_in_lds"] and stage == "trace"), (what, stage, p)
        else:
            assert p == {"launches": 0, "nodes_in_lds": 0, "stack16": 0, "wide": 0}, (what, stage, p)


def _check(got, want, f, w, h, what, spp=None):
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"large scenes {what}: worst colour error {err:.3g}; plan trace {got['plan']['trace']} shadow {got['plan']['shadow']}; "
          f"rays {got['stats']} shadow {got['shadow']} glass {got['glass']} glossy {got['glossy']}")
    bar = COLOR_TOL if f["bounces"] <= 1 else pc.color_bar({"sky": f["sky"], "sky_colors": ls.SKY})
    assert err <= bar, (what, err, bar)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, what
    assert got["stats"] == (w * h * (spp or f["spp"]), want["rays"]), (what, got["stats"], want["rays"], want["gen_rays"].tolist())
    assert got["shadow"] == (want["shadow_rays"], want["occluded"]), (what, got["shadow"], want["shadow_rays"], want["occluded"])
    assert got["glass"] == want["events"], (what, got["glass"], want["events"])
    assert got["glossy"] == want["glossy"], (what, got["glossy"], want["glossy"])


def _against_the_reference(soft, rwr, orc, ref_loader, suzanne, cube, ctx, f):
    s = ls.scene(f["scene"], rwr, orc, ref_loader, suzanne, cube)
    w, h = ls.SIZES[f["scene"]]
    want = ls.reference(soft, rwr, orc, ref_loader, suzanne, cube, f)
    got = _render(rwr, ctx, dict(f, marks=ls.marks(f)), s, ls.camera(rwr, orc, s, w, h), w, h)
    what = ls.describe(f)
    _check(got, want, f, w, h, what)
    _check_plan(got, f, ls.N_FACES[f["scene"]] <= ls.STACK16_MAX_FACES, what)
    return got


# ------------------------------------------------------------------ a. at the limit --
@pytest.mark.parametrize("i", range(len(ls.LIMIT)), ids=[ls.describe(f).replace(" ", "_") for f in ls.LIMIT])
def test_at_the_limit(soft, rwr, orc, ref_loader, suzanne, cube, lane_ctx, i):
    """4 095 faces: the last scene with 16-bit entries; 4 096: the first with 32-bit ones.  Shadows, both pairs of soft radii, sky,
    depth 4; both stages launched per lane and say which entries they had."""
    f = ls.LIMIT[i]
    got = _against_the_reference(soft, rwr, orc, ref_loader, suzanne, cube, lane_ctx, f)
    for stage in ("trace", "shadow"):
        assert got["plan"][stage]["launches"] > 0 and got["plan"][stage]["stack16"] == int(f["scene"] == "soup_4095"), (stage, got["plan"])


# ------------------------------------------------------------------ b. every extension beyond the limit --
@pytest.mark.parametrize("i", range(len(ls.LADDER)), ids=[ls.describe(f).replace(" ", "_") for f in ls.LADDER])
def test_every_extension_beyond_the_limit(soft, rwr, orc, ref_loader, suzanne, cube, lane_ctx, i):
    f = ls.LADDER[i]
    got = _against_the_reference(soft, rwr, orc, ref_loader, suzanne, cube, lane_ctx, f)
    for stage in ("trace", "shadow"):
        assert got["plan"][stage]["stack16"] == 0 and got["plan"][stage]["nodes_in_lds"] == 0, (stage, got["plan"])   # (a BVH of this size never fits LDS)


# ------------------------------------------------------------------ c. schedules --
def test_schedules_give_the_same_frame_on_a_large_scene(soft, rwr, orc, ref_loader, suzanne, cube):
    """tests/test_gpu_soft_shadows.py's sweep of the tunables on the instanced cube at depth 3 with soft shadows and a glossy part:
    the same bytes and counts from every schedule, with culling off, and in a band; the first frame against the reference."""
    f = ls.SCHEDULES
    s = ls.scene(f["scene"], rwr, orc, ref_loader, suzanne, cube)
    w, h = ls.SIZES[f["scene"]]
    cam_inv = ls.camera(rwr, orc, s, w, h)
    want = ls.reference(soft, rwr, orc, ref_loader, suzanne, cube, f)
    fm = dict(f, marks=ls.marks(f))
    saved = {k: os.environ.get(k) for k in SWEEP_KEYS}
    frames = []
    try:
        for zsplit, queues, group, dense, wide, fif in (("1", "1", "32", "0", "0", 1), ("4", "1", "32", "0", "1", 2),
                                                        ("3", "2", "3", "0", "0", 3), ("0", "3", "4", "0", "1", 2),
                                                        ("1", "1", "32", "40", "0", 1), ("4", "2", "4", "400", "1", 2)):
            os.environ.update({"RWR_WF_ZSPLIT": zsplit, "RWR_WF_OVERLAP": queues, "RWR_WF_GROUP": group, "RWR_WF_PACKET_RAYS": dense,
                               "RWR_WF_MIN_PACKET_POOLS": "0" if dense != "0" else "128", "RWR_WF_WIDE_LANE": wide})
            what = (zsplit, queues, group, dense, wide, fif)
            with rwr.Context(0) as c:        # the tunables are read when the context is created
                c.set_frames_in_flight(fif)
                got = _render(rwr, c, fm, s, cam_inv, w, h)
                again = _render(rwr, c, fm, s, cam_inv, w, h, upload=False)   # (zsplit 0: from the live count)
                third = _render(rwr, c, fm, s, cam_inv, w, h, upload=False)
                nocull = _render(rwr, c, fm, s, cam_inv, w, h, upload=False, extra=rwr.FLAG_NO_CULL)
                band = _render(rwr, c, fm, s, cam_inv, w, h, upload=False, rows=(24, 56))
            if not frames:
                _check(got, want, f, w, h, f"schedule {what}")
            for other in (got, again, third, nocull, band):
                _check_plan(other, f, False, what)
            for other in (again, third, nocull):
                _same(got, other, what)
            for k in PLANES:
                assert np.array_equal(got[k][24:56].view(np.uint8), band[k][24:56].view(np.uint8)), (what, k, "band")
            frames.append(got)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for fr in frames[1:]:
        _same(fr, frames[0], "schedules")


# ------------------------------------------------------------------ d. the forced 32-bit forms --
SMALL = tuple(sc.MIXED) + ("parts_grid",)
SMALL_DEPTH = dict(zip(SMALL, (1, 4, 4, 1, 4, 1, 4)))


def _small_scene(name, rwr, orc, ref_loader, suzanne, cube):
    if name == "parts_grid":
        m = mirror_common.scene(name, rwr, ref_loader, suzanne, cube)
        return (m["model"], m["spheres"].view(orc.SPHERE_DTYPE), m["instances"].view(orc.INSTANCE_DTYPE), m["eye"], m["target"], 0)
    return sc.scene(name, rwr, orc, suzanne, cube)


def _small_marks(s):
    """large_scenes.MARKS' variants on a small scene: its last part, sphere slots 0 and 1 (a slot the scene leaves empty does nothing)."""
    part = len(s[0]) - 1 if isinstance(s[0], (list, tuple)) else 0
    r, tint = (0.9, 0.8, 0.7), (0.95, 0.9, 1.0)
    return {"mirror": dict(mirror_parts={part: r}, mirror_spheres={0: (0.9, 0.9, 0.9)}),
            "glass": dict(glass_parts={part: (1.5, tint)}, glass_spheres={1: (1.33, (1.0, 1.0, 1.0))}),
            "gloss": dict(gloss_parts={part: (ls.ROUGH_LOW, r)}, gloss_spheres={0: (ls.ROUGH_HIGH, (0.8, 0.9, 1.0))}),
            "all": dict(mirror_spheres={0: (0.9, 0.9, 0.9)}, glass_spheres={1: (1.33, (1.0, 1.0, 1.0))}, gloss_parts={part: (ls.ROUGH_HIGH, r)})}


_in_lds_with_wide_entries = set()


@pytest.mark.parametrize("name", SMALL)
def test_forced_32_bit_entries_give_the_16_bit_frames(rwr, orc, ref_loader, suzanne, cube, stack_pair, name):
    """A context created with RWR_WF_STACK16=0 against a default one, on scenes whose frames the suite holds to the reference
    elsewhere, under part b's ladder at one depth: every plane and every count the same bytes; the diagnostic says 0 against 1."""
    forced, default = stack_pair
    s = _small_scene(name, rwr, orc, ref_loader, suzanne, cube)
    w, h = sc.W, sc.H
    cam_inv = ls.camera(rwr, orc, s, w, h)
    depth = SMALL_DEPTH[name]
    variants = _small_marks(s)
    ladder = [dict(spp=2, bounces=depth), dict(spp=2, bounces=depth, shadows=True), dict(spp=2, bounces=depth, radii=ls.RADII[0]),
              dict(spp=3, bounces=depth, radii=ls.RADII[1]), dict(spp=2, bounces=depth, radii=ls.RADII[0], sky=True)]
    ladder += [dict(spp=2, bounces=depth, radii=ls.RADII[0], sky=True, variant=v) for v in ("mirror", "glass", "gloss", "all")]
    for step in ladder:
        f = dict(scene=name, shadows=False, radii=None, sky=False, variant=None, seed=13)
        f.update(step)
        f["shadows"] = f["shadows"] or f["radii"] is not None
        f["marks"] = variants[f["variant"]] if f["variant"] else {}
        what = ls.describe(f)
        a = _render(rwr, forced, f, s, cam_inv, w, h)
        b = _render(rwr, default, f, s, cam_inv, w, h)
        _same(a, b, what)
        assert a["stats"][1] > 0 and (not f["shadows"] or a["shadow"][0] > 0), (what, a["stats"], a["shadow"])   # both stages had rays
        _check_plan(a, f, False, what)
        _check_plan(b, f, True, what)
        print(f"large scenes forced {what}: plan trace {a['plan']['trace']} shadow {a['plan']['shadow']} against {b['plan']['trace']} {b['plan']['shadow']}")
        for stage in ("trace", "shadow"):
            if a["plan"][stage]["nodes_in_lds"]:
                _in_lds_with_wide_entries.add((name, stage))
    # the smallest BVH (111 faces: some 5 KiB of nodelets and 14 KiB of 32-bit stacks, within lane_lds_plan's 28 KiB) runs both
    # stages in the form no scene reaches by itself: nodelets in LDS and 32-bit entries
    if name == "suzanne_side":
        assert {("suzanne_side", "trace"), ("suzanne_side", "shadow")} <= _in_lds_with_wide_entries


# ------------------------------------------------------------------ e. splits --
@pytest.mark.parametrize("strips", [True, False], ids=["strips", "rows"])
def test_splits_assemble_the_one_gpu_frame(soft, rwr, orc, ref_loader, suzanne, cube, strips):
    f = ls.SPLITS
    s = ls.scene(f["scene"], rwr, orc, ref_loader, suzanne, cube)
    w, h = ls.SIZES[f["scene"]]
    cam_inv = ls.camera(rwr, orc, s, w, h)
    fm = dict(f, marks=ls.marks(f))
    n = 3
    with unset("RWR_WF_STACK16"), rwr.Context(0) as c:
        full = _render(rwr, c, fm, s, cam_inv, w, h)
        _check(full, ls.reference(soft, rwr, orc, ref_loader, suzanne, cube, f), f, w, h, f"splits, the whole frame ({'strips' if strips else 'rows'})")
        asm = {k: np.zeros_like(full[k]) for k in PLANES}
        total = {k: np.zeros(len(np.atleast_1d(full[k])), np.int64) for k in ("shadow",)}
        for r in range(n):
            if strips:
                part = _render(rwr, c, fm, s, cam_inv, w, h, upload=False, strips=(r, n))
                rows = [y for y in range(h) if (y // 8) % n == r]
            else:
                band = rwr.dist_band(r, n, h)
                part = _render(rwr, c, fm, s, cam_inv, w, h, upload=False, rows=band)
                rows = list(range(*band))
            _check_plan(part, f, False, (strips, r))
            total["shadow"] += np.array(part["shadow"], np.int64)
            for k in PLANES:
                asm[k][rows] = part[k][rows]
            c.dist_loopback_deposit(r, n, strips)
        c.dist_loopback_finish(n, strips)
        _same(asm, full, (strips, n), counts=False)
        assert tuple(int(v) for v in total["shadow"]) == full["shadow"], (strips, total, full["shadow"])
        assert np.array_equal(c.dist_readback(), full["color"]), (strips, n)


def test_accumulation_of_k_frames_is_one_frame_of_k_s(rwr, orc, ref_loader, suzanne, cube, lane_ctx):
    f = ls.SPLITS
    s = ls.scene(f["scene"], rwr, orc, ref_loader, suzanne, cube)
    w, h = ls.SIZES[f["scene"]]
    cam_inv = ls.camera(rwr, orc, s, w, h)
    fm = dict(f, marks=ls.marks(f))
    K, s_ = 2, f["spp"] // 2
    want = _render(rwr, lane_ctx, fm, s, cam_inv, w, h)
    lane_ctx.accum_reset()
    total = np.zeros(2, np.int64)
    for k in range(1, K + 1):
        got = _render(rwr, lane_ctx, fm, s, cam_inv, w, h, upload=False, extra=rwr.FLAG_ACCUMULATE, spp=s_)
        assert lane_ctx.accum_samples() == k * s_
        _check_plan(got, f, False, ("accumulation", k))
        total += np.array(got["shadow"], np.int64)   # its own samples
    _same(got, want, (K, s_), counts=False)
    assert tuple(int(v) for v in total) == want["shadow"]
    lane_ctx.accum_reset()


# ------------------------------------------------------------------ the diagnostic and the tunable themselves --
def test_the_plan_record_and_the_tunables_values(rwr, orc, ref_loader, suzanne, cube):
    """Zeros before the first wavefront frame; a frame from the frame kernel leaves the last wavefront frame's record; NULL
    arguments are refused; RWR_WF_STACK16 of any value but 0 leaves the rule alone - it cannot give a scene beyond the limit 16-bit
    entries - and 0 switches them off."""
    import ctypes as C
    none = {"launches": 0, "nodes_in_lds": 0, "stack16": 0, "wide": 0}
    small = sc.scene("suzanne_side", rwr, orc, suzanne, cube)
    large = ls.scene("soup_4096", rwr, orc, ref_loader, suzanne, cube)
    f = dict(scene="", spp=2, bounces=1, shadows=True, radii=None, sky=False, variant=None, seed=5, marks={})
    for value, small16 in ((None, 1), ("1", 1), ("16", 1), ("-1", 1), ("", 1), ("off", 1), ("0", 0)):
        with unset("RWR_WF_STACK16"), pc.environment({} if value is None else {"RWR_WF_STACK16": value}), rwr.Context(0) as c:
            assert c.last_traversal_plan() == {"trace": none, "shadow": none}
            got = _render(rwr, c, f, small, ls.camera(rwr, orc, small, 48, 32), 48, 32)
            assert got["plan"]["trace"]["stack16"] == got["plan"]["shadow"]["stack16"] == small16, (value, got["plan"])
            assert got["plan"]["trace"]["launches"] == 1 and got["plan"]["shadow"]["launches"] == 2, (value, got["plan"])
            c.render(ls.camera(rwr, orc, small, 48, 32).view(rwr.CAMERA_INV_DTYPE), rwr.make_params())   # the frame kernel: no wavefront frame
            assert c.last_traversal_plan() == got["plan"], value
            got = _render(rwr, c, f, large, ls.camera(rwr, orc, large, 48, 32), 48, 32)
            assert got["plan"]["trace"]["stack16"] == got["plan"]["shadow"]["stack16"] == 0, (value, got["plan"])
            no_bounce = _render(rwr, c, dict(f, bounces=0, shadows=False), large, ls.camera(rwr, orc, large, 48, 32), 48, 32, upload=False)
            assert no_bounce["plan"] == {"trace": none, "shadow": none}, value
            four = np.zeros(4, np.uint32)
            p = four.ctypes.data_as(C.c_void_p)
            L = rwr.lib()
            assert L.rwr_last_traversal_plan(None, p, p) == rwr.ERR_INVALID_ARGUMENT
            assert L.rwr_last_traversal_plan(c._h, None, p) == rwr.ERR_INVALID_ARGUMENT
            assert L.rwr_last_traversal_plan(c._h, p, None) == rwr.ERR_INVALID_ARGUMENT
