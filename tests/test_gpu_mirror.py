"""Mirror surfaces (RWR_FLAG_MIRRORS) on the GPU: the MIRROR forms of the primary kernel and of the trace kernels'
EMIT forms against the tests' CPU reference (mirror_ref.c):
  * sample-0 planes (object id, distance, depth) bit-exact, bounce-ray and shadow-ray counts equal (from the second generation on
    they depend on where every reflected ray landed), colour within the bar tests/test_gpu_multi_bounce.py holds deeper paths to
    (COLOR_TOL there, read from that file: a reflectance <= 1 travels through the same unorm16 throughput as an albedo);
  * the closed form of the mirror quad;
  * every schedule, split, frames in flight and accumulation: the same bytes;
  * frames the flag does nothing to, the accumulation key, the validation, the denoiser behind it.
The scenes are tests/mirror_common.py's; tests/test_mirror_host.py asserts with the reference alone that they exercise the mirrors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref
import mirror_common
import mirror_ref
import sky_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# the colour bar of the deeper paths, for the same B: not a tolerance of this file's own
COLOR_TOL = float(re.search(r"^COLOR_TOL\s*=\s*([0-9.eE+-]+)", open(os.path.join(HERE, "test_gpu_multi_bounce.py")).read(), re.M).group(1))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
DEFAULT = (sky_ref.DEFAULT_ZENITH, sky_ref.DEFAULT_HORIZON)
MAX_SPHERES = mirror_ref.MAX_SPHERES


@pytest.fixture(scope="module")
def mref(tmp_path_factory):
    return mirror_ref.lib(tmp_path_factory)


def _no_sphere_mirrors(c):
    for i in range(MAX_SPHERES):
        c.set_sphere_mirror(i, None)


@pytest.fixture()
def ctx(gpu_ctx):
    """The shared context, left as it was found: default sky, no mirror sphere (the part attributes go with the next upload), no
    instances, no accumulation."""
    gpu_ctx.sky_set_params()
    _no_sphere_mirrors(gpu_ctx)
    yield gpu_ctx
    gpu_ctx.sky_set_params()
    _no_sphere_mirrors(gpu_ctx)
    gpu_ctx.set_instances(None)
    gpu_ctx.accum_reset()


def _flags(rwr, bounces, mirrors=True, sky=True, shadows=False, extra=0):
    return (rwr.FLAG_AUX_OUTPUTS | extra | (rwr.FLAG_MULTI_BOUNCE if bounces > 1 else 0) | (rwr.FLAG_SHADOWS if shadows else 0) |
            (rwr.FLAG_SKY if sky else 0) | (rwr.FLAG_MIRRORS if mirrors else 0))


def _upload(c, s, mirrors=True):
    if isinstance(s["model"], (list, tuple)):
        c.upload_parts(s["model"])
    else:
        c.upload_model(s["model"])
    c.set_instances(s["instances"])
    c.set_spheres(s["spheres"])
    c.resize(s["w"], s["h"])
    _no_sphere_mirrors(c)
    if mirrors:
        for k, r in s["mirror_parts"].items():
            c.set_part_mirror(k, r)
        for k, r in s["mirror_spheres"].items():
            c.set_sphere_mirror(k, r)


def _frame(c, cam_inv, params, **kw):
    c.render(cam_inv, params, **kw)
    out = c.readback(aux=True)
    out["stats"] = c.last_render_stats()
    out["shadow"] = c.last_shadow_stats()
    return out


def _same(a, b, what=""):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _check(got, want, what):
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"mirror colour error {what}: {err:.3g} (bar {COLOR_TOL:.3g})")
    assert err <= COLOR_TOL, (what, err)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, what


@pytest.mark.parametrize("sky", [True, False], ids=["sky", "dark"])
@pytest.mark.parametrize("shadows", [False, True], ids=["plain", "shadows"])
@pytest.mark.parametrize("name", mirror_common.GPU_SCENES)
def test_matches_the_reference(rwr, orc, mref, ctx, ref_loader, suzanne, cube, name, shadows, sky):
    s = mirror_common.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = mirror_common.camera(rwr, s)
    _upload(ctx, s)
    spp, bounces = s["spp"], s["bounces"]
    got = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=bounces, seed=13, flags=_flags(rwr, bounces, sky=sky, shadows=shadows)))
    want = mirror_common.reference(mref, rwr, orc, s, 13, sky=DEFAULT if sky else None, shadows=shadows, first=not shadows and sky, name=name)
    assert want["gen_mirror"][1] > 0 and want["gen_mirror"][2] > 0          # reflections from h0 and from h1
    _check(got, want, f"{name} shadows={shadows} sky={sky}")
    # the counts: from generation 2 on they depend on where every reflected ray went
    assert got["stats"] == (s["w"] * s["h"] * spp, want["rays"]), (name, want["gen_rays"].tolist())
    assert got["shadow"] == ((want["shadow_rays"], want["occluded"]) if shadows else (0, 0))
    # sample-0 planes do not depend on the flag, nor does the first generation's ray count
    off = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=1, seed=13, flags=_flags(rwr, 1, mirrors=False, sky=sky, shadows=shadows)))
    for k in ("obj_id", "hit_t", "depth"):
        assert got[k].tobytes() == off[k].tobytes(), (name, k)
    assert off["stats"][1] == want["gen_rays"][1]


def test_closed_form_of_the_mirror_quad(rwr, orc, mref, ctx, ref_loader, suzanne, cube):
    """tests/test_mirror_host.py's closed form against the GPU's frame: E(h0) + clamp(R * S(D')), the sky term recomputed in numpy
    from the D' the reference exports."""
    f = np.float32
    s = mirror_common.scene("quad_alone", rwr, ref_loader, suzanne, cube)
    cam_inv = mirror_common.camera(rwr, s)
    _upload(ctx, s)
    got = _frame(ctx, cam_inv, rwr.make_params(spp=1, max_bounces=1, seed=3, flags=_flags(rwr, 1)))
    ref = mirror_common.reference(mref, rwr, orc, s, 3, sky=DEFAULT, first=True, name="quad_alone")
    e0 = mirror_common.reference(mref, rwr, orc, s, 3, sky=DEFAULT, bounces=0, name="quad_alone")
    hit = ref["obj_id"] >= 0
    assert hit.any() and ref["gen_mirror"][1] == hit.sum() == ref["sky_terms"]
    d1 = ref["first"][:, :, 0, 0:3]
    z, hz = np.asarray(DEFAULT[0], f), np.asarray(DEFAULT[1], f)
    u = np.minimum(np.maximum(f(0.5) * d1[..., 1] + f(0.5), f(0.0)), f(1.0)).astype(f)
    S = (hz + ((z - hz) * u[..., None]).astype(f)).astype(f)
    term = np.clip((np.asarray(mirror_common.QUAD_R, f) * S).astype(f), f(0.0), f(64.0)) * hit[..., None]
    want = (e0["color_f32"][..., :3] + term.astype(f)).astype(f)
    assert np.array_equal(got["obj_id"], ref["obj_id"])
    err = float(np.abs(got["color_f32"][..., :3] - want).max())
    print(f"mirror quad, closed form: {err:.3g} (bar {COLOR_TOL:.3g})")
    assert err <= COLOR_TOL
    assert got["stats"] == (s["w"] * s["h"], int(hit.sum()))


_STATS = re.compile(r"rwr wavefront pools: packets (\d+) pools / (\d+) rays, per-lane (\d+) pools / (\d+) rays.*\n"
                    r"rwr wavefront launches: packet (\d+), per-lane (\d+), per-lane wide (\d+)")


@pytest.mark.parametrize("name", ["soup", "cube_grid"])
def test_schedules_give_the_same_frame(rwr, orc, mref, ref_loader, suzanne, cube, capfd, name):
    """The schedule overrides tests/test_gpu_sky.py exercises: packets forced (dense 40 / 400, no minimum of packet pools), per-lane
    forced (no dense rule, a minimum of 128 packet pools), the 1 024-thread LDS form asked for and not, listed tiles (a forced
    split).  Which kernels did run is read from the context's own account (RWR_WF_STATS=1, printed when it is destroyed)."""
    s = mirror_common.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = mirror_common.camera(rwr, s)
    params = rwr.make_params(spp=s["spp"], max_bounces=s["bounces"], seed=13, flags=_flags(rwr, s["bounces"]))
    want = mirror_common.reference(mref, rwr, orc, s, 13, sky=DEFAULT, first=True, name=name)
    keys = ("RWR_WF_ZSPLIT", "RWR_WF_OVERLAP", "RWR_WF_GROUP", "RWR_WF_PACKET_RAYS", "RWR_WF_MIN_PACKET_POOLS", "RWR_WF_WIDE_LANE", "RWR_WF_STATS")
    saved = {k: os.environ.get(k) for k in keys}
    h = s["h"]
    band_rows = (8, min(h, 24))
    ran = {"packet": False, "lane": False, "wide": False}
    try:
        with rwr.Context(0) as c:
            _upload(c, s)
            default = _frame(c, cam_inv, params)
        _check(default, want, f"schedule {name} default")
        assert default["stats"][1] == want["rays"]
        capfd.readouterr()
        for zsplit, queues, group, dense, wide in (("1", "1", "32", "0", "0"), ("4", "1", "32", "0", "1"), ("3", "2", "2", "0", "0"),
                                                   ("1", "2", "3", "0", "1"), ("0", "4", "1", "0", "0"), ("8", "3", "4", "0", "1"),
                                                   ("1", "1", "32", "40", "0"), ("4", "2", "4", "400", "1")):
            os.environ.update({"RWR_WF_ZSPLIT": zsplit, "RWR_WF_OVERLAP": queues, "RWR_WF_GROUP": group, "RWR_WF_PACKET_RAYS": dense,
                               "RWR_WF_MIN_PACKET_POOLS": "0" if dense != "0" else "128", "RWR_WF_WIDE_LANE": wide, "RWR_WF_STATS": "1"})
            what = (zsplit, queues, group, dense, wide)
            with rwr.Context(0) as c:        # the tunables are read when the context is created
                _upload(c, s)
                got = _frame(c, cam_inv, params)
                again = _frame(c, cam_inv, params)   # (zsplit 0: now from the first frame's live count)
                band = _frame(c, cam_inv, params, rows=band_rows)
            _same(got, default, what)
            _same(again, default, what)
            for k in PLANES:
                assert got[k][band_rows[0]:band_rows[1]].tobytes() == band[k][band_rows[0]:band_rows[1]].tobytes(), (what, k, "band")
            assert got["stats"] == default["stats"], what
            m = _STATS.search(capfd.readouterr().err)
            assert m, what
            p_pools, p_rays, l_pools, l_rays, n_packet, n_lane, n_wide = map(int, m.groups())
            with capfd.disabled():
                print(f"schedule {name} {what}: packet pools {p_pools} ({p_rays} rays), per-lane pools {l_pools} ({l_rays} rays), "
                      f"launches packet {n_packet} / per-lane {n_lane} / wide {n_wide}")
            assert p_rays + l_rays == 2 * got["stats"][1] + band["stats"][1], what     # every bounce ray went through a pool
            if dense != "0" and p_pools > 0:
                assert n_packet > 0, what
                ran["packet"] = True
            if l_pools > 0 or (dense == "0" and p_pools < 128):
                assert n_wide + n_lane > 0, what
                ran["wide" if n_wide > 0 else "lane"] = True
            assert (n_wide == 0) if wide == "0" else (n_lane == 0 or n_wide == 0), what
            if name == "cube_grid":   # four cubes' BVH: too large for a copy per 256-thread workgroup, so the switch decides
                assert (n_wide > 0 and n_lane == 0) if wide == "1" else (n_lane > 0 and n_wide == 0), what
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    # mirror frames reach the packet form and the per-lane form on either scene, and the wide form where the BVH asks for it
    assert ran["packet"] and ran["lane"], ran
    if name == "cube_grid":
        assert ran["wide"], ran


@pytest.mark.parametrize("name", ["soup", "cube_grid"])
@pytest.mark.parametrize("split", ["strips", "bands", "in_flight"])
def test_splits_assemble_the_frame(rwr, ref_loader, suzanne, cube, split, name):
    s = mirror_common.scene(name, rwr, ref_loader, suzanne, cube)
    s = dict(s, spp=min(s["spp"], 6))
    w, h = s["w"], s["h"]
    cam_inv = mirror_common.camera(rwr, s)
    params = rwr.make_params(spp=s["spp"], max_bounces=s["bounces"], seed=2, flags=_flags(rwr, s["bounces"], shadows=True))
    with rwr.Context(0) as c:
        _upload(c, s)
        full = _frame(c, cam_inv, params)
        c.render(cam_inv, rwr.make_params(spp=s["spp"], max_bounces=s["bounces"], seed=2, flags=_flags(rwr, s["bounces"], mirrors=False, shadows=True)))
        assert c.readback(aux=True)["color_f32"].tobytes() != full["color_f32"].tobytes()      # the mirrors are in the frame
        if split == "in_flight":
            for n in (1, 2, 3):
                c.set_frames_in_flight(n)
                for i in range(n + 1):
                    _same(_frame(c, cam_inv, params), full, (n, i))
            return
        for n in (2, 3):
            asm = {k: np.zeros_like(full[k]) for k in PLANES}
            rays, shadow = 0, [0, 0]
            for r in range(n):
                if split == "strips":
                    part = _frame(c, cam_inv, params, strips=(r, n))
                    rows = [y for y in range(h) if (y // 8) % n == r]
                else:
                    band = rwr.dist_band(r, n, h)
                    part = _frame(c, cam_inv, params, rows=band)
                    rows = list(range(*band))
                rays += part["stats"][1]
                shadow[0] += part["shadow"][0]; shadow[1] += part["shadow"][1]
                for k in PLANES:
                    asm[k][rows] = part[k][rows]
                c.dist_loopback_deposit(r, n, split == "strips")
            c.dist_loopback_finish(n, split == "strips")
            _same(asm, full, (split, n))
            assert rays == full["stats"][1] and tuple(shadow) == full["shadow"]
            assert np.array_equal(c.dist_readback(), full["color"]), (split, n)


@pytest.mark.parametrize("name", ["soup", "cube_grid"])
def test_accumulated_frames_are_one_frame_of_all_samples(rwr, ctx, ref_loader, suzanne, cube, name):
    s = mirror_common.scene(name, rwr, ref_loader, suzanne, cube)
    cam_inv = mirror_common.camera(rwr, s)
    _upload(ctx, s)
    flags = _flags(rwr, s["bounces"])
    want = _frame(ctx, cam_inv, rwr.make_params(spp=8, max_bounces=s["bounces"], seed=11, flags=flags))
    ctx.accum_reset()
    acc = rwr.make_params(spp=2, max_bounces=s["bounces"], seed=11, flags=flags | rwr.FLAG_ACCUMULATE)
    for k in range(1, 5):
        ctx.render(cam_inv, acc)
        assert ctx.accum_samples() == 2 * k
    _same(ctx.readback(aux=True), want, "4 x 2 spp")


def test_accumulation_key(rwr, ctx, ref_loader, suzanne, cube):
    """The rule implemented (include/rwr_hip.h, RWR_FLAG_MIRRORS item 7): every accepted call of the two setters changes the scene's
    generation, with or without the flag, whether or not the value is new; a refused call changes nothing; the flag (after its
    clearing rule) is one of the key's flags."""
    s = mirror_common.scene("soup", rwr, ref_loader, suzanne, cube)
    cam_inv = mirror_common.camera(rwr, s)
    _upload(ctx, s)
    b = s["bounces"]
    acc = rwr.make_params(spp=2, max_bounces=b, seed=11, flags=_flags(rwr, b) | rwr.FLAG_ACCUMULATE)

    def step(params=acc):
        ctx.render(cam_inv, params)
        return ctx.accum_samples()

    ctx.accum_reset()
    assert step() == 2 and step() == 4
    r = np.asarray(s["mirror_parts"][0], np.float32)
    r[1] = np.nextafter(r[1], np.float32(0.0))                      # one ulp of R
    ctx.set_part_mirror(0, r)
    assert step() == 2 and step() == 4
    ctx.set_sphere_mirror(0, None)                                  # clear
    assert step() == 2 and step() == 4
    ctx.set_sphere_mirror(0, s["mirror_spheres"][0])                # set
    assert step() == 2 and step() == 4
    off = rwr.make_params(spp=2, max_bounces=b, seed=11, flags=_flags(rwr, b, mirrors=False) | rwr.FLAG_ACCUMULATE)
    assert step(off) == 2 and step(off) == 4                        # the flag toggled ...
    assert step() == 2                                              # ... and back
    # with the flag off a setter still changes the scene: sphere 5 is no sphere of this scene, and the accumulation starts over
    assert step(off) == 2 and step(off) == 4
    ctx.set_sphere_mirror(5, (0.5, 0.5, 0.5))
    assert step(off) == 2
    # a refused call changes nothing, the accumulation included - with the flag off and with it on
    assert step(off) == 4
    for bad in (lambda: ctx.set_part_mirror(0, (2.0, 0.0, 0.0)), lambda: ctx.set_sphere_mirror(MAX_SPHERES, None),
                lambda: ctx.set_part_mirror(7, (0.5, 0.5, 0.5)), lambda: ctx.set_sphere_mirror(0, (np.nan, 0.0, 0.0))):
        with pytest.raises(rwr.RwrError):
            bad()
    assert step(off) == 6
    assert step() == 2 and step() == 4
    with pytest.raises(rwr.RwrError):
        ctx.set_sphere_mirror(0, (0.5, -0.5, 0.5))
    assert step() == 6
    # ... and an accepted call that sets the value a surface has already is a call that changes the scene
    ctx.set_sphere_mirror(0, s["mirror_spheres"][0])
    assert step() == 2


def test_frames_the_flag_does_nothing_to(rwr, ctx, ref_loader, suzanne, cube):
    for name in ("soup", "cube_grid", "suzanne"):
        s = mirror_common.scene(name, rwr, ref_loader, suzanne, cube)
        cam_inv = mirror_common.camera(rwr, s)
        b = s["bounces"]
        spp = min(s["spp"], 5)
        with rwr.Context(0) as fresh:      # a context that never heard of mirrors
            _upload(fresh, s, mirrors=False)
            never = {sh: _frame(fresh, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b, mirrors=False, shadows=sh)))
                     for sh in (False, True)}
            flat = {(n, sh): _frame(fresh, cam_inv, rwr.make_params(spp=n, max_bounces=0, seed=5, flags=_flags(rwr, 0, mirrors=False, shadows=sh)))
                    for n, sh in ((1, False), (4, False), (1, True))}
        _upload(ctx, s)
        for sh in (False, True):
            # the flag off, mirrors set
            off = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b, mirrors=False, shadows=sh)))
            _same(off, never[sh], (name, "flag off", sh))
            assert off["stats"] == never[sh]["stats"] and off["shadow"] == never[sh]["shadow"]
            on = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b, shadows=sh)))
            assert on["color_f32"].tobytes() != off["color_f32"].tobytes()
            for k in ("depth", "obj_id", "hit_t"):
                assert on[k].tobytes() == off[k].tobytes(), (name, k)
        # no bounce: the flag is ignored (the reference frame at spp 1 too)
        for (n, sh), want in flat.items():
            on = _frame(ctx, cam_inv, rwr.make_params(spp=n, max_bounces=0, seed=5, flags=_flags(rwr, 0, shadows=sh)))
            _same(on, want, (name, "no bounce", n, sh))
            assert on["stats"] == want["stats"] and on["shadow"] == want["shadow"]
        # every mirror cleared again with NULL, then no mirror ever set (a new upload): the flag alone changes nothing
        for k in s["mirror_parts"]:
            ctx.set_part_mirror(k, None)
        for k in s["mirror_spheres"]:
            ctx.set_sphere_mirror(k, None)
        for what in ("cleared", "never set"):
            if what == "never set":
                _upload(ctx, s, mirrors=False)
            for sh in (False, True):
                on = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b, shadows=sh)))
                _same(on, never[sh], (name, what, sh))
                assert on["stats"] == never[sh]["stats"] and on["shadow"] == never[sh]["shadow"]
        # a mirror on a sphere index the scene does not have is no mirror of the scene
        ctx.set_sphere_mirror(MAX_SPHERES - 1, (1.0, 1.0, 1.0))
        on = _frame(ctx, cam_inv, rwr.make_params(spp=spp, max_bounces=b, seed=5, flags=_flags(rwr, b)))
        _same(on, never[False], (name, "a sphere that is not there"))
        ctx.set_sphere_mirror(MAX_SPHERES - 1, None)


def test_validation(rwr, ctx, ref_loader, suzanne, cube):
    L = rwr.lib()
    s = mirror_common.scene("quad_floor", rwr, ref_loader, suzanne, cube)
    cam_inv = mirror_common.camera(rwr, s)
    _upload(ctx, s, mirrors=False)
    # the defaults, the getters
    assert ctx.get_part_mirror(0) is None and ctx.get_part_mirror(1) is None
    assert all(ctx.get_sphere_mirror(i) is None for i in range(MAX_SPHERES))
    ctx.set_part_mirror(1, (0.25, 0.5, 1.0))
    ctx.set_sphere_mirror(6, (0.0, 1.0, 0.125))
    ctx.set_part_mirror(0)      # reflectance 1, 1, 1
    assert ctx.get_part_mirror(1).tolist() == [0.25, 0.5, 1.0] and ctx.get_sphere_mirror(6).tolist() == [0.0, 1.0, 0.125]
    assert ctx.get_part_mirror(0).tolist() == [1.0, 1.0, 1.0]
    on, r = C.c_int(7), np.full(3, 9.0, np.float32)
    assert L.rwr_scene_get_part_mirror(ctx._h, 1, C.byref(on), None) == rwr.OK and on.value == 1
    assert L.rwr_scene_get_sphere_mirror(ctx._h, 0, None, r.ctypes.data_as(C.c_void_p)) == rwr.OK and r.tolist() == [0.0, 0.0, 0.0]
    # argument errors: the old state survives
    for bad in (-0.1, 1.0001, np.nan, np.inf, -np.inf, np.nextafter(np.float32(1.0), np.float32(2.0)), -1e-30):
        for c in range(3):
            v = np.array([0.5, 0.5, 0.5], np.float32)
            v[c] = bad
            for setter, idx in ((ctx.set_part_mirror, 1), (ctx.set_sphere_mirror, 6), (ctx.set_part_mirror, 0), (ctx.set_sphere_mirror, 2)):
                with pytest.raises(rwr.RwrError) as ei:
                    setter(idx, v)
                assert ei.value.code == rwr.ERR_INVALID_ARGUMENT, (bad, c, idx)
    for setter, getter, idx in ((ctx.set_part_mirror, ctx.get_part_mirror, 2), (ctx.set_part_mirror, ctx.get_part_mirror, 0xffffffff),
                                (ctx.set_sphere_mirror, ctx.get_sphere_mirror, MAX_SPHERES), (ctx.set_sphere_mirror, ctx.get_sphere_mirror, 0xffffffff)):
        for call in (lambda: setter(idx, (0.5, 0.5, 0.5)), lambda: setter(idx, None), lambda: getter(idx)):
            with pytest.raises(rwr.RwrError) as ei:
                call()
            assert ei.value.code == rwr.ERR_INVALID_ARGUMENT, idx
    assert L.rwr_scene_set_part_mirror(None, 0, None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_scene_set_sphere_mirror(None, 0, None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_scene_get_part_mirror(None, 0, None, None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_scene_get_sphere_mirror(None, 0, None, None) == rwr.ERR_INVALID_ARGUMENT
    assert ctx.get_part_mirror(1).tolist() == [0.25, 0.5, 1.0] and ctx.get_sphere_mirror(6).tolist() == [0.0, 1.0, 0.125]
    assert ctx.get_part_mirror(0).tolist() == [1.0, 1.0, 1.0] and ctx.get_sphere_mirror(2) is None
    # the sphere attributes persist across rwr_scene_set_spheres, the part attributes go with the scene
    ctx.set_spheres(rwr.make_spheres([((0.0, 0.0, 0.0), 1.0)]))
    ctx.set_spheres(rwr.make_spheres([]))
    assert ctx.get_sphere_mirror(6).tolist() == [0.0, 1.0, 0.125]
    ctx.upload_parts(s["model"])
    assert ctx.get_part_mirror(0) is None and ctx.get_part_mirror(1) is None and ctx.get_sphere_mirror(6).tolist() == [0.0, 1.0, 0.125]
    ctx.set_part_mirror(1, (0.5, 0.5, 0.5))
    assert L.rwr_scene_clear(ctx._h) == rwr.OK
    with pytest.raises(rwr.RwrError):
        ctx.get_part_mirror(0)             # no parts left
    ctx.upload_model(cube)
    assert ctx.get_part_mirror(0) is None
    ctx.set_sphere_mirror(6, None)
    # reference-frame-only modes refuse the flag: whatever max_bounces is, mirror or no mirror
    _upload(ctx, s)
    for mirrors in (True, False):
        if not mirrors:
            ctx.set_part_mirror(0, None)
        for params in (rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_MIRRORS | rwr.FLAG_ORTHO_RAYS),
                       rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_MIRRORS | rwr.FLAG_USE_BVH),
                       rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_MIRRORS | rwr.FLAG_ORTHO_RAYS),
                       rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_MIRRORS | rwr.FLAG_USE_BVH)):
            with pytest.raises(rwr.RwrError) as ei:
                ctx.render(cam_inv, params)
            assert ei.value.code == rwr.ERR_UNSUPPORTED, params
        ctx.set_triangles(rwr.make_triangles([((0.0, 0.0, -2.0), (1.0, 0.0, -2.0), (0.0, 1.0, -2.0))]))
        try:
            for bounces in (0, 1):
                with pytest.raises(rwr.RwrError) as ei:
                    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=bounces, flags=rwr.FLAG_MIRRORS))
                assert ei.value.code == rwr.ERR_UNSUPPORTED
        finally:
            ctx.set_triangles(rwr.make_triangles())
    ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=1, flags=rwr.FLAG_MIRRORS))   # the context is still usable


def test_denoiser_filters_the_mirror_frame(rwr, orc, mref, ctx, ref_loader, suzanne, cube, tmp_path_factory):
    """With RWR_FLAG_DENOISE the frame is denoise_ref.c applied to the mirror reference's planes, within 1e-4 (the bar
    tests/test_gpu_sky.py holds the filtered sky frame to); background passes through."""
    dref = denoise_ref.lib(tmp_path_factory)
    s = mirror_common.scene("cube_grid", rwr, ref_loader, suzanne, cube)
    s = dict(s, spp=4)
    cam_inv = mirror_common.camera(rwr, s)
    _upload(ctx, s)
    b = s["bounces"]
    ref = mirror_common.reference(mref, rwr, orc, s, 9, sky=DEFAULT, name="cube_grid denoise")
    assert ref["gen_mirror"][1] > 0
    nhat = denoise_ref.face_normals(dref, orc, s["model"], s["instances"].view(orc.INSTANCE_DTYPE))
    want = denoise_ref.denoise(dref, ref["color_f32"], ref["obj_id"], ref["hit_t"], nhat, **denoise_ref.DEFAULTS)
    ctx.set_denoise_params()
    plain = _frame(ctx, cam_inv, rwr.make_params(spp=4, max_bounces=b, seed=9, flags=_flags(rwr, b)))
    got = _frame(ctx, cam_inv, rwr.make_params(spp=4, max_bounces=b, seed=9, flags=_flags(rwr, b) | rwr.FLAG_DENOISE))
    for k in ("depth", "obj_id", "hit_t"):
        assert got[k].tobytes() == ref[k].tobytes(), k
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"denoised mirror frame against the filtered reference: {err:.3g}")
    assert err <= 1e-4
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1
    assert got["color_f32"].tobytes() != plain["color_f32"].tobytes()              # the filter ran
    bg = ref["obj_id"] == -1
    assert bg.any() and np.array_equal(got["color_f32"][bg], plain["color_f32"][bg]) and np.array_equal(got["color"][bg], plain["color"][bg])
