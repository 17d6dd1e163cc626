"""The Owen-scrambled Sobol sample sequence (RWR_FLAG_SOBOL) on the GPU:
  * the kernels' device function, word for word against the definition (tests/sobol_ref.py);
  * frames against the stacked CPU references drawing the same words (sobol_ref's switched library): sample-0 planes and every
    count exact, colour within the bar the scenes' own GPU tests use - COLOR_TOL of tests/test_gpu_multi_bounce.py, read from that
    file, times the largest Le where something emits;
  * every schedule, split, accumulation: the same bytes; the keys; frames the flag does nothing to; the refusals.
The scenes are tests/sobol_common.py's, taken from the other features' common modules."""
import os
import re

import numpy as np
import pytest

import path_cases
import refusals_common
import sobol_common as sc
import sobol_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
COLOR_TOL = float(re.search(r"^COLOR_TOL\s*=\s*([0-9.eE+-]+)", open(os.path.join(HERE, "test_gpu_multi_bounce.py")).read(), re.M).group(1))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
COUNTS = ("stats", "shadow", "glass", "glossy", "emissive", "light", "part")
MAX_SPHERES = 8


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return sobol_ref.lib(tmp_path_factory)


def _plain_spheres(c):
    for i in range(MAX_SPHERES):
        c.set_sphere_gloss(i, 0.5, None)     # (any of the three model setters with None makes the surface diffuse)
        c.set_sphere_emission(i, None)


@pytest.fixture()
def ctx(gpu_ctx):
    """The shared context, left as it was found."""
    gpu_ctx.sky_set_params()
    _plain_spheres(gpu_ctx)
    yield gpu_ctx
    gpu_ctx.sky_set_params()
    gpu_ctx.shadow_set_params(0.0, 0.0)
    _plain_spheres(gpu_ctx)
    gpu_ctx.set_instances(None)
    gpu_ctx.set_frames_in_flight(1)
    gpu_ctx.accum_reset()
    gpu_ctx.reproject_reset()


def _upload(c, s):
    if isinstance(s["model"], (list, tuple)):
        c.upload_parts(s["model"])
    else:
        c.upload_model(s["model"])
    c.set_instances(s["instances"])
    c.set_spheres(s["spheres"])
    c.resize(s["w"], s["h"])
    _plain_spheres(c)
    c.sky_set_params()
    c.shadow_set_params(*(s["radii"] or (0.0, 0.0)))
    for k, r in s["mirror_parts"].items():
        c.set_part_mirror(k, r)
    for k, (ior, tint) in s["glass_spheres"].items():
        c.set_sphere_glass(k, ior, tint)
    for k, (rough, refl) in s["gloss_parts"].items():
        c.set_part_gloss(k, rough, refl)
    for k, le in s["emissive_parts"].items():
        c.set_part_emission(k, le)
    for k, le in s["emissive_spheres"].items():
        c.set_sphere_emission(k, le)


def _frame(c, cam_inv, params, **kw):
    c.render(cam_inv, params, **kw)
    out = c.readback(aux=True)
    out["stats"] = c.last_render_stats()
    out["shadow"] = c.last_shadow_stats()
    out["glass"] = c.last_glass_stats()
    out["glossy"] = c.last_gloss_stats()
    out["emissive"] = c.last_emission_stats()
    out["light"] = c.last_light_stats()
    out["part"] = c.last_part_light_stats()
    return out


def _same(a, b, what=""):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _same_counts(a, b, what=""):
    for k in COUNTS:
        assert a[k] == b[k], (what, k, a[k], b[k])


def _params(rwr, s, spp, seed=13, bounces=None, sobol=True, extra=0):
    b = s["bounces"] if bounces is None else bounces
    return rwr.make_params(spp=spp, max_bounces=b, seed=seed, flags=sc.flags(rwr, s, bounces=b, sobol=sobol, extra=extra))


def test_the_device_function_is_the_definition(rwr, ctx):
    """4 096 tuples, bit for bit: samples 0, 1, 31, 32, 33, 2^16, 2^31, 2^32 - 1 and every one-bit index; dimensions 0, 1, 2, 17, 130,
    131, 290; the rest random."""
    rng = np.random.default_rng(23)
    n = 4096
    pixel = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    sample = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    dim = rng.integers(0, 300, n, dtype=np.uint64)
    seed = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    samples = [0, 1, 31, 32, 33, 2 ** 16, 2 ** 31, 2 ** 32 - 1] + [1 << b for b in range(32)]
    dims = [0, 1, 2, 17, 130, 131, 290]
    k = 0
    for s_ in samples:
        for d in dims:
            sample[k], dim[k] = s_, d
            k += 1
    pixel[k:k + 64] = np.arange(64)
    sample[k + 64:k + 64 + 4096 // 8] = np.arange(4096 // 8)
    seed[:8] = (0, 1, 2, 3, 2 ** 31, 2 ** 32 - 1, 13, 0x9E3779B9)
    got = ctx.selftest_sobol(pixel, sample, dim, seed)
    want = sobol_ref.rng_sobol(pixel, sample, dim, seed)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    assert ctx.selftest_sobol([], [], [], []).size == 0


@pytest.mark.parametrize("spp,bounces", sc.SPP_PLANS)
@pytest.mark.parametrize("name", tuple(sc.PARITY))
def test_matches_the_reference(rwr, orc, sref, ctx, ref_loader, suzanne, cube, name, spp, bounces):
    s = sc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    b = s["bounces"] if bounces is None else bounces
    cam_inv = sc.camera(rwr, s)
    _upload(ctx, s)
    got = _frame(ctx, cam_inv, _params(rwr, s, spp, bounces=b))
    want = sc.reference(sref, rwr, orc, s, 13, spp, name, bounces=b)
    what = f"{name} spp={spp} bounces={b}"
    for k in ("obj_id", "hit_t", "depth"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)
    assert got["stats"] == (s["w"] * s["h"] * spp, want["rays"]), (what, want["gen_rays"].tolist())
    assert got["shadow"] == ((want["shadow_rays"], want["occluded"]) if s["shadows"] else (0, 0)), what
    assert got["glass"] == want["events"] and got["glossy"] == want["glossy"], what
    if sc.emits(s):
        assert got["emissive"] == want["emissive_hits"], (what, want["gen_glow"].tolist())
        assert got["light"] == (want["light_rays"], want["reached"], want["suppressed"]), (what, want["light_gen"].tolist())
        assert got["part"] == want["part_light"], (what, want["part_gen"].tolist())
        if s["mis"] and b:
            assert want["mis"][0] + want["mis"][1] == want["suppressed"]
    bar = COLOR_TOL * sc.bar_factor(s)
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    print(f"sobol colour error {what}: {err:.3g} (bar {bar:.3g}); rays {got['stats'][1]}, shadow {got['shadow']}, glass {got['glass']}, glossy {got['glossy']}, "
          f"emissive {got['emissive']}, light {got['light']}, part {got['part']}")
    assert err <= bar, (what, err)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, what
    if spp > 1 or b:      # the sequence is not the hash: the frame without the flag differs (and is the hashed reference's, to the same bar)
        off = _frame(ctx, cam_inv, _params(rwr, s, spp, bounces=b, sobol=False))
        assert off["color_f32"].tobytes() != got["color_f32"].tobytes(), what


def _with_env(rwr, env, s, cam_inv, params):
    keys = sorted(set(env) | {"RWR_WF_GROUP", "RWR_WF_PACKET_FILL", "RWR_WF_PACKET_EXTENT", "RWR_WF_MIN_PACKET_POOLS", "RWR_WF_STACK16"})
    saved = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(env)
        with rwr.Context(0) as c:        # the tunables are read when the context is created
            _upload(c, s)
            return _frame(c, cam_inv, params)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture()
def lamp_room(rwr, orc, sref, ctx, ref_loader, suzanne, cube):
    """The lamp-lit room at 64 x 40, 33 spp (sphere light sampling and MIS): the default schedule's frame, vouched for by the reference."""
    s = sc.scene("lamp_room", rwr, ref_loader, suzanne, cube, orc)
    cam_inv = sc.camera(rwr, s)
    params = _params(rwr, s, 33)
    _upload(ctx, s)
    full = _frame(ctx, cam_inv, params)
    want = sc.reference(sref, rwr, orc, s, 13, 33, "lamp_room")
    assert (s["w"], s["h"]) == (64, 40) and full["stats"][1] == want["rays"] and full["light"] == (want["light_rays"], want["reached"], want["suppressed"])
    assert full["light"][1] > 0 and float(np.abs(full["color_f32"] - want["color_f32"]).max()) <= COLOR_TOL * sc.bar_factor(s)
    return s, cam_inv, params, full


@pytest.mark.parametrize("what,env", (("forced packets, launch groups of five", dict(path_cases.FORCED_SCHEDULE)), ("32-bit stacks", {"RWR_WF_STACK16": "0"})))
def test_schedules_give_the_same_bytes(rwr, lamp_room, what, env):
    s, cam_inv, params, full = lamp_room
    got = _with_env(rwr, env, s, cam_inv, params)
    _same(got, full, what)
    _same_counts(got, full, what)


def test_frames_in_flight_strips_bands_and_the_gather(rwr, ctx, lamp_room):
    s, cam_inv, params, full = lamp_room
    h = s["h"]
    for n in (1, 2, 3):
        ctx.set_frames_in_flight(n)
        for i in range(n + 1):
            got = _frame(ctx, cam_inv, params)
            _same(got, full, (n, i))
            _same_counts(got, full, (n, i))
    ctx.set_frames_in_flight(1)
    for n in (2, 3):       # strips of n ranks, the loopback gather
        asm = {k: np.zeros_like(full[k]) for k in PLANES}
        rays, light = 0, np.zeros(3, np.int64)
        for r in range(n):
            part = _frame(ctx, cam_inv, params, strips=(r, n))
            rows = [y for y in range(h) if (y // 8) % n == r]
            rays += part["stats"][1]
            light += np.asarray(part["light"])
            for k in PLANES:
                asm[k][rows] = part[k][rows]
            ctx.dist_loopback_deposit(r, n, True)
        ctx.dist_loopback_finish(n, True)
        _same(asm, full, ("strips", n))
        assert rays == full["stats"][1] and tuple(light.tolist()) == full["light"], n
        assert np.array_equal(ctx.dist_readback(), full["color"]), n
    asm = {k: np.zeros_like(full[k]) for k in PLANES}
    light = np.zeros(3, np.int64)
    for band in ((0, 16), (16, h)):
        part = _frame(ctx, cam_inv, params, rows=band)
        light += np.asarray(part["light"])
        for k in PLANES:
            asm[k][band[0]:band[1]] = part[k][band[0]:band[1]]
    _same(asm, full, "bands")
    assert tuple(light.tolist()) == full["light"]


def test_three_frames_of_11_samples_are_one_frame_of_33(rwr, ctx, lamp_room):
    s, cam_inv, params, full = lamp_room
    acc = _params(rwr, s, 11, extra=rwr.FLAG_ACCUMULATE)
    ctx.accum_reset()
    counts, rays = np.zeros(3, np.int64), 0
    for k in range(1, 4):
        ctx.render(cam_inv, acc)
        assert ctx.accum_samples() == 11 * k
        counts += np.asarray(ctx.last_light_stats())      # (an accumulating frame counts its own samples)
        rays += ctx.last_render_stats()[1]
    _same(ctx.readback(aux=True), full, "3 x 11 spp")
    assert tuple(counts.tolist()) == full["light"] and rays == full["stats"][1]


def test_the_flag_is_part_of_both_keys(rwr, ctx, ref_loader, suzanne, cube, orc):
    s = sc.scene("lamp_room", rwr, ref_loader, suzanne, cube, orc)
    cam_inv = sc.camera(rwr, s)
    _upload(ctx, s)
    acc, off = _params(rwr, s, 2, seed=11, extra=rwr.FLAG_ACCUMULATE), _params(rwr, s, 2, seed=11, sobol=False, extra=rwr.FLAG_ACCUMULATE)
    rep, rep_off = _params(rwr, s, 2, seed=11, extra=rwr.FLAG_REPROJECT), _params(rwr, s, 2, seed=11, sobol=False, extra=rwr.FLAG_REPROJECT)

    def step(params=acc):
        ctx.render(cam_inv, params)
        return ctx.accum_samples()

    def history(params=rep):
        ctx.render(cam_inv, params)
        return ctx.reproject_frames()

    ctx.accum_reset()
    assert step() == 2 and step() == 4
    assert step(off) == 2 and step(off) == 4                    # the flag toggled: the accumulation starts over ...
    assert step() == 2 and step() == 4                          # ... and back
    ctx.reproject_reset()
    assert history() == 1 and history() == 2
    assert history(rep_off) == 1 and history(rep_off) == 2      # the reprojection history likewise
    assert history() == 1 and history() == 2


def test_the_flag_does_something_and_only_where_it_should(rwr, ctx, ref_loader, suzanne, cube, orc):
    s = sc.scene("cube", rwr, ref_loader, suzanne, cube, orc)
    cam_inv = sc.camera(rwr, s)
    _upload(ctx, s)
    on, off = _frame(ctx, cam_inv, _params(rwr, s, 4)), _frame(ctx, cam_inv, _params(rwr, s, 4, sobol=False))
    assert on["color_f32"].tobytes() != off["color_f32"].tobytes() and on["stats"][0] == off["stats"][0]
    # spp 1, no bounce, no other flag: the reference frame's kernels, the flag cleared - the unflagged frame byte for byte
    plain = _frame(ctx, cam_inv, rwr.make_params(spp=1, max_bounces=0, seed=13, flags=rwr.FLAG_AUX_OUTPUTS))
    flagged = _frame(ctx, cam_inv, rwr.make_params(spp=1, max_bounces=0, seed=13, flags=rwr.FLAG_AUX_OUTPUTS | rwr.FLAG_SOBOL))
    _same(flagged, plain, "spp 1, no bounce")
    _same_counts(flagged, plain, "spp 1, no bounce")
    bare = rwr.make_params(spp=1, max_bounces=0, seed=13, flags=rwr.FLAG_SOBOL)
    ctx.render(cam_inv, bare)
    assert ctx.readback()["color"].tobytes() == plain["color"].tobytes()
    # an accumulating frame takes the integrator whatever its spp, so there the flag is effective and part of the key
    acc_on = rwr.make_params(spp=1, max_bounces=0, seed=13, flags=rwr.FLAG_ACCUMULATE | rwr.FLAG_SOBOL)
    acc_off = rwr.make_params(spp=1, max_bounces=0, seed=13, flags=rwr.FLAG_ACCUMULATE)
    ctx.accum_reset()
    ctx.render(cam_inv, acc_on)
    ctx.render(cam_inv, acc_on)
    assert ctx.accum_samples() == 2
    ctx.render(cam_inv, acc_off)
    assert ctx.accum_samples() == 1


def test_refusals(rwr, ctx, ref_loader, suzanne, cube, orc):
    """RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes refuse the flag - the code and the message - and leave the
    context usable."""
    s = sc.scene("cube", rwr, ref_loader, suzanne, cube, orc)
    cam_inv = sc.camera(rwr, s)
    _upload(ctx, s)
    text = refusals_common.OFF_REFERENCE % "SOBOL"
    for params in (rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_SOBOL | rwr.FLAG_ORTHO_RAYS),
                   rwr.make_params(spp=1, max_bounces=0, flags=rwr.FLAG_SOBOL | rwr.FLAG_USE_BVH),
                   rwr.make_params(spp=2, max_bounces=1, flags=rwr.FLAG_SOBOL | rwr.FLAG_ORTHO_RAYS)):
        with pytest.raises(rwr.RwrError) as ei:
            ctx.render(cam_inv, params)
        assert ei.value.code == rwr.ERR_UNSUPPORTED and text in str(ei.value), (params, str(ei.value))
    ctx.set_triangles(rwr.make_triangles([((0.0, 0.0, -2.0), (1.0, 0.0, -2.0), (0.0, 1.0, -2.0))]))
    try:
        for bounces in (0, 1):
            with pytest.raises(rwr.RwrError) as ei:
                ctx.render(cam_inv, rwr.make_params(spp=1, max_bounces=bounces, flags=rwr.FLAG_SOBOL))
            assert ei.value.code == rwr.ERR_UNSUPPORTED and text in str(ei.value), str(ei.value)
    finally:
        ctx.set_triangles(rwr.make_triangles())
    got = _frame(ctx, cam_inv, _params(rwr, s, 2))          # the context is still usable
    assert got["stats"][0] == s["w"] * s["h"] * 2
