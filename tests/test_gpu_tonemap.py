"""Tone mapping and exposure (RWR_FLAG_TONEMAP) on the GPU against the tests' CPU reference (tonemap_ref.c).
The scheme is tests/test_gpu_denoise.py's: the frame without the flag (AUX), mapped by the reference, against the frame with the flag:
  * rgba8 IDENTICAL - the stage is multiplies, adds and one IEEE division in a fixed order: a differing byte is a bug, not a tolerance;
    colour_f32, depth, id and t identical to the plain frame's; log_sum and count equal to the reference's, E equal as bits;
  * frames in flight with alternating parameters, a frame without the flag after one with it, the stage behind the filter and behind
    the reprojection stage, accumulation, refusals and parameters, the device targets.
The frames are tests/tonemap_common.py's; tests/test_tonemap_host.py asserts on the CPU path reference that they hold what this relies on."""
import ctypes as C

import numpy as np
import pytest

import emission_common as ec
import tonemap_common as tc
import tonemap_ref as tr

pytestmark = pytest.mark.gpu
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
KEPT = ("depth", "color_f32", "obj_id", "hit_t")
MAX_SPHERES = 8
PART_FRAME = "RWR_FLAG_TONEMAP: the stage needs the whole frame (the exposure is measured over all of it)"
A = dict(curve=tr.ACES, auto_exposure=1, exposure=1.0, key=0.18, white=4.0)
B = dict(curve=tr.REINHARD, auto_exposure=0, exposure=0.4, key=0.3, white=2.0)


@pytest.fixture(scope="module")
def tref(tmp_path_factory):
    return tr.lib(tmp_path_factory)


def _plain_spheres(c):
    for i in range(MAX_SPHERES):
        c.set_sphere_gloss(i, 0.5, None)     # (any of the three model setters with None makes the surface diffuse)
        c.set_sphere_emission(i, None)


@pytest.fixture()
def ctx(rwr, gpu_ctx):
    """The shared context, left as it was found: default parameters, plain dark spheres, no instances, no history, one frame in flight."""
    def clean():
        gpu_ctx.set_frames_in_flight(1)
        gpu_ctx.set_tonemap_params()
        gpu_ctx.set_denoise_params()
        gpu_ctx.set_reproject_params()
        gpu_ctx.sky_set_params()
        gpu_ctx.set_instances(None)
        gpu_ctx.set_triangles(rwr.make_triangles())
        gpu_ctx.accum_reset()
        _plain_spheres(gpu_ctx)
    clean()
    yield gpu_ctx
    clean()


def _upload(c, s):
    if isinstance(s["model"], (list, tuple)):
        c.upload_parts(s["model"])
    else:
        c.upload_model(s["model"])
    c.set_instances(s["instances"])
    c.set_spheres(s["spheres"])
    c.resize(s["w"], s["h"])
    _plain_spheres(c)
    for k, r in s["mirror_parts"].items():
        c.set_part_mirror(k, r)
    for k, le in s["emissive_parts"].items():
        c.set_part_emission(k, le)
    for k, le in s["emissive_spheres"].items():
        c.set_sphere_emission(k, le)


def _frame(c, cam_inv, params, **kw):
    c.render(cam_inv, params, **kw)
    out = c.readback(aux=True)
    out["tonemap"] = c.last_tonemap_stats()
    return out


def _same(a, b, what="", planes=PLANES):
    for k in planes:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _params(rwr, s, spp, bounces=None, extra=0, seed=13):
    bounces = s["bounces"] if bounces is None else bounces
    return rwr.make_params(spp=spp, max_bounces=bounces, seed=seed, flags=ec.flags(rwr, s, bounces=bounces, extra=extra))


def _mapped(rwr, params):
    """The same call with the flag and without RWR_FLAG_AUX_OUTPUTS: the stage implies the aux planes."""
    p = params.copy()
    p["flags"] = (p["flags"] & ~np.uint32(rwr.FLAG_AUX_OUTPUTS)) | np.uint32(rwr.FLAG_TONEMAP)
    return p


def _check(tref, got, plain, tp, what):
    """got: the frame with the flag under parameters tp; plain: the frame without it."""
    want = tr.tonemap(tref, plain["color_f32"], **{**tr.DEFAULTS, **tp})
    _same(got, plain, what, KEPT)
    log_sum, count, E = got["tonemap"]
    print(f"tonemap {what}: log_sum {log_sum} count {count} E {E!r} (reference {want['log_sum']} {want['count']} {float(want['exposure'])!r}); "
          f"{int((got['color'] != plain['color']).any(axis=2).sum())} of {plain['obj_id'].size} pixels change, "
          f"{int((got['color'] != want['color']).sum())} bytes differ from the reference")
    assert (log_sum, count) == (want["log_sum"], want["count"]), what
    assert tr.bits(E) == tr.bits(want["exposure"]), what
    if not tp.get("auto_exposure"):
        assert (log_sum, count) == (0, 0) and tr.bits(E) == tr.bits(tp.get("exposure", 1.0)), what
    assert got["color"].tobytes() == want["color"].tobytes(), what
    return want


@pytest.mark.parametrize("spp", tc.SPPS)
@pytest.mark.parametrize("frame", tc.FRAMES, ids=lambda f: tc.label(*f))
def test_matches_the_reference(rwr, tref, ctx, ref_loader, suzanne, cube, frame, spp):
    s = tc.sized(rwr, ref_loader, suzanne, cube, *frame)
    cam_inv = ec.camera(rwr, s)
    _upload(ctx, s)
    plain = _frame(ctx, cam_inv, _params(rwr, s, spp))
    assert plain["tonemap"] == (0, 0, 0.0)                       # a frame without the flag
    assert float(plain["color_f32"][..., :3].max()) > 1.0
    changed = 0
    for tp in tc.PARAMS:
        ctx.set_tonemap_params()
        ctx.set_tonemap_params(**tp)
        got = _frame(ctx, cam_inv, _mapped(rwr, _params(rwr, s, spp)))
        _check(tref, got, plain, tp, (tc.label(*frame), spp, tp))
        changed += int((got["color"] != plain["color"]).any())
    assert changed == len(tc.PARAMS)                             # every set moves some byte of every frame


def test_a_reference_frame_request_goes_to_the_integrator(rwr, tref, ctx, ref_loader, suzanne, cube):
    """spp 1, no bounce, no other flag: alone the request is the reference's frame kernel's; with the flag it is the integrator's
    frame - its sample-0 planes are the reference frame's, and its colour is what the integrator resolves."""
    s = tc.sized(rwr, ref_loader, suzanne, cube, "tiny", 70, 13)
    cam_inv = ec.camera(rwr, s)
    _upload(ctx, s)
    ctx.set_tonemap_params(**A)
    got = _frame(ctx, cam_inv, rwr.make_params(spp=1, max_bounces=0, seed=13, flags=rwr.FLAG_TONEMAP))   # (the aux planes are there: implied)
    ref_frame = _frame(ctx, cam_inv, rwr.make_params(spp=1, max_bounces=0, seed=13, flags=rwr.FLAG_AUX_OUTPUTS))
    _same(got, ref_frame, "sample-0 planes", ("depth", "obj_id", "hit_t"))
    assert float(np.abs(got["color_f32"] - ref_frame["color_f32"]).max()) <= 1e-4   # the project's bar between the two kernels' colours
    want = tr.tonemap(tref, got["color_f32"], **A)
    assert want["count"] > 0 and got["color"].tobytes() == want["color"].tobytes()
    assert got["tonemap"][:2] == (want["log_sum"], want["count"]) and tr.bits(got["tonemap"][2]) == tr.bits(want["exposure"])
    assert got["color"].tobytes() != ref_frame["color"].tobytes() and ref_frame["tonemap"] == (0, 0, 0.0)


def test_a_frame_large_enough_for_the_measure_to_stride(rwr, tref, ctx, ref_loader, suzanne, cube):
    """1024 x 520 = 532 480 pixels: more than the 2 048 x 256 the measure's capped grid covers in one round."""
    s = tc.sized(rwr, ref_loader, suzanne, cube, "room", 1024, 520)
    cam_inv = ec.camera(rwr, s)
    _upload(ctx, s)
    plain = _frame(ctx, cam_inv, _params(rwr, s, 1, bounces=1))
    ctx.set_tonemap_params(**A)
    got = _frame(ctx, cam_inv, _mapped(rwr, _params(rwr, s, 1, bounces=1)))
    _check(tref, got, plain, A, "1024x520")


@pytest.mark.parametrize("fif", (2, 3))
def test_frames_in_flight_with_alternating_parameters(rwr, tref, ctx, ref_loader, suzanne, cube, fif):
    """Frames follow each other without a wait, their parameters alternating: the last one's bytes and stats are its own, whichever
    slot it landed in and whatever the frame before it measured."""
    s = tc.sized(rwr, ref_loader, suzanne, cube, "room", 70, 13)
    cam_inv = ec.camera(rwr, s)
    _upload(ctx, s)
    plain = _frame(ctx, cam_inv, _params(rwr, s, 3))
    mapped = _mapped(rwr, _params(rwr, s, 3))
    ctx.set_frames_in_flight(fif)
    lasts = []
    for run in range(2 * fif + 1):               # 2, 3, ... frames back to back: the last one is B's, A's, B's, ... in every slot in turn
        last = None
        for k in range(run + 2):
            last = (A, B)[k % 2]
            ctx.set_tonemap_params(**last)
            ctx.render(cam_inv, mapped)
        got = ctx.readback(aux=True)
        got["tonemap"] = ctx.last_tonemap_stats()
        _check(tref, got, plain, last, ("in flight", fif, run))
        lasts.append(last["curve"])
    assert set(lasts) == {A["curve"], B["curve"]}


def test_flag_off_after_flag_on(rwr, tref, ctx, ref_loader, suzanne, cube):
    s = tc.sized(rwr, ref_loader, suzanne, cube, "room", 70, 13)
    cam_inv = ec.camera(rwr, s)
    _upload(ctx, s)
    plain = _frame(ctx, cam_inv, _params(rwr, s, 2))
    ctx.set_tonemap_params(**A)
    for fif in (1, 2):
        ctx.set_frames_in_flight(fif)
        on = _frame(ctx, cam_inv, _mapped(rwr, _params(rwr, s, 2)))
        assert on["color"].tobytes() != plain["color"].tobytes() and on["tonemap"][1] > 0
        off = _frame(ctx, cam_inv, _params(rwr, s, 2))
        _same(off, plain, ("flag off after flag on", fif))
        assert off["tonemap"] == (0, 0, 0.0)


def test_behind_the_filter_and_behind_the_reprojection_stage(rwr, tref, ctx, ref_loader, suzanne, cube):
    """The stage maps what the filter, or the reprojection stage, left in colour_f32."""
    s = tc.sized(rwr, ref_loader, suzanne, cube, "room", 70, 13)
    cam_inv = ec.camera(rwr, s)
    _upload(ctx, s)
    plain = _frame(ctx, cam_inv, _params(rwr, s, 2))
    for tp in (A, B):
        ctx.set_tonemap_params(**tp)
        dn = _frame(ctx, cam_inv, _params(rwr, s, 2, extra=rwr.FLAG_DENOISE))
        assert dn["color_f32"].tobytes() != plain["color_f32"].tobytes()     # the filter did something
        got = _frame(ctx, cam_inv, _mapped(rwr, _params(rwr, s, 2, extra=rwr.FLAG_DENOISE)))
        _check(tref, got, dn, tp, ("behind the filter", tp["curve"]))
        # two frames of a history, the parameters changing between them: the history goes on and never sees the stage
        ctx.reproject_reset()
        for _ in range(2):
            rp = _frame(ctx, cam_inv, _params(rwr, s, 2, extra=rwr.FLAG_REPROJECT))
        assert ctx.reproject_frames() == 2 and rp["color_f32"].tobytes() != plain["color_f32"].tobytes()
        ctx.reproject_reset()
        ctx.set_tonemap_params(**(B if tp is A else A))
        _frame(ctx, cam_inv, _mapped(rwr, _params(rwr, s, 2, extra=rwr.FLAG_REPROJECT)))
        ctx.set_tonemap_params(**tp)
        got = _frame(ctx, cam_inv, _mapped(rwr, _params(rwr, s, 2, extra=rwr.FLAG_REPROJECT)))
        assert ctx.reproject_frames() == 2
        _check(tref, got, rp, tp, ("behind the reprojection stage", tp["curve"]))
        ctx.reproject_reset()


def test_accumulation(rwr, tref, ctx, ref_loader, suzanne, cube):
    """Four frames of 2 spp are one frame of 8 spp; other parameters at frame 3 restart nothing."""
    s = tc.sized(rwr, ref_loader, suzanne, cube, "room", 70, 13)
    cam_inv = ec.camera(rwr, s)
    _upload(ctx, s)
    plain8 = _frame(ctx, cam_inv, _params(rwr, s, 8))
    ctx.set_tonemap_params(**A)
    want = _frame(ctx, cam_inv, _mapped(rwr, _params(rwr, s, 8)))
    _check(tref, want, plain8, A, "one frame of 8 spp")
    for fif in (1, 2):
        ctx.set_frames_in_flight(fif)
        ctx.accum_reset()
        for k in range(1, 5):
            ctx.set_tonemap_params(**(B if k == 3 else A))
            got = _frame(ctx, cam_inv, _mapped(rwr, _params(rwr, s, 2, extra=rwr.FLAG_ACCUMULATE)))
            assert ctx.accum_samples() == 2 * k, (fif, k)
            if k == 3:
                assert got["tonemap"] == (0, 0, float(np.float32(B["exposure"])))
        _same(got, want, ("four frames of 2 spp", fif))
        assert got["tonemap"] == want["tonemap"]
        # the history never saw the stage: the next frame without the flag is the plain accumulation of 10
        ctx.render(cam_inv, _params(rwr, s, 2, extra=rwr.FLAG_ACCUMULATE))
        assert ctx.accum_samples() == 10
        ten = ctx.readback(aux=True)
        ctx.accum_reset()
        _same(ten, _frame(ctx, cam_inv, _params(rwr, s, 10)), ("the accumulation of 10 without the flag", fif))


def test_refusals_and_parameters(rwr, ctx, ref_loader, suzanne, cube):
    s = tc.sized(rwr, ref_loader, suzanne, cube, "room", 64, 40)
    cam = ec.camera(rwr, s)
    _upload(ctx, s)
    assert ctx.tonemap_params() == pytest.approx(tr.DEFAULTS)
    kept = dict(curve=tr.REINHARD, auto_exposure=1, exposure=0.5, key=0.25, white=8.0)
    ctx.set_tonemap_params(**kept)
    assert ctx.tonemap_params() == kept
    tm = rwr.FLAG_TONEMAP

    def refused(text, **kw):
        with pytest.raises(rwr.RwrError) as ei:
            ctx.render(cam, **kw)
        assert ei.value.code == rwr.ERR_UNSUPPORTED and text in ei.value.message, (kw, ei.value.message)
        assert ctx.tonemap_params() == kept

    # parts of a frame, with the stage's own message
    refused(PART_FRAME + "; rows [0,32) every 1-th strip is a part of it", params=rwr.make_params(flags=tm), rows=(0, 32))
    refused(PART_FRAME, params=rwr.make_params(flags=tm), rows=(8, 40))
    refused(PART_FRAME, params=rwr.make_params(flags=tm), strips=(0, 2))
    refused(PART_FRAME, params=rwr.make_params(flags=tm), strips=(1, 2))
    # the filter's rule comes first in the table: a call with both faults is refused in its name, as before
    refused("RWR_FLAG_DENOISE: the filter needs the whole frame", params=rwr.make_params(flags=tm | rwr.FLAG_DENOISE), rows=(0, 32))
    # the reference frame's own forms
    off = "RWR_FLAG_TONEMAP: RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes apply to the reference frame only"
    refused(off, params=rwr.make_params(flags=tm | rwr.FLAG_ORTHO_RAYS))
    refused(off, params=rwr.make_params(flags=tm | rwr.FLAG_USE_BVH))
    ctx.set_triangles(rwr.make_triangles([((0, 0, -1), (1, 0, -1), (0, 1, -1))]))
    try:
        refused(off, params=rwr.make_params(flags=tm))
    finally:
        ctx.set_triangles(rwr.make_triangles())
    # a call that covers the whole frame behaves as rwr_render
    p = rwr.make_params(spp=2, max_bounces=1, seed=4, flags=tm | rwr.FLAG_EMISSIVE)
    whole = _frame(ctx, cam, p)
    for kw in ({"rows": (0, 40)}, {"strips": (0, 1)}):
        _same(_frame(ctx, cam, p, **kw), whole, kw)
    # parameters out of range or NaN: refused, the previous ones stay
    nan, inf = float("nan"), float("inf")
    for bad in ({"curve": 3}, {"curve": 0xffffffff}, {"auto_exposure": 2}, {"exposure": 0.0}, {"exposure": -1.0}, {"exposure": nan}, {"exposure": inf},
                {"exposure": 2.0 ** -17}, {"exposure": 2.0 ** 16 + 1.0}, {"key": 0.0}, {"key": nan}, {"key": 2.0 ** -17}, {"key": 2.0 ** 17},
                {"white": 0.0}, {"white": nan}, {"white": inf}, {"white": 2.0 ** -9}, {"white": 2.0 ** 17}, {"white": -4.0}):
        with pytest.raises(rwr.RwrError) as ei:
            ctx.set_tonemap_params(**bad)
        assert ei.value.code == rwr.ERR_INVALID_ARGUMENT, bad
        assert ctx.tonemap_params() == kept, bad
    for ok in ({"exposure": 2.0 ** -16}, {"exposure": 2.0 ** 16}, {"key": 2.0 ** -16}, {"key": 2.0 ** 16}, {"white": 2.0 ** -8}, {"white": 2.0 ** 16}):
        ctx.set_tonemap_params(**ok)                             # the ranges' ends are inside
    ctx.set_tonemap_params(**kept)
    L = rwr.lib()
    buf = np.zeros(1, rwr.TONEMAP_PARAMS_DTYPE)
    assert L.rwr_tonemap_set_params(None, buf.ctypes.data_as(C.c_void_p)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_tonemap_get_params(None, buf.ctypes.data_as(C.c_void_p)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_tonemap_get_params(ctx._h, None) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_last_tonemap_stats(ctx._h, None, None, None) == rwr.ERR_INVALID_ARGUMENT
    assert ctx.tonemap_params() == kept
    # the context is still usable, and NULL restores the defaults
    _same(_frame(ctx, cam, p), whole, "after the refusals")
    ctx.set_tonemap_params()
    assert ctx.tonemap_params() == pytest.approx(tr.DEFAULTS)


def _loaded_hip_runtime():
    """The HIP runtime this process has already bound (the library's own), by its path: opening that file again loads nothing new."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime is loaded")


def test_the_device_targets_hold_the_mapped_bytes(rwr, tref, ctx, ref_loader, suzanne, cube):
    s = tc.sized(rwr, ref_loader, suzanne, cube, "room", 70, 13)
    cam_inv = ec.camera(rwr, s)
    _upload(ctx, s)
    plain = _frame(ctx, cam_inv, _params(rwr, s, 2))
    ctx.set_tonemap_params(**A)
    got = _frame(ctx, cam_inv, _mapped(rwr, _params(rwr, s, 2)))
    want = _check(tref, got, plain, A, "device targets")
    ctx.synchronize()
    d_rgba8, _ = ctx.device_targets()
    hip = _loaded_hip_runtime()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    host = np.zeros((13, 70, 4), np.uint8)
    assert hip.hipMemcpy(host.ctypes.data, d_rgba8, host.nbytes, 2) == 0   # hipMemcpyDeviceToHost
    assert host.tobytes() == want["color"].tobytes()
