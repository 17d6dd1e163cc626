"""Progressive accumulation across frames (RWR_FLAG_ACCUMULATE).  The contract: K accumulating frames of
s1..sK samples with an unchanged key give, byte for byte on every plane, ONE frame without the flag of spp = s1 + ... + sK
and the same seed (whenever that sum is >= 2); any change of the key starts over; past the cap a frame adds nothing."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, H = 96, 56
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
COLOR_TOL = 1e-4


def _cam(rwr, eye=(0, 0, 3), w=W, h=H, target=(0.2, 0.2, -2.0)):
    return rwr.camera_build_inv_uniform(rwr.make_camera(eye=eye, target=target, aspect=w / h))


def _setup(rwr, ctx, model, w=W, h=H, spheres=None, instances=None):
    ctx.upload_model(model)
    ctx.set_instances(instances)
    ctx.set_spheres(rwr.make_spheres() if spheres is None else spheres)
    ctx.resize(w, h)


def _single(rwr, ctx, cam, spp, bounces, seed=11, flags=0, **kw):
    """One frame without the flag (it also ends any accumulation of the context)."""
    ctx.render(cam, rwr.make_params(spp=spp, max_bounces=bounces, seed=seed, flags=flags | rwr.FLAG_AUX_OUTPUTS), **kw)
    return ctx.readback(aux=True)


def _accum(rwr, ctx, cam, spp, bounces, seed=11, flags=0, **kw):
    ctx.render(cam, rwr.make_params(spp=spp, max_bounces=bounces, seed=seed, flags=flags | rwr.FLAG_AUX_OUTPUTS | rwr.FLAG_ACCUMULATE), **kw)
    return ctx.readback(aux=True)


def _same(a, b, what="", rows=None):
    for k in PLANES:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert x.tobytes() == y.tobytes(), (what, k)


@pytest.mark.parametrize("bounces", [0, 1])
@pytest.mark.parametrize("s,K", [(1, 2), (1, 8), (3, 5), (16, 4)])
def test_k_frames_equal_one_frame_of_all_samples(rwr, gpu_ctx, suzanne, s, K, bounces):
    _setup(rwr, gpu_ctx, suzanne)
    cam = _cam(rwr)
    want = _single(rwr, gpu_ctx, cam, K * s, bounces)
    assert gpu_ctx.accum_samples() == 0                    # the frame did not accumulate
    for k in range(1, K + 1):
        got = _accum(rwr, gpu_ctx, cam, s, bounces)
        assert gpu_ctx.accum_samples() == k * s
    _same(got, want, (s, K, bounces))


def test_prefixes_and_varying_spp(rwr, gpu_ctx, suzanne):
    """Per-frame spp may vary inside one accumulation (1 spp while moving, 8 once resting); every prefix of >= 2 samples is
    the frame of that many samples."""
    _setup(rwr, gpu_ctx, suzanne)
    cam = _cam(rwr)
    seq = [1, 2, 5, 8]
    want = {n: _single(rwr, gpu_ctx, cam, n, 1) for n in np.cumsum(seq)}
    total = 0
    for s in seq:
        got = _accum(rwr, gpu_ctx, cam, s, 1)
        total += s
        assert gpu_ctx.accum_samples() == total
        if total >= 2:
            _same(got, want[total], total)
    # the first accumulated frame of 1 sample is jittered: not the reference (pixel-centre) frame
    ref = _single(rwr, gpu_ctx, cam, 1, 1)
    one = _accum(rwr, gpu_ctx, cam, 1, 1)
    assert gpu_ctx.accum_samples() == 1
    assert one["color_f32"].tobytes() != ref["color_f32"].tobytes()


def _check_oracle(got, want):
    assert np.array_equal(got["obj_id"], want["obj_id"])
    assert np.array_equal(got["hit_t"].view(np.uint32), want["hit_t"].view(np.uint32))
    assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32))
    err = np.abs(got["color_f32"] - want["color_f32"]).max()
    assert err <= COLOR_TOL, f"max colour error {err}"


@pytest.mark.parametrize("scene", ["suzanne", "cube", "grid"])
def test_accumulation_matches_oracle(rwr, orc, gpu_ctx, suzanne, cube, scene):
    inst = None
    spheres = rwr.make_spheres()
    if scene == "suzanne":
        model, eye, target, seq, seed = suzanne, (2.4, 0.9, 1.0), (0.2, 0.2, -2.0), [2, 3], 11
    elif scene == "cube":
        model, eye, target, seq, seed = cube, (2.2, 1.7, 3.1), (0, 0, 0), [1, 1, 2], 1
        spheres = rwr.make_spheres([((1.6, 1.2, 1.4), 0.5)])
    else:
        model, eye, target, seq, seed = suzanne, (0, 0, 7), (0, 0, 0), [1, 3], 5
        inst = rwr.make_instance_grid(2, 3.0)
    _setup(rwr, gpu_ctx, model, spheres=spheres, instances=inst)
    cam = _cam(rwr, eye=eye, target=target)
    for s in seq:
        got = _accum(rwr, gpu_ctx, cam, s, 1, seed=seed)
    assert gpu_ctx.accum_samples() == sum(seq)
    want = orc.render_path(cam.view(orc.CAMERA_INV_DTYPE), orc.make_screen(W, H), orc.make_params(sum(seq), 1, seed=seed),
                           spheres.view(orc.SPHERE_DTYPE), model,
                           instances=None if inst is None else inst.view(orc.INSTANCE_DTYPE))
    _check_oracle(got, want)


def _key_change_cases(rwr, suzanne):
    """(name, apply the change to ctx and return (cam, seed, bounces, flags, size))."""
    base = dict(cam=_cam(rwr), seed=11, bounces=1, flags=0)
    return [
        ("camera", lambda ctx: dict(base, cam=_cam(rwr, eye=(0.1, 0, 3)))),
        ("seed", lambda ctx: dict(base, seed=12)),
        ("bounces", lambda ctx: dict(base, bounces=0)),
        ("flags", lambda ctx: dict(base, flags=rwr.FLAG_NO_CULL)),
        ("resize", lambda ctx: (ctx.resize(W + 8, H), dict(base, cam=_cam(rwr, w=W + 8)))[1]),
        ("set_spheres", lambda ctx: (ctx.set_spheres(rwr.make_spheres()), base)[1]),          # the same spheres: still a change
        ("set_instances", lambda ctx: (ctx.set_instances(None), base)[1]),
        ("upload", lambda ctx: (ctx.upload_model(suzanne), base)[1]),
        ("accum_reset", lambda ctx: (ctx.accum_reset(), base)[1]),
        ("frame_without_flag", lambda ctx: (ctx.render(base["cam"], rwr.make_params(spp=2, max_bounces=1, seed=11)), base)[1]),
    ]


@pytest.mark.parametrize("case", range(10))
def test_key_change_starts_over(rwr, gpu_ctx, suzanne, case):
    name, change = _key_change_cases(rwr, suzanne)[case]
    # what the changed configuration's first accumulated frame of 3 samples must be: a fresh context's
    with rwr.Context(0) as fresh:
        _setup(rwr, fresh, suzanne)
        cfg = change(fresh)
        want = _accum(rwr, fresh, cfg["cam"], 3, cfg["bounces"], seed=cfg["seed"], flags=cfg["flags"])
        assert fresh.accum_samples() == 3
    _setup(rwr, gpu_ctx, suzanne)
    for _ in range(2):
        _accum(rwr, gpu_ctx, _cam(rwr), 2, 1, seed=11)
    assert gpu_ctx.accum_samples() == 4
    cfg = change(gpu_ctx)
    got = _accum(rwr, gpu_ctx, cfg["cam"], 3, cfg["bounces"], seed=cfg["seed"], flags=cfg["flags"])
    assert gpu_ctx.accum_samples() == 3, name
    _same(got, want, name)
    # and an unchanged key goes on
    _accum(rwr, gpu_ctx, cfg["cam"], 2, cfg["bounces"], seed=cfg["seed"], flags=cfg["flags"])
    assert gpu_ctx.accum_samples() == 5, name


@pytest.mark.parametrize("slots", [2, 3])
def test_frames_in_flight(rwr, suzanne, slots):
    s, K = 2, 4
    with rwr.Context(0) as ctx:
        _setup(rwr, ctx, suzanne)
        cam = _cam(rwr)
        want = {k: _single(rwr, ctx, cam, k * s, 1) for k in range(1, K + 1)}
        ctx.set_frames_in_flight(slots)
        for rnd in range(2):                      # the second round reuses the slots' buffers
            ctx.accum_reset()
            for _ in range(K):                    # queued back to back, the last one read
                ctx.render(cam, rwr.make_params(spp=s, max_bounces=1, seed=11, flags=rwr.FLAG_AUX_OUTPUTS | rwr.FLAG_ACCUMULATE))
            assert ctx.accum_samples() == K * s
            _same(ctx.readback(aux=True), want[K], (slots, rnd, "queued"))
            ctx.accum_reset()
            for k in range(1, K + 1):             # read one by one
                got = _accum(rwr, ctx, cam, s, 1)
                assert ctx.accum_samples() == k * s
                _same(got, want[k], (slots, rnd, k))


@pytest.mark.parametrize("split", ["strips", "bands"])
def test_strips_and_bands_assemble_the_accumulated_frame(rwr, gpu_ctx, suzanne, split):
    s, K = 2, 3
    _setup(rwr, gpu_ctx, suzanne)
    cam = _cam(rwr)
    for _ in range(K):
        whole = _accum(rwr, gpu_ctx, cam, s, 1)
    asm = {k: np.zeros_like(v) for k, v in whole.items()}
    for rank in range(2):
        with rwr.Context(0) as ctx:
            _setup(rwr, ctx, suzanne)
            kw = dict(strips=(rank, 2)) if split == "strips" else dict(rows=((rank * H) // 2, ((rank + 1) * H) // 2))
            for _ in range(K):
                part = _accum(rwr, ctx, cam, s, 1, **kw)
            assert ctx.accum_samples() == K * s
            if split == "strips":
                rows = [y for y in range(H) if (y // 8) % 2 == rank]
            else:
                rows = list(range(*kw["rows"]))
            for k in asm:
                asm[k][rows] = part[k][rows]
    _same(asm, whole, split)


@pytest.mark.parametrize("env", [{"RWR_WF_ZSPLIT": "4"}, {"RWR_WF_WIDE_LANE": "0"}, {"RWR_WF_WIDE_LANE": "1"}, {"RWR_WF_GROUP": "3"},
                                 {"RWR_WF_OVERLAP": "3", "RWR_WF_GROUP": "2"}])
def test_schedules_give_the_same_accumulation(rwr, gpu_ctx, suzanne, monkeypatch, env):
    """A small mesh on an empty screen (the live-tile path after the first frame) with two slots: whatever the schedule,
    the same accumulated bytes."""
    seq = [5, 7, 5]
    cam = _cam(rwr, eye=(0, 0, 12), target=(0, 0, 0))
    with rwr.Context(0) as ref:
        _setup(rwr, ref, suzanne)
        want = _single(rwr, ref, cam, sum(seq), 1)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with rwr.Context(0) as ctx:
        _setup(rwr, ctx, suzanne)
        ctx.set_frames_in_flight(2)
        for s in seq:
            got = _accum(rwr, ctx, cam, s, 1)
        assert ctx.accum_samples() == sum(seq)
    _same(got, want, env)


def test_cap(rwr, suzanne, monkeypatch):
    monkeypatch.setenv("RWR_ACCUM_MAX_SAMPLES", "8")
    with rwr.Context(0) as ctx:
        _setup(rwr, ctx, suzanne)
        cam = _cam(rwr)
        want = _single(rwr, ctx, cam, 8, 1)
        _accum(rwr, ctx, cam, 4, 1)
        assert ctx.accum_samples() == 4
        second = _accum(rwr, ctx, cam, 4, 1)
        assert ctx.accum_samples() == 8
        _same(second, want, "at the cap")
        third = _accum(rwr, ctx, cam, 4, 1)       # past the cap: nothing added, the same image
        assert ctx.accum_samples() == 8
        _same(third, second, "past the cap")
        assert ctx.last_render_stats()[0] == 0    # no rays traced
        ctx.accum_reset()
        with pytest.raises(rwr.RwrError) as ei:   # a first frame of more samples than the cap
            _accum(rwr, ctx, cam, 9, 1)
        assert ei.value.code == rwr.ERR_INVALID_ARGUMENT


def test_refusals_and_stats(rwr, gpu_ctx, suzanne):
    _setup(rwr, gpu_ctx, suzanne)
    cam = _cam(rwr)
    for flag in (rwr.FLAG_ORTHO_RAYS, rwr.FLAG_USE_BVH):
        with pytest.raises(rwr.RwrError) as ei:
            gpu_ctx.render(cam, rwr.make_params(spp=1, flags=flag | rwr.FLAG_ACCUMULATE))
        assert ei.value.code == rwr.ERR_UNSUPPORTED
    gpu_ctx.set_triangles(rwr.make_triangles([((0, 0, -3), (1, 0, -3), (0, 1, -3))]))
    try:
        with pytest.raises(rwr.RwrError) as ei:
            gpu_ctx.render(cam, rwr.make_params(spp=1, flags=rwr.FLAG_ACCUMULATE))
        assert ei.value.code == rwr.ERR_UNSUPPORTED
    finally:
        gpu_ctx.set_triangles([])
    for spp in (1, 3):
        _accum(rwr, gpu_ctx, cam, spp, 1)
        assert gpu_ctx.last_render_stats()[0] == W * H * spp      # this frame's rays, not the accumulation's
    assert gpu_ctx.accum_samples() == 4


def test_cli_accumulate_matches_python_frame(rwr, gpu_ctx, suzanne, tmp_path):
    exe = os.path.abspath(os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render"))
    if not os.path.exists(exe):
        rwr.build()
    w, h = 96, 64
    out = str(tmp_path / "accum.png")
    r = subprocess.run([exe, "--res", rwr.RES_DIR, "--size", f"{w}x{h}", "--keys", "S*3", "--frames", "6", "--spp", "2", "--accumulate",
                        "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.search(r"^samples (\d+)$", r.stdout, re.M)
    assert m, r.stdout
    n = int(m.group(1))
    assert n == 2 * 7     # the last moving frame and the 6 resting ones share the camera uniform
    cam = rwr.make_camera(aspect=w / h)
    for keys in [rwr.KEY_BACKWARD] * 3 + [0] * 6:
        cam = rwr.circle_controller_update(cam, keys)
    _setup(rwr, gpu_ctx, suzanne, w=w, h=h)
    gpu_ctx.render(rwr.camera_build_inv_uniform(cam), rwr.make_params(spp=n))
    mine = str(tmp_path / "python.png")
    rwr.write_png(mine, gpu_ctx.readback()["color"], flip_vertical=True, encode_srgb=True)
    a = rwr.decode_image_rgba8(open(out, "rb").read())
    b = rwr.decode_image_rgba8(open(mine, "rb").read())
    assert a.shape == (h, w, 4) and np.array_equal(a, b)
