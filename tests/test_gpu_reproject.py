"""Temporal reprojection (RWR_FLAG_REPROJECT) on the GPU against the tests' CPU reference (reproject_ref.c).

For every sequence of reproject_common, context A renders with the flag and context B renders each frame without it, with
seed + k and AUX; the reference chain runs over B's planes.  A's depth / id / t are B's bit for bit, the n' plane and the three
counts are the reference's exactly (they depend on geometry alone), colour is held to the project's bar.  Then: max_history = 1,
frames in flight, the filter on top, restarts, refusals and parameter errors."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref
import reproject_common as rc
import reproject_ref as rr

pytestmark = pytest.mark.gpu
COLOR_TOL = 1e-4   # the project's bar (tests/test_gpu_multi_bounce.py)
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return rr.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def dref(tmp_path_factory):
    return denoise_ref.lib(tmp_path_factory)


def _nhat(dref, orc, s):
    return denoise_ref.face_normals(dref, orc, s["model"], None if s["instances"] is None else s["instances"].view(orc.INSTANCE_DTYPE))


def _params(rwr, s, seed, flags):
    return rwr.make_params(spp=s["spp"], max_bounces=s["bounces"], seed=seed & 0xffffffff, flags=rc.gpu_flags(rwr, s) | flags)


def _tol(s):
    return COLOR_TOL * max([1.0] + [float(v) for c in (s["sky"] or ()) for v in c])


def _plain_frames(rwr, s):
    """Context B: frame k without the flag, seed + k, AUX; with that frame's render, shadow and glass stats.  Kept for the session."""
    key = ("gpu", s["name"])
    if key not in rc._cache:
        out = []
        with rwr.Context(0) as B:
            rc.upload(B, s)
            for k, cam in enumerate(s["cam_invs"]):
                B.render(cam, _params(rwr, s, rc.SEED + k, rwr.FLAG_AUX_OUTPUTS))
                f = B.readback(aux=True)
                f["stats"] = (B.last_render_stats(), B.last_shadow_stats(), B.last_glass_stats())
                out.append(f)
        rc._cache[key] = out
    return rc._cache[key]


def _compare(got, n, counts, want, plain, s, what):
    for k in ("depth", "obj_id", "hit_t"):
        assert got[k].tobytes() == plain[k].tobytes(), (what, k)
    assert counts == want["counts"] and sum(counts) == s["w"] * s["h"], (what, counts, want["counts"])
    assert n.tobytes() == want["n"].tobytes(), (what, "n'", int((n != want["n"]).sum()))
    err = float(np.abs(got["color_f32"] - want["color_f32"]).max())
    assert err <= _tol(s), (what, err)
    assert np.abs(got["color"].astype(int) - want["color"].astype(int)).max() <= 1, what
    assert got["color_f32"][..., 3].tobytes() == plain["color_f32"][..., 3].tobytes(), what
    return err


@pytest.mark.parametrize("name", rc.NAMES)
def test_sequence_parity(rwr, orc, L, dref, suzanne, cube, name):
    s = rc.sequence(name, rwr, orc, suzanne, cube)
    plains = _plain_frames(rwr, s)
    chain = rr.chain(L, plains, _nhat(dref, orc, s), s["cam_invs"])
    worst = 0.0
    with rwr.Context(0) as A:
        rc.upload(A, s)
        assert A.reproject_frames() == 0 and A.last_reproject_stats() == (0, 0, 0)
        for k, cam in enumerate(s["cam_invs"]):
            A.render(cam, _params(rwr, s, rc.SEED, rwr.FLAG_REPROJECT))   # AUX implied
            got = A.readback(aux=True)
            assert A.reproject_frames() == k + 1
            assert (A.last_render_stats(), A.last_shadow_stats(), A.last_glass_stats()) == plains[k]["stats"], (name, k)
            worst = max(worst, _compare(got, A.reproject_history(), A.last_reproject_stats(), chain[k], plains[k], s, (name, k)))
    moved = float(np.abs(chain[-1]["color_f32"] - plains[-1]["color_f32"]).max())
    print(f"reproject parity {name}: worst colour error {worst:.3g} over {len(chain)} frames; the last blend moves a pixel by up to {moved:.3g}")
    if name in ("still", "orbit", "dolly", "instances", "far"):
        assert moved > 1e-3   # the stage did something


@pytest.mark.parametrize("name", ["orbit", "all_flags", "tiny"])
def test_max_history_one_is_the_plain_frame(rwr, orc, suzanne, cube, name):
    s = rc.sequence(name, rwr, orc, suzanne, cube)
    plains = _plain_frames(rwr, s)
    with rwr.Context(0) as A:
        rc.upload(A, s)
        A.set_reproject_params(max_history=1)
        for k, cam in enumerate(s["cam_invs"]):
            A.render(cam, _params(rwr, s, rc.SEED, rwr.FLAG_REPROJECT))
            got = A.readback(aux=True)
            for p in PLANES:
                assert got[p].tobytes() == plains[k][p].tobytes(), (name, k, p)
            n = A.reproject_history()
            assert set(np.unique(n)) <= {0.0, 1.0} and np.array_equal(n == 0.0, got["obj_id"] == -1)


def test_frames_in_flight_give_the_same_bytes(rwr, orc, L, dref, suzanne, cube):
    """Frames enqueued back to back, nothing read in between: 1, 2 and 3 frames in flight give the same planes, counts and n' - and
    they are the reference's."""
    s = rc.sequence("orbit", rwr, orc, suzanne, cube)
    plains = _plain_frames(rwr, s)
    want = rr.chain(L, plains, _nhat(dref, orc, s), s["cam_invs"])[-1]
    results = []
    for fif in (1, 2, 3):
        with rwr.Context(0) as A:
            rc.upload(A, s)
            A.set_frames_in_flight(fif)
            for cam in s["cam_invs"]:
                A.render(cam, _params(rwr, s, rc.SEED, rwr.FLAG_REPROJECT))
            assert A.reproject_frames() == len(s["cam_invs"])
            results.append((A.readback(aux=True), A.reproject_history(), A.last_reproject_stats()))
    _compare(*results[0], want, plains[-1], s, "one frame in flight")
    for got, n, counts in results[1:]:
        for p in PLANES:
            assert got[p].tobytes() == results[0][0][p].tobytes(), p
        assert n.tobytes() == results[0][1].tobytes() and counts == results[0][2]


def test_the_filter_runs_behind_the_stage(rwr, orc, L, dref, suzanne, cube):
    """With RWR_FLAG_DENOISE on top the frame is the filter's reference applied to the reprojected frame, and the next frame's
    history has not seen the filter: the chain goes on over the unfiltered frames.  The bit is not part of the key: frames
    without it in between go on with the same history."""
    s = rc.sequence("orbit", rwr, orc, suzanne, cube)
    plains = _plain_frames(rwr, s)
    nhat = _nhat(dref, orc, s)
    chain = rr.chain(L, plains, nhat, s["cam_invs"])
    with rwr.Context(0) as A:
        rc.upload(A, s)
        for k, cam in enumerate(s["cam_invs"][:6]):
            filtered = k not in (2, 3)
            A.render(cam, _params(rwr, s, rc.SEED, rwr.FLAG_REPROJECT | (rwr.FLAG_DENOISE if filtered else 0)))
            got = A.readback(aux=True)
            assert A.reproject_frames() == k + 1
            want = dict(chain[k])
            if filtered:
                want.update(denoise_ref.denoise(dref, chain[k]["color_f32"], chain[k]["obj_id"], chain[k]["hit_t"], nhat))
            _compare(got, A.reproject_history(), A.last_reproject_stats(), want, plains[k], s, ("denoise", k))


def _restart_context(rwr, orc, suzanne, cube):
    s = rc.sequence("still", rwr, orc, suzanne, cube)
    A = rwr.Context(0)
    rc.upload(A, s)
    return s, A, s["cam_invs"][0]


def test_restarts(rwr, orc, suzanne, cube):
    s, A, cam = _restart_context(rwr, orc, suzanne, cube)
    rp = rwr.FLAG_REPROJECT
    base = dict(spp=2, max_bounces=1, seed=5, flags=rp)
    hits = None

    def frame(expect, **change):
        nonlocal hits
        A.render(cam, rwr.make_params(**{**base, **change}))
        assert A.reproject_frames() == expect, (expect, change)
        reused, fresh, background = A.last_reproject_stats()
        assert reused + fresh + background == s["w"] * s["h"]
        if expect == 1:   # a new history: every hit pixel is fresh
            assert reused == 0 and fresh > 0, change
            n = A.reproject_history()
            assert set(np.unique(n)) == {0.0, 1.0}
        else:
            assert reused > 0, (expect, change)

    with A:
        frame(1); frame(2); frame(3)
        restarts = {
            "resize": lambda: A.resize(s["w"], s["h"]),
            "reset": A.reproject_reset,
            "a frame without the flag": lambda: A.render(cam, rwr.make_params(spp=2, max_bounces=1, seed=5, flags=0)),
            "a mirror setter": lambda: A.set_sphere_mirror(0, (1.0, 1.0, 1.0)),
            "a mirror setter that clears": lambda: A.set_sphere_mirror(0, None),
            "set_spheres": lambda: A.set_spheres(s["spheres"]),
            "set_params with other values": lambda: A.set_reproject_params(max_history=16),
            "set_params with the same values": lambda: A.set_reproject_params(max_history=16),
            "set_params defaults": lambda: A.set_reproject_params(),
        }
        for what, act in restarts.items():
            act()
            if what == "a frame without the flag":
                assert A.reproject_frames() == 0 and A.last_reproject_stats() == (0, 0, 0)
                with pytest.raises(rwr.RwrError) as ei:
                    A.reproject_history()
                assert ei.value.code == rwr.ERR_NOT_READY
            frame(1); frame(2)
        # a change of spp, max_bounces, seed or a flag other than DENOISE: the changed frame starts over, and so does the way back
        for change in (dict(spp=3), dict(max_bounces=0), dict(seed=6), dict(flags=rp | rwr.FLAG_SHADOWS), dict(flags=rp | rwr.FLAG_NO_CULL)):
            frame(1, **change); frame(2, **change)
            frame(1); frame(2)
        # a refused setter and the DENOISE bit do not restart
        for bad in (lambda: A.set_reproject_params(max_history=0), lambda: A.set_sphere_mirror(0, (2.0, 0.0, 0.0)), lambda: A.set_sphere_mirror(99, (1.0, 1.0, 1.0))):
            with pytest.raises(rwr.RwrError):
                bad()
        frame(3)
        frame(4, flags=rp | rwr.FLAG_DENOISE)
        frame(5)
        A.set_denoise_params(iterations=2)
        frame(6, flags=rp | rwr.FLAG_DENOISE)
        A.sky_set_params((0.1, 0.2, 0.3), (1.0, 1.0, 1.0))   # the sky does not light this frame: not part of its key
        frame(7)
        frame(1, flags=rp | rwr.FLAG_SKY); frame(2, flags=rp | rwr.FLAG_SKY)
        A.sky_set_params((0.3, 0.2, 0.1), (1.0, 1.0, 1.0))   # ... and now it does
        frame(1, flags=rp | rwr.FLAG_SKY)


def test_refusals_and_parameter_errors(rwr, orc, suzanne, cube):
    s, A, cam = _restart_context(rwr, orc, suzanne, cube)
    rp, h = rwr.FLAG_REPROJECT, s["h"]
    ok = rwr.make_params(spp=2, max_bounces=1, seed=5, flags=rp)
    with A:
        A.set_reproject_params(max_history=7, normal_cos_min=0.5, depth_rel=0.125)
        kept = {"max_history": 7, "normal_cos_min": 0.5, "depth_rel": 0.125}
        assert A.reproject_params() == kept
        A.render(cam, ok); A.render(cam, ok)
        frames = 2

        def goes_on():
            nonlocal frames
            assert A.reproject_params() == kept
            A.render(cam, ok)
            frames += 1
            assert A.reproject_frames() == frames and A.last_reproject_stats()[0] > 0

        def refused(**kw):
            with pytest.raises(rwr.RwrError) as ei:
                A.render(cam, **kw)
            assert ei.value.code == rwr.ERR_UNSUPPORTED, kw
            goes_on()

        refused(params=rwr.make_params(spp=2, max_bounces=1, seed=5, flags=rp | rwr.FLAG_ACCUMULATE))
        refused(params=ok, rows=(0, 32))
        refused(params=ok, rows=(8, h))
        refused(params=ok, strips=(0, 2))
        refused(params=ok, strips=(1, 2))
        refused(params=rwr.make_params(flags=rp | rwr.FLAG_ORTHO_RAYS))
        refused(params=rwr.make_params(flags=rp | rwr.FLAG_USE_BVH))
        A.set_triangles(rwr.make_triangles([((0, 0, -1), (1, 0, -1), (0, 1, -1))]))   # (a scene attribute: accepted, so it restarts)
        with pytest.raises(rwr.RwrError) as ei:
            A.render(cam, ok)
        assert ei.value.code == rwr.ERR_UNSUPPORTED
        A.set_triangles(rwr.make_triangles())
        A.render(cam, ok)
        frames = A.reproject_frames()
        assert frames == 1
        # a call that covers the whole frame behaves as rwr_render
        for kw in ({"rows": (0, h)}, {"strips": (0, 1)}):
            A.render(cam, ok, **kw)
            frames += 1
            assert A.reproject_frames() == frames
        # parameters out of range or NaN: refused, the previous ones stay and the history goes on
        nan, inf = float("nan"), float("inf")
        for bad in ({"max_history": 0}, {"max_history": 1025}, {"normal_cos_min": nan}, {"normal_cos_min": 1.5}, {"normal_cos_min": -1.5},
                    {"normal_cos_min": inf}, {"depth_rel": -0.5}, {"depth_rel": nan}, {"depth_rel": inf}):
            with pytest.raises(rwr.RwrError) as ei:
                A.set_reproject_params(**bad)
            assert ei.value.code == rwr.ERR_INVALID_ARGUMENT, bad
            assert A.reproject_params() == kept, bad
        goes_on()
        lib = rwr.lib()
        p = np.zeros(1, rwr.REPROJECT_PARAMS_DTYPE)
        u = C.c_uint64()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        assert lib.rwr_reproject_set_params(None, vp(p)) == rwr.ERR_INVALID_ARGUMENT
        assert lib.rwr_reproject_get_params(None, vp(p)) == rwr.ERR_INVALID_ARGUMENT
        assert lib.rwr_reproject_get_params(A._h, None) == rwr.ERR_INVALID_ARGUMENT
        assert lib.rwr_reproject_reset(None) == rwr.ERR_INVALID_ARGUMENT
        assert lib.rwr_reproject_frames(A._h, None) == rwr.ERR_INVALID_ARGUMENT
        assert lib.rwr_reproject_frames(None, C.byref(u)) == rwr.ERR_INVALID_ARGUMENT
        assert lib.rwr_last_reproject_stats(A._h, C.byref(u), None, C.byref(u)) == rwr.ERR_INVALID_ARGUMENT
        assert lib.rwr_reproject_readback(A._h, None) == rwr.ERR_INVALID_ARGUMENT
        goes_on()
        A.set_reproject_params()   # NULL restores the defaults (and starts over)
        assert A.reproject_params() == pytest.approx(rr.DEFAULTS)
        A.render(cam, ok)
        assert A.reproject_frames() == 1
