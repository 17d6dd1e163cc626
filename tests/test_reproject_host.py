"""Temporal reprojection (RWR_FLAG_REPROJECT) on the CPU reference alone (reproject_ref.c), with c_now from the CPU path
reference: the projection lands where it should, the history grows and is capped as defined, max_history = 1 is the plain frame,
every sequence of reproject_common exercises what it is there for on its final frame, and the reprojected frame is closer to a
1 024-spp frame than the plain one."""
import numpy as np
import pytest

import denoise_ref
import glass_ref
import reproject_common as rc
import reproject_ref as rr

COLOR_TOL = 1e-4   # the project's bar (tests/test_gpu_multi_bounce.py)


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return rr.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def gref(tmp_path_factory):
    return glass_ref.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def dref(tmp_path_factory):
    return denoise_ref.lib(tmp_path_factory)


def _nhat(dref, orc, s):
    return denoise_ref.face_normals(dref, orc, s["model"], None if s["instances"] is None else s["instances"].view(orc.INSTANCE_DTYPE))


def _chain(L, gref, dref, rwr, orc, s, **params):
    return rr.chain(L, rc.cpu_frames(gref, rwr, orc, s), _nhat(dref, orc, s), s["cam_invs"], **params)


def test_header_declares_the_entry_points(rwr):
    declared = set(rwr.exported_symbols_declared_in_header())
    names = {"rwr_reproject_set_params", "rwr_reproject_get_params", "rwr_reproject_reset", "rwr_reproject_frames",
             "rwr_last_reproject_stats", "rwr_reproject_readback"}
    assert names <= declared
    assert all(hasattr(rwr.lib(), n) for n in names)
    assert rwr.FLAG_REPROJECT == 1 << 12 and rwr.REPROJECT_PARAMS_DTYPE.itemsize == 12
    assert "RWR_FLAG_REPROJECT = 1u << 12" in open(rwr.HEADER_PATH).read()


def test_a_point_on_a_centre_ray_projects_back_to_its_pixel(rwr, L):
    """P = O + t Dc of pixel (x, y) under a random camera lands on (x, y) of that camera's own frame within 1e-3 pixels: the
    definition's f32 result against the pixel, and against the same formulas in float64 on the same f32 inputs."""
    rng = np.random.default_rng(5)
    worst = worst64 = 0.0
    for _ in range(200):
        w, h = int(rng.integers(5, 200)), int(rng.integers(3, 150))
        eye = rng.uniform(-4, 4, 3)
        target = eye + rng.normal(size=3) * (1.0, 0.4, 1.0)
        cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=tuple(eye), target=tuple(target), aspect=w / h, fovy=float(rng.uniform(30, 90))))
        rec = rr.camera(L, cam_inv)
        x, y, t = int(rng.integers(0, w)), int(rng.integers(0, h)), float(rng.uniform(0.2, 30.0))
        P = rr.centre_point(L, cam_inv, w, h, x, y, t)
        got = rr.project(L, rec, P, w, h)
        assert got is not None, (eye, target)
        fx, fy, te = got
        c = {k: rec[k][0].astype(np.float64) for k in ("o", "c0", "cx", "cy", "nrm")}
        d = P.astype(np.float64) - c["o"]
        mu = (c["nrm"] @ c["c0"]) / (c["nrm"] @ d)
        r = mu * d - c["c0"]
        nn = c["nrm"] @ c["nrm"]
        fx64 = (np.cross(r, c["cy"]) @ c["nrm"] / nn + 1.0) * 0.5 * w - 0.5
        fy64 = (np.cross(c["cx"], r) @ c["nrm"] / nn + 1.0) * 0.5 * h - 0.5
        worst = max(worst, abs(fx - x), abs(fy - y))
        worst64 = max(worst64, abs(fx - fx64), abs(fy - fy64))
        assert abs(te - t) <= 1e-4 * t
    print(f"projection: worst |f - pixel| {worst:.3g} px, worst |f32 - f64| {worst64:.3g} px")
    assert worst <= 1e-3 and worst64 <= 1e-3


def test_still_history_grows_and_is_capped(rwr, orc, L, gref, dref, suzanne, cube):
    """Noise-free input (spp 1, no bounce): n' = min(k + 1, max_history) on every hit pixel whose id and t have not changed since
    frame 0, and out = c_now within the bar."""
    s = rc.sequence("still", rwr, orc, suzanne, cube)
    frames = rc.cpu_frames(gref, rwr, orc, s, spp=1, bounces=0)
    nhat = _nhat(dref, orc, s)
    for cap in (32, 4):
        ch = rr.chain(L, frames, nhat, s["cam_invs"], max_history=cap)
        steady = frames[0]["obj_id"] != -1
        for k, (f, c) in enumerate(zip(ch, frames)):
            steady &= (c["obj_id"] == frames[0]["obj_id"]) & (c["hit_t"].view(np.uint32) == frames[0]["hit_t"].view(np.uint32))
            assert steady.sum() >= 0.5 * (c["obj_id"] != -1).sum(), k
            assert np.array_equal(f["n"][steady], np.full(int(steady.sum()), min(k + 1, cap), np.float32)), (cap, k)
            assert float(np.abs(f["color_f32"] - c["color_f32"])[steady].max()) <= COLOR_TOL, (cap, k)
            assert sum(f["counts"]) == s["w"] * s["h"]


@pytest.mark.parametrize("name", ["orbit", "turn_away", "tiny"])
def test_max_history_one_is_the_plain_frame(rwr, orc, L, gref, dref, suzanne, cube, name):
    s = rc.sequence(name, rwr, orc, suzanne, cube)
    frames = rc.cpu_frames(gref, rwr, orc, s)
    for f, c in zip(_chain(L, gref, dref, rwr, orc, s, max_history=1), frames):
        assert f["color_f32"].tobytes() == c["color_f32"].tobytes()
        assert set(np.unique(f["n"])) <= {0.0, 1.0}
        assert np.array_equal(f["n"] == 0.0, c["obj_id"] == -1)


@pytest.mark.parametrize("name", rc.NAMES)
def test_sequences_are_worth_rendering(rwr, orc, L, gref, dref, suzanne, cube, name):
    """The conditions on each sequence's final frame (and the invariants of every frame)."""
    s = rc.sequence(name, rwr, orc, suzanne, cube)
    assert (s["w"], s["h"]) in ((64, 48), (80, 56), (37, 29), (5, 3)) and 1 <= s["spp"] <= 4 and s["bounces"] <= 2
    ch = _chain(L, gref, dref, rwr, orc, s)
    for k, f in enumerate(ch):
        reused, fresh, background = f["counts"]
        assert reused + fresh + background == s["w"] * s["h"]
        assert background == int((f["obj_id"] == -1).sum()) == int((f["n"] == 0.0).sum())
        assert reused == int(f["diag"]["reused"].sum()) <= int((f["diag"]["counting"] > 0).sum())
        assert f["n"].max() <= k + 1.001 and (k > 0 or reused == 0)
        assert f["color_f32"][..., 3].tobytes() == rc.cpu_frames(gref, rwr, orc, s)[k]["color_f32"][..., 3].tobytes()
    f, d = ch[-1], ch[-1]["diag"]
    reused, fresh, background = f["counts"]
    hit = reused + fresh
    print(f"{name}: final frame reused {reused} fresh {fresh} background {background}; " + ", ".join(f"{k} {int(v.sum())}" for k, v in d.items()))
    assert hit > 0
    if name in ("still", "orbit", "dolly", "instances", "far"):
        assert reused >= 0.5 * hit
    if name == "occluder":
        is_fresh = (f["obj_id"] != -1) & (d["reused"] == 0)
        assert fresh >= 0.01 * hit
        assert (is_fresh & (d["refused_depth"] > 0)).any() and (is_fresh & (d["refused_id"] > 0)).any()
        assert (f["obj_id"] == -2).any() and (f["obj_id"] >= 0).any()   # the sphere and the cube are both in view
    if name == "turn_away":
        assert d["behind"].sum() >= 1 and ch[1]["counts"][0] > 0   # the small turn reuses, the large one cannot
    if name == "orbit":
        assert int(((d["counting"] >= 1) & (d["counting"] <= 3)).sum()) >= 0.01 * hit and d["outside"].sum() >= 1
    if name == "instances":
        assert d["by_normal"].sum() >= 1 and f["obj_id"].max() >= len(cube["faces"])   # a later instance's faces are seen
    if name == "dolly":
        assert float(np.abs(ch[1]["hit_t"] - ch[0]["hit_t"])[(ch[1]["obj_id"] >= 0) & (ch[0]["obj_id"] >= 0)].max()) > 0.1   # te is not t
    if name == "spheres_only":
        assert (f["obj_id"] >= 0).sum() == 0 and (f["obj_id"] <= -2).any() and reused > 0
    if name == "all_flags":
        assert s["shadows"] and s["sky"] and s["mirror_spheres"] and s["glass_spheres"] and s["bounces"] == 2 and reused > 0


def test_what_it_buys(rwr, orc, L, gref, dref, suzanne, cube):
    """The oracle's cube at 64x48, 2 spp + 1 bounce: the mean absolute error of frame 8 against a 1 024-spp frame at the same camera,
    with and without the flag.  Measured, not promised: the assertion is only that the reprojected error is the smaller one
    (which is also the check that seed + k decorrelates the frames).  DESIGN.md §6 has the figures."""
    for name in ("still", "orbit"):
        s = rc.sequence(name, rwr, orc, suzanne, cube)
        assert (s["w"], s["h"], s["spp"], s["bounces"], len(s["cam_invs"])) == (64, 48, 2, 1, 9)
        truth = rc.cpu_frame(gref, rwr, orc, s, s["cam_invs"][8], 999, spp=1024)["color_f32"][..., :3]
        plain = rc.cpu_frames(gref, rwr, orc, s)[8]["color_f32"][..., :3]
        got = _chain(L, gref, dref, rwr, orc, s)[8]["color_f32"][..., :3]
        e_plain, e_got = float(np.abs(plain - truth).mean()), float(np.abs(got - truth).mean())
        print(f"{name}: mean absolute error of frame 8 against 1 024 spp: plain {e_plain:.6f}, reprojected {e_got:.6f}")
        assert e_got < e_plain, (name, e_got, e_plain)
