"""Light rays aimed at the sky's image (RWR_FLAG_LIGHT_SKY), host side: the public surface, the library's table
builder (csrc/rwr_sky_light.h through sky_light_host.cpp) against the reference's bit for bit and by its own properties, the
sampler's density on the reference alone, the conditions the GPU file's scenes must meet - asserted here, not assumed - and the
estimator itself: unbiased, and less noisy than the plain frame under the image.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bvh_host
import sky_image_ref
import sky_light_common as sc
import sky_light_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return sky_light_ref.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def builder(tmp_path_factory):
    """The library's builder, compiled without HIP the way test_part_light_host.py compiles part_light_host.cpp."""
    out = os.path.join(str(tmp_path_factory.mktemp("sky_light_host")), "libsky_light_host.so")
    cmd = [bvh_host.compiler(), "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-Wall", "-Wextra", "-I", bvh_host.CSRC, "-shared", "-o", out,
           os.path.join(HERE, "sky_light_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("sky_light_host.cpp build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
    lib = C.CDLL(out)
    lib.sky_light_host_build.restype = C.c_double
    lib.sky_light_host_build.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    return lib


def _built(builder, img, stride=3):
    img = np.ascontiguousarray(img, np.float32)
    n = img.shape[0]
    src = img if stride == 3 else np.ascontiguousarray(np.concatenate([img, np.zeros((n, n, 1), np.float32)], axis=2))
    t = np.full(n + n * n, -1.0, np.float32)
    W = builder.sky_light_host_build(src.ctypes.data_as(C.c_void_p), n, stride, t.ctypes.data_as(C.c_void_p))
    return W, t


def _corner(n):
    img = np.zeros((n, n, 3), np.float32)
    img[0, 0] = (40.0, 30.0, 20.0)
    return img


def _black_rows(n):
    img = sky_image_ref.make_image(n, seed=9)
    img[: n // 2] = 0.0          # with the 3 x 3 neighbourhood: rows 0 ... n/2 - 2 have no weight
    img[-1] = 0.0
    return img


MAPS = {"random2": lambda: sky_image_ref.make_image(2), "random5": lambda: sky_image_ref.make_image(5), "random16": lambda: sky_image_ref.make_image(16),
        "corner5": lambda: _corner(5), "corner16": lambda: _corner(16), "rows16": lambda: _black_rows(16), "sun16": lambda: sc.SUN}


def _probabilities(t, n):
    """float64 (n, n): the f32 products P_ji of the two cdfs' f32 steps."""
    R, Cc = t[:n], t[n:].reshape(n, n)
    dr = np.diff(np.concatenate([[np.float32(0.0)], R])).astype(np.float32)
    dc = np.diff(np.concatenate([np.zeros((n, 1), np.float32), Cc], axis=1), axis=1).astype(np.float32)
    return (dr[:, None] * dc).astype(np.float32).astype(np.float64)


def test_header_declares_the_flag(rwr):
    text = open(os.path.join(ROOT, "include", "rwr_hip.h")).read()
    m = re.search(r"RWR_FLAG_LIGHT_SKY\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and int(m.group(1)) == 25
    bits = [int(v) for v in re.findall(r"RWR_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", text)]
    assert bits.count(25) == 1 and not set(bits) & {17, 18, 19, 20}
    public = re.search(r"#define RWR_FLAGS_PUBLIC \((.*)\)\s*$", text, re.M).group(1)
    assert eval(public.replace("u", "")) & (1 << 25) and not eval(public.replace("u", "")) & (0xf << 17)
    for name in ("rwr_last_sky_light_stats", "rwr_sky_get_light_info", "rwr_selftest_sky_light"):
        assert name in text and name in rwr.exported_symbols_declared_in_header(), name
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "RWR_FLAG_LIGHT_SKY" in open(os.path.join(ROOT, doc)).read(), doc
    assert rwr.FLAG_LIGHT_SKY == 1 << 25 and rwr.FLAG_SKY_IMAGE == 1 << 24


@pytest.mark.parametrize("name", sorted(MAPS))
def test_the_table(builder, sref, name):
    """The library's table equals the reference's as bits (from 3 and from 4 floats a texel); both cdfs are monotone and end at 1.0f;
    a texel has weight exactly where its 3 x 3 neighbourhood holds light; rows without weight are never drawn; sum P = 1 to a few
    ulps of the n * n rounded products."""
    img = MAPS[name]()
    n = img.shape[0]
    W, t = _built(builder, img)
    W4, t4 = _built(builder, img, stride=4)
    Wr, tr = sky_light_ref.table(sref, img)
    assert W > 0.0 and W == W4 == Wr
    assert t.tobytes() == tr.tobytes() == t4.tobytes()
    R, Cc = t[:n], t[n:].reshape(n, n)
    assert (np.diff(R) >= 0).all() and R[-1] == 1.0 and (R >= 0).all()
    assert (np.diff(Cc, axis=1) >= 0).all() and (Cc[:, -1] == 1.0).all() and (Cc >= 0).all()
    lum = img.astype(np.float64).sum(axis=2)
    pad = np.pad(lum, 1, mode="edge")
    b = sum(pad[1 + dj: 1 + dj + n, 1 + di: 1 + di + n] for dj in (-1, 0, 1) for di in (-1, 0, 1))
    P = _probabilities(t, n)
    assert ((P > 0) <= (b > 0)).all()                            # no probability without weight
    assert ((b > 0) & (P == 0)).sum() <= max(1, n * n // 64)     # (a weight too small for an f32 step may round away)
    dark_rows = np.flatnonzero(b.sum(axis=1) == 0)
    assert (Cc[dark_rows] == 1.0).all()
    if name in ("corner5", "corner16"):
        assert (P[:2, :2] > 0).all() and P[2:].sum() == 0 and P[:, 2:].sum() == 0     # the clamped neighbourhood: 2 x 2 texels see the corner
        assert b[0, 0] == 4 * 90.0 and b[0, 1] == 2 * 90.0 and b[1, 1] == 90.0      # the corner is counted 4, 2, 2 and 1 times
    if name == "rows16":
        assert len(dark_rows) == n // 2 - 1
    print(f"table {name}: W {W:.6g}, sum P - 1 = {P.sum() - 1.0:.3g}, texels with weight {int((b > 0).sum())}, with P > 0 {int((P > 0).sum())}")
    assert abs(P.sum() - 1.0) <= 4.0 * n * n * 2.0 ** -24 * P.max() + 4 * 2.0 ** -24
    u = np.random.default_rng(5).random((20000, 4)).astype(np.float32)
    u[:64, 0] = np.resize(np.concatenate([[0.0, 1.0 - 2.0 ** -24], R[R < 1.0][:14]]).astype(np.float32), 64)    # 0, the last float below 1 and the cdf's own values
    u[:64, 1] = np.resize(np.asarray([0.0, 1.0 - 2.0 ** -24], np.float32), 64)
    got = sky_light_ref.samples(sref, t, n, u)
    assert (P[got["drawn"][:, 1], got["drawn"][:, 0]] > 0).all()                     # no draw lands in a texel of probability 0
    assert not np.isin(got["drawn"][:, 1], dark_rows).any()


def test_an_all_black_map_has_no_table(builder, sref):
    img = np.zeros((5, 5, 3), np.float32)
    W, t = _built(builder, img)
    assert W == 0.0 and (t == -1.0).all()
    assert sky_light_ref.table(sref, img)[0] == 0.0


def test_the_builder_under_the_sanitizers(tmp_path):
    """The builder in a stand-alone program with its own main, under -fsanitize=address,undefined."""
    exe = str(tmp_path / "sky_light_host_asan")
    cmd = [bvh_host.compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSKY_LIGHT_HOST_MAIN",
           "-I", bvh_host.CSRC, "-o", exe, os.path.join(HERE, "sky_light_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "sky_light_host ok" in r.stdout, r.stdout + r.stderr


def test_the_density(sref):
    """10^6 draws on the sun map: 1 / (L p_l) = 1 / (p_b / g) averages to the support's solid angle, 4 pi here (every texel has
    weight), to its standard error; the texel moves in the round trip in fewer than 1 in 10^4 draws; dropped samples (P = 0 after
    the round trip) are at most 1 in 10^3."""
    n = sc.SUN.shape[0]
    W, t = sky_light_ref.table(sref, sc.SUN)
    u = np.random.default_rng(17).random((1000000, 4)).astype(np.float32)
    got = sky_light_ref.samples(sref, t, n, u, normal=(0.0, 1.0, 0.0), n_lights=1)
    moved = (got["drawn"] != got["texel"]).any(axis=1)
    dropped = ~(got["P"] > 0)
    # g = p_b / p_l with p_b = ndw / pi and L = 1: 1 / p_l = g * pi / ndw, defined for every draw (ndw cancels; take |.| of both)
    inv_pl = (got["g"].astype(np.float64) * np.pi / got["ndw"].astype(np.float64))[~dropped & (got["ndw"] != 0)]
    mean, se = inv_pl.mean(), inv_pl.std(ddof=1) / np.sqrt(len(inv_pl))
    print(f"density: mean 1/p_l {mean:.6f} (4 pi = {4 * np.pi:.6f}), standard error {se:.3g}, ratio {abs(mean - 4 * np.pi) / se:.2f}; "
          f"texel moved in {int(moved.sum())} of 10^6, dropped {int(dropped.sum())}; share of draws in the sun {np.mean(got['P'] > 0.01):.3f}")
    assert abs(mean - 4.0 * np.pi) < 4.0 * se
    assert moved.sum() < 100 and dropped.sum() <= 1000
    assert np.allclose(np.linalg.norm(got["omega"].astype(np.float64), axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("name", sc.SCENES + ("sunlit", "bare_lamp_sun", "bare_panel_sun"))
def test_each_scene_shows_what_its_gpu_test_relies_on(rwr, orc, sref, ref_loader, suzanne, cube, name):
    """On the reference alone: sky rays are traced, some reach and some are occluded, marked misses are suppressed; without the flag
    the loop is the frame under the image (sky_image_ref's) with no sky light count."""
    s = sc.scene(name, rwr, ref_loader, suzanne, cube, orc)
    for mis in (True, False):
        f = sc.reference(sref, rwr, orc, s, 13, name, mis=mis)
        rays, reached, quiet = f["sky_light"]
        print(f"{name} mis={mis}: sky light rays {rays}, reached {reached}, suppressed misses {quiet}, dropped {f['sky_dropped']}, capped {f['sky_capped']}, "
              f"totals {f['light_rays']}/{f['reached']}/{f['suppressed']}")
        assert 0 < reached <= rays and quiet > 0
        if not name.startswith("cube_b"):     # (a convex cube alone occludes none of the rays that leave its faces)
            assert reached < rays
        assert f["light_rays"] >= rays and f["reached"] >= reached and f["suppressed"] >= quiet
        assert f["sky_dropped"] * 1000 <= rays
        if mis:
            assert f["sky_capped"] == 0 and f["sky_weighted"] > 0
    off = sc.reference(sref, rwr, orc, s, 13, name, sky_light=False)
    assert off["sky_light"] == (0, 0, 0) and off["sky_terms"] > 0
    on = sc.reference(sref, rwr, orc, s, 13, name)
    for k in ("depth", "obj_id", "hit_t"):
        assert on[k].tobytes() == off[k].tobytes(), k
    assert on["rays"] == off["rays"] and on["sky_terms"] == off["sky_terms"]            # no ray of the path changes
    if name == "lamp_panel_sun":
        assert on["part_light"][0] > 0 and on["light_rays"] > on["part_light"][0] + on["sky_light"][0]   # all three kinds of lane


def test_without_an_image_it_is_mis_refs_frame(rwr, orc, sref, ref_loader, suzanne, cube, tmp_path_factory):
    """sky_light_render_path without an image is mis_render_path: planes and counts."""
    import mis_ref
    mref = mis_ref.lib(tmp_path_factory)
    s = sc.scene("lamp_panel_sun", rwr, ref_loader, suzanne, cube, orc)
    got = sc.reference(sref, rwr, orc, s, 13, "lamp_panel_sun", image=None)
    want = mis_ref.render_path(mref, orc, sc.camera(rwr, s).view(orc.CAMERA_INV_DTYPE), orc.make_screen(s["w"], s["h"]),
                               orc.make_params(s["spp"], s["bounces"], seed=13), s["spheres"].view(orc.SPHERE_DTYPE), s["model"],
                               emissive_parts=s["emissive_parts"], emissive_spheres=s["emissive_spheres"], light=True, parts=True, mis=True,
                               sky=sky_light_ref.BLACK)
    for k in PLANES:
        assert got[k].tobytes() == want[k].tobytes(), k
    for k in ("rays", "light_rays", "reached", "suppressed", "part_light", "mis", "emissive_hits"):
        assert got[k] == want[k], k


def _mean(frames):
    return np.asarray([f["color_f32"][..., :3].reshape(-1, 3).mean(axis=0, dtype=np.float64) for f in frames])


def test_the_estimator_is_unbiased(rwr, orc, sref, ref_loader, suzanne, cube):
    """Scene `sunlit`: the frame mean per channel over 8 seeds with the flag and RWR_FLAG_LIGHT_MIS against 8 seeds of plain
    RWR_FLAG_SKY_IMAGE frames (disjoint seeds): the means differ by less than 4 standard errors of their difference, estimated from
    the 16 frames themselves - test_mis_host.py's bar.  First: the reference counts no capped light term."""
    s = sc.scene("sunlit", rwr, ref_loader, suzanne, cube, orc)
    spp = 48
    frames = [sc.reference(sref, rwr, orc, s, 100 + k, "sunlit", spp=spp) for k in range(8)]
    assert sum(f["light_capped"] + f["sky_capped"] for f in frames) == 0 and all(f["sky_light"][1] > 0 and f["sky_weighted"] > 0 for f in frames)
    on = _mean(frames)
    off = _mean([sc.reference(sref, rwr, orc, s, 200 + k, "sunlit", spp=spp, sky_light=False, mis=False) for k in range(8)])
    diff = on.mean(axis=0) - off.mean(axis=0)
    se = np.sqrt(on.var(axis=0, ddof=1) / 8.0 + off.var(axis=0, ddof=1) / 8.0)
    print(f"unbiased sunlit: mean with {on.mean(axis=0)}, plain {off.mean(axis=0)}, difference {diff}, standard error {se}, ratio {np.abs(diff) / se}")
    assert (se > 0.0).all() and (np.abs(diff) < 4.0 * se).all(), (diff, se)


def test_less_noisy_than_the_plain_frame(rwr, orc, sref, ref_loader, suzanne, cube):
    """`sunlit` at 4 spp against a 2 048-spp plain frame, over the pixels that show the mesh: the MSE with the flag and
    RWR_FLAG_LIGHT_MIS is below the plain frame's.  The direction alone is asserted; the figures are printed."""
    s = sc.scene("sunlit", rwr, ref_loader, suzanne, cube, orc)
    truth = sc.reference(sref, rwr, orc, s, 7, "sunlit", spp=2048, sky_light=False, mis=False)
    mesh = truth["obj_id"] >= 0
    assert mesh.sum() > 500

    def mse(f):
        return float(((f["color_f32"][mesh][:, :3].astype(np.float64) - truth["color_f32"][mesh][:, :3].astype(np.float64)) ** 2).mean())

    a = mse(sc.reference(sref, rwr, orc, s, 31, "sunlit", spp=4))
    b = mse(sc.reference(sref, rwr, orc, s, 31, "sunlit", spp=4, mis=False))
    c = mse(sc.reference(sref, rwr, orc, s, 31, "sunlit", spp=4, sky_light=False, mis=False))
    print(f"less noise sunlit: MSE at 4 spp with the flag and MIS {a:.5g}, the flag alone {b:.5g}, plain {c:.5g}; ratio to the plain frame {a / c:.4f}, the flag alone {b / c:.4f}")
    assert a < c
