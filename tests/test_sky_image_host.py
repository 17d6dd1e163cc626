"""Sky light from an image (RWR_FLAG_SKY_IMAGE) without a GPU: what the header declares, the mapping's range and its
fixed points, and rwr_sky_image_from_equirect against the pictures it is given — through the tests' own S_img (sky_image_ref.c)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sky_image_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def iref(tmp_path_factory):
    return sky_image_ref.lib(tmp_path_factory)


def test_header_and_documents_declare_the_flag(rwr):
    text = open(rwr.HEADER_PATH).read()
    assert re.search(r"RWR_FLAG_SKY_IMAGE\s*=\s*1u\s*<<\s*24\b", text)
    assert rwr.FLAG_SKY_IMAGE == 1 << 24
    public = re.search(r"^#define RWR_FLAGS_PUBLIC (.*)$", text, re.M).group(1)
    assert eval(public.replace("u", "")) & (1 << 24)
    declared = rwr.exported_symbols_declared_in_header()
    for name in ("rwr_sky_set_image", "rwr_sky_get_image_info", "rwr_sky_image_from_equirect", "rwr_selftest_sky_image"):
        assert name in declared and hasattr(rwr.lib(), name), name
    assert re.search(r"#define RWR_SKY_IMAGE_SIZE_MAX 2048u\b", text) and re.search(r"#define RWR_SKY_IMAGE_COMPONENT_MAX 64\.0f\b", text)
    assert (rwr.SKY_IMAGE_SIZE_MAX, rwr.SKY_IMAGE_COMPONENT_MAX) == (2048, 64.0)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "RWR_FLAG_SKY_IMAGE" in open(os.path.join(ROOT, doc)).read(), doc


def test_every_direction_lands_in_the_unit_square(iref):
    dirs = np.concatenate([sky_image_ref.special_directions(), sky_image_ref.random_directions(20000, 1),
                           sky_image_ref.random_directions(2000, 2) * np.float32(1e-20), sky_image_ref.random_directions(2000, 3) * np.float32(1e18)])
    uv = sky_image_ref.uv(iref, dirs)
    assert np.isfinite(uv).all() and (uv >= 0.0).all() and (uv <= 1.0).all()
    # the zenith is the centre, the nadir a corner, the horizon's axes the diamond's corners
    sp = sky_image_ref.uv(iref, [(0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1)])
    assert sp[0].tolist() == [0.5, 0.5] and set(sp[1].tolist()) <= {0.0, 1.0}
    assert sp[2:].tolist() == [[1.0, 0.5], [0.0, 0.5], [0.5, 1.0], [0.5, 0.0]]
    # upper hemisphere inside the diamond, lower outside
    d = sky_image_ref.random_directions(5000, 4)
    uv = sky_image_ref.uv(iref, d).astype(np.float64)
    r = np.abs(2 * uv[:, 0] - 1) + np.abs(2 * uv[:, 1] - 1)
    assert (r[d[:, 1] > 1e-3] < 1.0).all() and (r[d[:, 1] < -1e-3] > 1.0).all()


@pytest.mark.parametrize("n", [2, 5, 8])
def test_texel_centres_map_back_onto_themselves(iref, n):
    """S_img at a texel centre's direction is that texel, exactly: the fractions are 0 or the weights pick one texel."""
    img = sky_image_ref.make_image(n)
    dirs = sky_image_ref.texel_centre_directions(n)
    uv = sky_image_ref.uv(iref, dirs).astype(np.float64)
    c = (np.arange(n) + 0.5) / n
    vv, uu = np.meshgrid(c, c, indexing="ij")
    err = max(np.abs(uv[:, 0] - uu.ravel()).max(), np.abs(uv[:, 1] - vv.ravel()).max())
    print(f"texel centres n = {n}: (u, v) error {err:.3g}")
    if n == 8:                      # centres are dyadic: every step is exact
        assert err == 0.0
        assert np.array_equal(sky_image_ref.radiance(iref, img, dirs), img.reshape(-1, 3))
    else:                           # (2 i + 1) / (2 n) is rounded: within an ulp of 1
        assert err <= 2.0 ** -23


def test_constant_picture_gives_a_constant_map(rwr, iref):
    src = np.full((8, 16, 3), 2.5, np.float32)
    dirs = sky_image_ref.random_directions(20000, 7)
    for n in (2, 16, 64):
        img = rwr.sky_image_from_equirect(src, n)
        assert img.shape == (n, n, 3) and img.dtype == np.float32
        err = float(np.abs(sky_image_ref.radiance(iref, img, dirs) - 2.5).max())
        print(f"constant picture n = {n}: {err:.3g}")
        assert err <= 1e-6 * 2.5
    assert np.array_equal(rwr.sky_image_from_equirect(src, 4, scale=2.0), np.full((4, 4, 3), 5.0, np.float32))
    assert np.array_equal(rwr.sky_image_from_equirect(src, 4, scale=100.0), np.full((4, 4, 3), 64.0, np.float32))      # clamped
    assert np.array_equal(rwr.sky_image_from_equirect(-src, 4), np.zeros((4, 4, 3), np.float32))


def _equirect(f, w, h):
    """f(D) at the pixel centres of a w x h latitude-longitude picture: row 0 straight up, the centre column (0, 0, -1), +x to the right."""
    theta = (np.arange(h) + 0.5) / h * np.pi
    phi = ((np.arange(w) + 0.5) / w - 0.5) * 2.0 * np.pi
    t, p = np.meshgrid(theta, phi, indexing="ij")
    d = np.stack([np.sin(t) * np.sin(p), np.cos(t), -np.sin(t) * np.cos(p)], axis=-1)
    return f(d).astype(np.float32)


def test_smooth_picture_survives_the_conversion(rwr, iref):
    f = lambda d: 0.5 + 0.5 * d
    dirs = sky_image_ref.random_directions(20000, 7)
    want = f(dirs.astype(np.float64))
    err = {}
    for (w, h), n in (((256, 128), 64), ((512, 256), 128)):
        img = rwr.sky_image_from_equirect(_equirect(f, w, h), n)
        err[n] = float(np.abs(sky_image_ref.radiance(iref, img, dirs) - want).max())
        print(f"smooth picture {w} x {h} -> n = {n}: {err[n]:.4g}")
    assert err[64] <= 0.02
    assert err[128] <= 0.01 and err[128] < err[64]               # the bar shrinks with n: half the texel, half the bar
    # the orientation: a picture bright towards +x only lights the map's u = 1 side, one bright straight up its centre
    img = rwr.sky_image_from_equirect(_equirect(lambda d: np.repeat(np.maximum(d[..., 0:1], 0.0), 3, axis=-1), 64, 32), 16)
    assert img[8, 15].max() > 0.5 and img[8, 0].max() < 0.05
    img = rwr.sky_image_from_equirect(_equirect(lambda d: np.repeat(np.maximum(d[..., 1:2], 0.0) ** 8, 3, axis=-1), 64, 32), 16)
    assert img[7:9, 7:9].min() > 0.7 and img[0, 0].max() < 0.01 and img[15, 15].max() < 0.01
    img = rwr.sky_image_from_equirect(_equirect(lambda d: np.repeat(np.maximum(-d[..., 2:3], 0.0), 3, axis=-1), 64, 32), 16)
    assert img[0, 8].max() > 0.5 and img[15, 8].max() < 0.05     # -z is v = 0


def test_conversion_refusals(rwr):
    L = rwr.lib()
    src = np.ones((4, 8, 3), np.float32)
    out = np.zeros(64, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.rwr_sky_image_from_equirect(p(src), 8, 4, C.c_float(1.0), 4, p(out)) == rwr.OK
    for n in (0, 1, 2049, 1 << 20):
        assert L.rwr_sky_image_from_equirect(p(src), 8, 4, C.c_float(1.0), n, p(out)) == rwr.ERR_INVALID_ARGUMENT, n
    for w, h in ((0, 4), (8, 0), (1 << 20, 1 << 20)):
        assert L.rwr_sky_image_from_equirect(p(src), w, h, C.c_float(1.0), 4, p(out)) == rwr.ERR_INVALID_ARGUMENT, (w, h)
    for scale in (np.nan, -1.0, np.inf):
        assert L.rwr_sky_image_from_equirect(p(src), 8, 4, C.c_float(scale), 4, p(out)) == rwr.ERR_INVALID_ARGUMENT, scale
    assert L.rwr_sky_image_from_equirect(None, 8, 4, C.c_float(1.0), 4, p(out)) == rwr.ERR_INVALID_ARGUMENT
    assert L.rwr_sky_image_from_equirect(p(src), 8, 4, C.c_float(1.0), 4, None) == rwr.ERR_INVALID_ARGUMENT
    for bad in (np.nan, np.inf, -np.inf):
        s = src.copy()
        s[2, 5, 1] = bad
        with pytest.raises(rwr.RwrError) as ei:
            rwr.sky_image_from_equirect(s, 4)
        assert ei.value.code == rwr.ERR_INVALID_ARGUMENT and "[" + str((2 * 8 + 5) * 3 + 1) + "]" in ei.value.message
    assert L.rwr_sky_image_from_equirect(p(np.ones((1, 1, 3), np.float32)), 1, 1, C.c_float(1.0), 2, p(out)) == rwr.OK
    assert np.array_equal(out.reshape(-1)[:12], np.ones(12, np.float32))


def test_frame_reference_reproduces_the_chains_gradient_frame(rwr, orc, ref_loader, cube, iref, tmp_path_factory):
    """The frame reference is the chain's frame under a black sky plus terms formed from its miss records.  Formed for the
    gradient, that construction gives the chain's own frame under the gradient: the two differ by the terms' conversion to 2^-22
    fixed point (at most 2^-22 a term, so 2^-22 a pixel) and the f32 rounding of the sums (a few ulp of a colour below 16)."""
    import mis_ref
    import shadow_common
    mref = mis_ref.lib(tmp_path_factory)
    rng = np.random.default_rng(11)
    tris = rng.uniform(-1.2, 1.2, size=(60, 1, 3)) + rng.normal(scale=0.45, size=(60, 3, 3))
    model = shadow_common.triangle_model(ref_loader, [tuple(map(tuple, t)) for t in tris.astype(np.float32)], cube["texture"])
    spheres = rwr.make_spheres([((0.9, 0.4, 0.6), 0.5), ((-0.8, -0.5, 0.2), 0.35)])
    w, h, spp, bounces = 37, 29, 5, 3
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0.3, 0.5, 2.2), target=(0, 0, 0), aspect=w / h))
    sky = ((0.25, 2.0, 0.0), (3.5, 0.5, 0.125))
    args = (orc, cam_inv.view(orc.CAMERA_INV_DTYPE), orc.make_screen(w, h), orc.make_params(spp, bounces, seed=13), spheres.view(orc.SPHERE_DTYPE), model)
    for shadows in (False, True):
        kw = dict(shadows=shadows, mirror_spheres={0: (1.0, 1.0, 1.0)})
        chain = mis_ref.render_path(mref, *args, light=False, parts=False, mis=False, sky=sky, **kw)
        ours = sky_image_ref.render_path(iref, mref, *args, sky_image_ref.make_image(8), gradient=sky, **kw)
        assert ours["sky_terms"] == chain["sky_terms"] > 0 and ours["rays"] == chain["rays"] and (ours["misses"][..., 6] >= 2).any()
        for k in ("obj_id", "hit_t", "depth"):
            assert np.array_equal(ours[k], chain[k]), k
        err = float(np.abs(ours["gradient_f32"] - chain["color_f32"]).max())
        print(f"construction against the chain, shadows={shadows}: {err:.3g}")
        assert err <= 2.0 ** -22 + 8 * 2.0 ** -20       # (8 ulp at 16)
        assert not np.array_equal(ours["color_f32"], ours["gradient_f32"])
