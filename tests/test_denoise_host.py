"""The a-trous denoiser's CPU reference (tests/denoise_ref.c: the definition of RWR_FLAG_DENOISE, include/rwr_hip.h)
checked against the properties the definition implies, and its effect on a low-sample frame of the oracle.  No GPU."""
import numpy as np
import pytest

import denoise_ref


@pytest.fixture(scope="module")
def dref(tmp_path_factory):
    return denoise_ref.lib(tmp_path_factory)


def _planes(h, w, ids=0, t=2.0):
    return np.full((h, w), ids, np.int32), np.full((h, w), t, np.float32)


NHAT2 = np.array([[0, 0, 1], [1, 0, 0]], np.float32)   # two faces at a right angle


def test_declares_the_flag_and_the_parameter_calls(rwr):
    """The public surface: the flag's value, the defaults the reference assumes, the two entry points in the header."""
    assert rwr.FLAG_DENOISE == 1 << 8
    assert {"rwr_denoise_set_params", "rwr_denoise_get_params"} <= set(rwr.exported_symbols_declared_in_header())
    assert rwr.DENOISE_PARAMS_DTYPE.itemsize == 16
    assert denoise_ref.DEFAULTS == {"iterations": 5, "sigma_color": 0.04, "normal_cos_min": 0.95, "depth_rel": 0.05}


def test_a_constant_image_is_a_fixed_point(dref):
    """Every tap has w = 1 and the colour of the centre: sum / norm = c (h w) 25 times over / the same sum.  Exact for a colour
    whose products with the dyadic kernel weights are exact (0.5, 0.25, 0.75); within the roundings of the sums for any colour."""
    h, w = 37, 53
    ids, t = _planes(h, w)
    for colour, exact in (((0.5, 0.25, 0.75, 2.0), True), ((0.3, 0.7, 0.123, 2.0), False)):
        img = np.tile(np.array(colour, np.float32), (h, w, 1))
        for n in (1, 3, 5):
            out = denoise_ref.denoise(dref, img, ids, t, NHAT2, iterations=n)["color_f32"]
            if exact:
                assert out.tobytes() == img.tobytes(), n
            else:
                # 25 rounded products and 25 rounded additions in the sum, 25 additions in the norm, one division: below
                # 52 relative roundings of 2^-24 per iteration
                assert np.abs(out - img).max() <= n * 52 * 2.0 ** -24 * 0.7, n
                assert out[..., 3].tobytes() == img[..., 3].tobytes()


def test_background_pixels_pass_through_and_are_never_tapped(dref):
    rng = np.random.default_rng(1)
    h, w = 24, 40
    img = rng.random((h, w, 4), np.float32)
    ids, t = _planes(h, w)
    ids[:, 20:] = -1
    img[:, 20:, :3] = 100.0     # were a background pixel tapped, its neighbours would show it
    out = denoise_ref.denoise(dref, img, ids, t, NHAT2)["color_f32"]
    assert out[:, 20:].tobytes() == img[:, 20:].tobytes()
    assert out[:, :20, :3].max() < 1.0
    assert out[..., 3].tobytes() == img[..., 3].tobytes()
    all_bg = denoise_ref.denoise(dref, img, np.full((h, w), -1, np.int32), t, NHAT2)["color_f32"]
    assert all_bg.tobytes() == img.tobytes()


@pytest.mark.parametrize("kind", ["normals", "depth", "spheres", "sphere_mesh"])
def test_two_surfaces_at_a_straight_edge_keep_their_colours(dref, kind):
    """Colours constant per id, the ids apart in normal, in depth, or as analytic spheres: no tap crosses the edge, and each side is
    a constant image of dyadic colour - the output is the input exactly."""
    h, w = 30, 44
    ids, t = _planes(h, w)
    nhat = NHAT2
    if kind == "normals":
        ids[:, 22:] = 1
    elif kind == "depth":
        nhat = np.array([[0, 0, 1], [0, 0, 1]], np.float32)
        ids[:, 22:] = 1
        t[:, 22:] = 2.2           # 10 % apart, depth_rel 5 %
    elif kind == "spheres":
        ids[:, :22], ids[:, 22:] = -2, -3
    else:
        ids[:, 22:] = -2
    img = np.zeros((h, w, 4), np.float32)
    img[:, :22] = (0.5, 0.25, 0.125, 2.0)
    img[:, 22:] = (0.0625, 0.75, 0.5, 2.0)
    out = denoise_ref.denoise(dref, img, ids, t, nhat)
    assert out["color_f32"].tobytes() == img.tobytes()
    assert (out["color"][:, :22] == (128, 64, 32, 255)).all()
    # the same two faces with the same normal and depth are ONE surface: the edge blurs
    if kind in ("normals", "depth"):
        merged = denoise_ref.denoise(dref, img, ids, np.full((h, w), 2.0, np.float32), np.array([[0, 0, 1], [0, 0, 1]], np.float32))["color_f32"]
        assert not np.array_equal(merged[:, 20:24], img[:, 20:24])


def test_taps_outside_the_frame_are_skipped(dref):
    """3 x 2 pixels, five iterations: finite, and equal to the definition evaluated here over the in-frame taps alone (from step 4
    on only the centre tap is inside: those iterations change nothing)."""
    rng = np.random.default_rng(5)
    h, w = 2, 3
    img = rng.random((h, w, 4)).astype(np.float32)
    ids, t = _planes(h, w)
    out5 = denoise_ref.denoise(dref, img, ids, t, NHAT2, iterations=5, sigma_color=0.5)["color_f32"]
    out2 = denoise_ref.denoise(dref, img, ids, t, NHAT2, iterations=2, sigma_color=0.5)["color_f32"]
    assert np.isfinite(out5).all()
    f32 = np.float32
    kern = [f32(0.375), f32(0.25), f32(0.0625)]
    cur = img.copy()
    inv = f32(1.0) / (f32(0.5) * f32(0.5))
    for i in range(2):
        s, nxt = 1 << i, cur.copy()
        for y in range(h):
            for x in range(w):
                acc, norm = [f32(0), f32(0), f32(0)], f32(0)
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qx, qy = x + s * dx, y + s * dy
                        if not (0 <= qx < w and 0 <= qy < h):
                            continue
                        d = cur[y, x, :3] - cur[qy, qx, :3]
                        d2 = f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])
                        hw = f32(kern[abs(dx)] * kern[abs(dy)]) * f32(f32(1.0) / f32(f32(1.0) + f32(d2 * inv)))
                        for c in range(3):
                            acc[c] = f32(acc[c] + f32(hw * cur[qy, qx, c]))
                        norm = f32(norm + hw)
                for c in range(3):
                    nxt[y, x, c] = f32(acc[c] / norm)
        cur, inv = nxt, f32(inv * f32(4.0))
    assert out2.tobytes() == cur.tobytes()
    # steps 4, 8, 16: the centre tap alone, c = (h w c) / (h w) - two roundings (the product, the quotient) per iteration, colours < 1
    assert np.abs(out5 - out2).max() <= 3 * 2 * np.spacing(f32(1.0))


def test_face_normals_follow_the_instances(dref, orc, rwr, cube):
    n0 = denoise_ref.face_normals(dref, orc, cube)
    assert n0.shape == (len(cube["faces"]), 3)
    assert np.allclose(np.linalg.norm(n0, axis=1), 1.0, atol=1e-6)
    grid = rwr.make_instance_grid(2, 3.0).view(orc.INSTANCE_DTYPE)
    n4 = denoise_ref.face_normals(dref, orc, cube, grid)
    assert n4.shape == (4 * len(cube["faces"]), 3)
    assert np.allclose(np.linalg.norm(n4, axis=1), 1.0, atol=1e-6)


def test_effect_on_a_low_sample_frame(dref, orc, cube):
    """A 4 spp + 1 bounce cube frame of the oracle against 1 024 spp of the same scene: the mean absolute error is strictly lower
    after the filter (defaults) than before.  An ordering, not a margin; the two errors are recorded in DESIGN.md §6."""
    w, h = 64, 48
    cam = orc.camera_build_inv_uniform(orc.make_camera(eye=(1.4, 1.0, 1.9), target=(0, 0, 0), aspect=w / h, fovy=60.0))
    screen, spheres = orc.make_screen(w, h), np.zeros(0, orc.SPHERE_DTYPE)
    noisy = orc.render_path(cam, screen, orc.make_params(4, 1, seed=3), spheres, cube)
    truth = orc.render_path(cam, screen, orc.make_params(1024, 1, seed=77), spheres, cube)
    assert (noisy["obj_id"] >= 0).sum() > w * h // 8
    nhat = denoise_ref.face_normals(dref, orc, cube)
    out = denoise_ref.denoise(dref, noisy["color_f32"], noisy["obj_id"], noisy["hit_t"], nhat, **denoise_ref.DEFAULTS)
    before = float(np.abs(noisy["color_f32"][..., :3].astype(np.float64) - truth["color_f32"][..., :3]).mean())
    after = float(np.abs(out["color_f32"][..., :3].astype(np.float64) - truth["color_f32"][..., :3]).mean())
    print(f"denoise effect, cube 64x48, 4 spp + 1 bounce against 1 024 spp: mean absolute error {before:.6f} -> {after:.6f}")
    assert after < before, (before, after)
    for k in ("obj_id", "hit_t", "depth"):
        assert k in noisy
