"""Glass surfaces (RWR_FLAG_GLASS), host side: the public surface, the scattering rule against float64 and one f32
operation at a time, the tests' CPU reference (glass_ref.c, built on mirror_ref.c and through it on the oracle) against mirror_ref
where both define the frame, and the conditions the GPU file's scenes must meet - asserted here, not assumed.  No GPU."""
import os
import re

import numpy as np
import pytest

import glass_common
import glass_ref
import mirror_ref
import path_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")
DEFAULT = (glass_ref.DEFAULT_ZENITH, glass_ref.DEFAULT_HORIZON)
COUNTS = ("rays", "shadow_rays", "occluded", "sky_terms")


@pytest.fixture(scope="module")
def gref(tmp_path_factory):
    return glass_ref.lib(tmp_path_factory)


def test_header_declares_and_library_exports_the_glass(rwr):
    text = open(os.path.join(ROOT, "include", "rwr_hip.h")).read()
    m = re.search(r"RWR_FLAG_GLASS\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and int(m.group(1)) == 11
    bits = [int(v) for v in re.findall(r"RWR_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", text)]
    assert bits.count(11) == 1                                  # a bit nobody else has
    assert re.search(r"RWR_API int rwr_scene_set_part_glass\(rwr_context \*ctx, uint32_t part, float ior, const float \*tint\);", text)
    assert re.search(r"RWR_API int rwr_scene_set_sphere_glass\(rwr_context \*ctx, uint32_t sphere, float ior, const float \*tint\);", text)
    assert re.search(r"RWR_API int rwr_scene_get_part_glass\(rwr_context \*ctx, uint32_t part, int \*is_glass, float \*ior, float tint\[3\]\);", text)
    assert re.search(r"RWR_API int rwr_scene_get_sphere_glass\(rwr_context \*ctx, uint32_t sphere, int \*is_glass, float \*ior, float tint\[3\]\);", text)
    assert re.search(r"RWR_API int rwr_last_glass_stats\(rwr_context \*ctx, uint64_t \*reflected, uint64_t \*transmitted, uint64_t \*tir\);", text)
    assert rwr.FLAG_GLASS == 1 << 11
    declared = rwr.exported_symbols_declared_in_header()
    lib = rwr.lib()
    for name in ("rwr_scene_set_part_glass", "rwr_scene_set_sphere_glass", "rwr_scene_get_part_glass", "rwr_scene_get_sphere_glass", "rwr_last_glass_stats"):
        assert name in declared and hasattr(lib, name), name
    for name in ("set_part_glass", "set_sphere_glass", "get_part_glass", "get_sphere_glass", "last_glass_stats"):
        assert hasattr(rwr.Context, name), name


def _uniform(L, pixel, sample, dim, seed):
    return np.float32(L.or_rng_hash(pixel, sample, dim, seed) >> 8) * np.float32(1.0 / 16777216.0)


def test_scattering_rule(gref):
    """glass_scatter against the definition written out one f32 operation at a time, and against Snell's and the reflection law
    in float64: a transmitted direction has sin(theta_t) = e sin(theta_i) and unit length within 1e-6 (a dozen f32 roundings of
    quantities <= 4, the largest index), a reflected one mirrors Dh about n_f; the side m is -n_f for a transmission alone."""
    f = np.float32
    rng = np.random.default_rng(23)
    seen = set()
    worst = 0.0
    for k in range(6000):
        n = rng.normal(size=3)
        n = (n / np.linalg.norm(n)).astype(f)
        d = (rng.normal(size=3) * rng.uniform(0.2, 3.0)).astype(f)        # any length
        eta = f((1.0, 1.33, 1.5, 2.4, 4.0)[k % 5])
        face = bool(k & 1)
        if face and float(n.astype(np.float64) @ d.astype(np.float64)) > 0:
            n = -n                                                       # a face's HitRecord normal is flipped towards the ray
        fent = bool((k >> 1) & 1)
        pixel, sample, dim, seed = k * 7, k % 5, 2 + 16 * (k % 3), 99
        got_d, got_m, ev = glass_ref.scatter(gref, n, d, face, fent, eta, pixel, sample, dim, seed)
        # the definition
        ln = np.sqrt(f(f(f(d[0] * d[0]) + f(d[1] * d[1])) + f(d[2] * d[2])))
        dh = np.array([d[0] / ln, d[1] / ln, d[2] / ln], f)
        s = f(f(f(n[0] * dh[0]) + f(n[1] * dh[1])) + f(n[2] * dh[2]))
        entering = fent if face else not (s > 0)
        nf = n if (face or entering) else -n
        c = min(f(1.0), max(f(0.0), -f(f(f(nf[0] * dh[0]) + f(nf[1] * dh[1])) + f(nf[2] * dh[2]))))
        e = f(f(1.0) / eta) if entering else eta
        kk = f(f(1.0) - f(f(e * e) * f(f(1.0) - f(c * c))))
        if kk < 0:
            a, b, m, want_ev = f(1.0), f(f(2.0) * c), nf, 2
        else:
            ct = np.sqrt(kk)
            q = f(f(f(1.0) - eta) / f(f(1.0) + eta))
            r0 = f(q * q)
            x = f(f(1.0) - (c if entering else ct))
            x2 = f(x * x)
            F = f(r0 + f(f(f(1.0) - r0) * f(f(x2 * x2) * x)))
            if _uniform(gref, pixel, sample, dim, seed) < F:
                a, b, m, want_ev = f(1.0), f(f(2.0) * c), nf, 0
            else:
                a, b, m, want_ev = e, f(f(e * c) - ct), -nf, 1
        want_d = np.array([f(f(a * dh[i]) + f(b * nf[i])) for i in range(3)], f)
        assert ev == want_ev and got_d.tobytes() == want_d.tobytes() and got_m.tobytes() == np.asarray(m, f).tobytes(), k
        seen.add((ev, bool(entering)))
        # the laws, in float64 (where the clamp of c did not act: the ray does come from n_f's side)
        D, N = dh.astype(np.float64), np.asarray(nf, np.float64)
        ci = -N @ D
        if ci <= 0:
            continue
        G = got_d.astype(np.float64)
        if ev == 1:
            sin_i, sin_t = np.sqrt(max(0.0, 1 - ci * ci)), np.linalg.norm(np.cross(N, G))
            worst = max(worst, abs(sin_t - float(e) * sin_i), abs(np.linalg.norm(G) - 1.0))
            assert G @ N < 0
        else:
            worst = max(worst, float(np.abs(G - (D + 2 * ci * N)).max()))
            assert G @ N > 0 or ci < 1e-6
    print(f"glass scattering against float64: {worst:.3g}; events seen (event, entering): {sorted(seen)}")
    assert worst <= 1e-5
    assert {(0, True), (1, True), (0, False), (1, False), (2, False)} <= seen
    # eta = 1: never a total reflection, and a transmission goes straight on
    for k in range(200):
        n = rng.normal(size=3)
        n = (n / np.linalg.norm(n)).astype(f)
        d = rng.normal(size=3)
        d = (d / np.linalg.norm(d)).astype(f)
        got_d, got_m, ev = glass_ref.scatter(gref, n, d, False, False, 1.0, k, 0, 2, 1)
        assert ev in (0, 1)
        if ev == 1:
            assert np.abs(got_d.astype(np.float64) - d.astype(np.float64)).max() <= 1e-6


CASES = (3, 17, 29, 58)   # four cases of tests/path_cases.py: with mirrors, with shadows and sky, on instances


@pytest.mark.parametrize("i", CASES)
def test_without_glass_it_is_the_mirror_reference(gref, orc, ref_loader, cube, suzanne, i):
    """glass_render_path with the case's table (mirror records alone) equals mirror_render_path byte for byte: every plane, every count."""
    c = path_cases.case(i, ref_loader, orc, cube, suzanne)
    kw = dict(instances=c["instances"], shadows=c["shadows"], sky=c["sky_colors"] if c["sky"] else None,
              mirror_parts=c["mirror_parts"] if c["mirrors"] else None, mirror_spheres=c["mirror_spheres"] if c["mirrors"] else None)
    args = (gref, orc, c["cam_inv"].view(orc.CAMERA_INV_DTYPE), orc.make_screen(c["w"], c["h"]),
            orc.make_params(c["spp"], c["bounces"], seed=c["seed"], flags=c["extra"] & path_cases.FLAG_NORMAL_MAP), c["spheres"].view(orc.SPHERE_DTYPE), c["model"])
    want = glass_ref.render_path(*args, use_mirror_ref=True, **kw)
    got = glass_ref.render_path(*args, **kw)
    for k in PLANES:
        assert got[k].tobytes() == want[k].tobytes(), (i, k)
    for k in COUNTS:
        assert got[k] == want[k], (i, k)
    assert np.array_equal(got["gen_rays"], want["gen_rays"]) and np.array_equal(got["gen_mirror"], want["gen_mirror"])
    assert got["events"] == (0, 0, 0) and got["multi"] == 0


@pytest.mark.parametrize("name", glass_common.GPU_SCENES)
def test_the_scenes_exercise_the_glass(rwr, orc, gref, ref_loader, suzanne, cube, name):
    """What tests/test_gpu_glass.py relies on: every scene that claims an event has it, Fresnel reflections and transmissions
    are each at least 1 % of the scene's glass events, the claimed total reflections and paths of two transmissions exist;
    sample-0 planes and generation 1's ray count do not depend on the glass; the frame does."""
    s = glass_common.scene(name, rwr, ref_loader, suzanne, cube)
    on = glass_common.reference(gref, rwr, orc, s, 13, 2, sky=DEFAULT, name=name)
    off = glass_common.reference(gref, rwr, orc, s, 13, 2, glass=False, sky=DEFAULT, name=name)
    refl, trans, tir = on["events"]
    total = refl + trans + tir
    print(f"glass scene {name}: reflected {refl}, transmitted {trans}, totally reflected {tir}, paths with >= 2 transmissions {on['multi']}, "
          f"rays per generation {on['gen_rays'][1:].tolist()}")
    assert total > 0 and off["events"] == (0, 0, 0)
    if "reflected" in s["claims"]:
        assert refl >= 0.01 * total, (name, on["events"])
    if "transmitted" in s["claims"]:
        assert trans >= 0.01 * total, (name, on["events"])
    if "tir" in s["claims"]:
        assert tir > 0, (name, on["events"])
    if "multi" in s["claims"]:
        assert on["multi"] > 0, name
    for k in ("depth", "obj_id", "hit_t"):
        assert on[k].tobytes() == off[k].tobytes(), (name, k)
    assert on["gen_rays"][1] == off["gen_rays"][1]
    if name != "black":
        assert not np.array_equal(on["color_f32"], off["color_f32"])
    assert s["w"] % 64 != 0 or s["h"] % 8 != 0      # no multiple of the 64 x 8 tile


def test_eta_one_and_black(rwr, orc, gref, ref_loader, suzanne, cube):
    s = glass_common.scene("eta_one", rwr, ref_loader, suzanne, cube)
    r = glass_common.reference(gref, rwr, orc, s, 13, 2, sky=DEFAULT, name="eta_one")
    assert r["events"][2] == 0 and r["events"][1] > 0
    # black glass: the event counts and the ray counts are those of clear glass of the same index (the throughput steers nothing)
    b = glass_common.scene("black", rwr, ref_loader, suzanne, cube)
    black = glass_common.reference(gref, rwr, orc, b, 13, 2, sky=DEFAULT, name="black")
    clear = glass_common.reference(gref, rwr, orc, dict(b, glass_spheres={0: (1.5, glass_common.CLEAR)}), 13, 2, sky=DEFAULT, name="black as clear")
    assert black["events"] == clear["events"] and np.array_equal(black["gen_rays"], clear["gen_rays"]) and sum(black["events"]) > 0
    assert (black["color_f32"] <= clear["color_f32"]).all() and not np.array_equal(black["color_f32"], clear["color_f32"])
