"""Tone mapping and exposure (RWR_FLAG_TONEMAP), host side: the public surface, the library's shared header
(csrc/rwr_tonemap.h through tonemap_host.cpp) against the tests' reference (tonemap_ref.c) bit for bit, the reference's own
properties, and the conditions the GPU file's scenes must meet - asserted on the CPU path reference's frames, not assumed.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bvh_host
import emission_common as ec
import emission_ref
import tonemap_common as tc
import tonemap_ref as tr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32


@pytest.fixture(scope="module")
def tref(tmp_path_factory):
    return tr.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def eref(tmp_path_factory):
    return emission_ref.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The library's header, compiled without HIP the way test_sky_light_host.py compiles sky_light_host.cpp."""
    out = os.path.join(str(tmp_path_factory.mktemp("tonemap_host")), "libtonemap_host.so")
    cmd = [bvh_host.compiler(), "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-Wall", "-Wextra", "-I", bvh_host.CSRC, "-shared", "-o", out,
           os.path.join(HERE, "tonemap_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("tonemap_host.cpp build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
    lib = C.CDLL(out)
    lib.tonemap_host_luma_bits.restype, lib.tonemap_host_luma_bits.argtypes = None, [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.tonemap_host_exposure.restype, lib.tonemap_host_exposure.argtypes = C.c_float, [C.c_int64, C.c_uint32, C.c_uint32, C.c_float, C.c_float]
    lib.tonemap_host_pixels.restype = None
    lib.tonemap_host_pixels.argtypes = [C.c_void_p, C.c_uint64, C.c_float, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
    return lib


def test_header_declares_and_library_exports_the_stage(rwr):
    text = open(os.path.join(ROOT, "include", "rwr_hip.h")).read()
    m = re.search(r"RWR_FLAG_TONEMAP\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and int(m.group(1)) == 26
    bits = [int(v) for v in re.findall(r"RWR_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", text)]
    assert bits.count(26) == 1 and not set(bits) & {17, 18, 19, 20}
    public = eval(re.search(r"#define RWR_FLAGS_PUBLIC \((.*)\)\s*$", text, re.M).group(1).replace("u", ""))
    assert public & (1 << 26) and not public & (0xf << 17)
    assert re.search(r"enum \{ RWR_TONEMAP_CLAMP = 0, RWR_TONEMAP_REINHARD = 1, RWR_TONEMAP_ACES = 2 \};", text)
    assert re.search(r"RWR_API int rwr_tonemap_set_params\(rwr_context \*\w*, const rwr_tonemap_params \*\w*\);", text)
    assert re.search(r"RWR_API int rwr_tonemap_get_params\(rwr_context \*\w*, rwr_tonemap_params \*\w*\);", text)
    assert re.search(r"RWR_API int rwr_last_tonemap_stats\(rwr_context \*\w*, int64_t \*log_sum, uint32_t \*count, float \*exposure\);", text)
    assert rwr.FLAG_TONEMAP == 1 << 26
    assert (rwr.TONEMAP_CLAMP, rwr.TONEMAP_REINHARD, rwr.TONEMAP_ACES) == (0, 1, 2) == tr.CURVES
    assert rwr.TONEMAP_PARAMS_DTYPE.itemsize == 20 and rwr.TONEMAP_PARAMS_DTYPE.names == ("curve", "auto_exposure", "exposure", "key", "white")
    d = re.search(r"#define RWR_TONEMAP_DEFAULTS \{RWR_TONEMAP_ACES, 0u, 1\.0f, 0\.18f, 4\.0f\}", text)
    assert d and tr.DEFAULTS == {"curve": 2, "auto_exposure": 0, "exposure": 1.0, "key": 0.18, "white": 4.0}
    declared = rwr.exported_symbols_declared_in_header()
    lib = rwr.lib()
    for name in ("rwr_tonemap_set_params", "rwr_tonemap_get_params", "rwr_last_tonemap_stats"):
        assert name in declared and hasattr(lib, name), name
    for name in ("set_tonemap_params", "tonemap_params", "last_tonemap_stats"):
        assert hasattr(rwr.Context, name), name
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "RWR_FLAG_TONEMAP" in open(os.path.join(ROOT, doc)).read(), doc


def _edge_pixels():
    """Every triple of the edge values as r, g, b (alpha 1, and the same with alpha 0)."""
    nan = F("nan")
    e = np.array([0.0, 2.0 ** -50, 2.0 ** -16, 1.0, 4.0, 64.0 * 17.0, nan, -1.0, -2.0 ** -20, -1e6, 2.0 ** 16, 3e38], F)
    r, g, b = np.meshgrid(e, e, e, indexing="ij")
    px = np.stack([r.ravel(), g.ravel(), b.ravel(), np.ones(r.size, F)], axis=1)
    return np.ascontiguousarray(np.concatenate([px, px * np.array([1, 1, 1, 0], F)]), F)


def _random_pixels(n=100000, seed=5):
    """Log-uniform radiances over 2^-20 ... 2^11 (past both clamps of the measure), a tenth of them background."""
    rng = np.random.default_rng(seed)
    px = np.exp2(rng.uniform(-20.0, 11.0, (n, 4))).astype(F)
    px[:, 3] = 1.0
    px[rng.random(n) < 0.1] = 0.0
    return np.ascontiguousarray(px)


@pytest.mark.parametrize("pixels", ("edges", "random"))
def test_the_header_equals_the_reference(tref, host, pixels):
    px = _edge_pixels() if pixels == "edges" else _random_pixels()
    n = len(px)
    got_l = np.zeros(n, np.int32)
    host.tonemap_host_luma_bits(px.ctypes.data, n, got_l.ctypes.data)
    want_l = np.array([tref.tr_luma_bits(*map(float, p[:3])) for p in px[: 20000]], np.int32)
    assert np.array_equal(got_l[: len(want_l)], want_l)
    counted = px[:, 3] != 0
    assert tr.measure(tref, px) == (int(got_l[counted].astype(np.int64).sum()), int(counted.sum()))
    white_of = {0: 4.0, 1: 2.5, 2: 4.0}
    for curve in tr.CURVES:
        for E in (F(1.0), F(0.37), F(2.0 ** -16), F(2.0 ** 48), F(1234.5)):
            white = white_of[curve] if pixels == "random" else 4.0   # (edges: `white` is one of the inputs)
            want = tr.tonemap(tref, px, curve=curve, auto_exposure=0, exposure=float(E), white=white)
            got = np.zeros(n, np.uint32)
            host.tonemap_host_pixels(px.ctypes.data, n, float(E), curve, white, got.ctypes.data, None)
            assert want["exposure"] == E
            assert got.view(np.uint8).reshape(n, 4).tobytes() == want["color"].tobytes(), (curve, E)


def test_the_header_s_exposure_equals_the_reference_s(tref, host):
    rng = np.random.default_rng(3)
    cases = [(0, 0), (0, 5), (-1, 2), (1, 2), (-(1 << 57), 1 << 30), (1 << 57, 1 << 30), (-3 * (1 << 23), 1), (7, 7), (-7, 7), (-8, 7)]
    cases += [(int(s), int(c)) for s, c in zip(rng.integers(-(1 << 40), 1 << 40, 2000), rng.integers(1, 1 << 20, 2000))]
    for log_sum, count in cases:
        if abs(log_sum) > count << 27:
            continue   # (no frame gives it: |L| <= 2^27 per pixel)
        for auto in (0, 1):
            for key, exposure in ((0.18, 1.0), (2.0 ** -16, 2.0 ** 16), (0.25, 1.7)):
                a = host.tonemap_host_exposure(log_sum, count, auto, key, exposure)
                b = tref.tr_exposure(log_sum, count, auto, key, exposure)
                assert tr.bits(a) == tr.bits(b), (log_sum, count, auto, key, exposure)
    # count == 0 and manual mode: E = exposure, whatever the sums
    assert tref.tr_exposure(12345, 0, 1, 0.18, 3.0) == 3.0 and tref.tr_exposure(12345, 9, 0, 0.18, 3.0) == 3.0
    empty = tr.tonemap(tref, np.zeros((4, 4, 4), F), auto_exposure=1, exposure=0.75)
    assert (empty["log_sum"], empty["count"], empty["exposure"]) == (0, 0, F(0.75)) and not empty["color"].any()


def _log_normal_image(seed=11, n=4096):
    rng = np.random.default_rng(seed)
    px = np.ones((n, 4), F)
    px[:, :3] = np.exp(rng.normal(-1.0, 1.5, (n, 3))).astype(F)
    px[:: 9] = 0.0   # background
    return px


def test_constant_luminance_of_a_power_of_two_is_measured_exactly(tref):
    for k in (-16, -9, -1, 0, 1, 6, 16):
        img = np.full((7, 5, 4), 2.0 ** k, F)
        img[..., 3] = 1.0
        img[0, 0] = 0.0
        log_sum, count = tr.measure(tref, img)
        assert count == 34 and log_sum == 34 * k * (1 << 23)
        E = tref.tr_exposure(log_sum, count, 1, 0.18, 1.0)
        assert tr.bits(E) == tr.bits(F(0.18) / F(2.0 ** k))   # G = 2^k exactly


def test_scaling_by_a_power_of_two_shifts_the_measure_and_keeps_every_byte(tref):
    """Floor division's point: M moves by exactly j 2^23 on either side of zero, E by 2^-j, no byte changes."""
    img = _log_normal_image()
    inside = img.copy()
    inside[:, :3] = np.clip(inside[:, :3], 2.0 ** -8, 2.0 ** 8)   # (after scaling by 2^-7 ... 2^5 no luminance meets the measure's clamps)
    floor = lambda s, c: s // c   # noqa: E731  (Python's // is floor division)
    for curve in tr.CURVES:
        base = tr.tonemap(tref, inside, curve=curve, auto_exposure=1)
        m0 = floor(base["log_sum"], base["count"])
        signs = set()
        for j in (-7, -3, 1, 5):
            scaled = inside.copy()
            scaled[:, :3] *= F(2.0 ** j)
            out = tr.tonemap(tref, scaled, curve=curve, auto_exposure=1)
            assert out["count"] == base["count"]
            assert floor(out["log_sum"], out["count"]) == m0 + j * (1 << 23), (curve, j)
            assert out["exposure"] == base["exposure"] * F(2.0 ** -j)
            assert out["color"].tobytes() == base["color"].tobytes(), (curve, j)
            signs.add(out["log_sum"] > 0)
        assert signs == {False, True}   # the sum changed sign along the way: truncation would have broken the shift


def test_the_piecewise_linear_log_reads_a_little_low(tref):
    """What the exact integer sum costs: against the true log-average the measure is low by at most 0.086 stops."""
    img = _log_normal_image()
    hit = img[:, 3] != 0
    log_sum, count = tr.measure(tref, img)
    lum = (F(0.2126) * img[hit, 0] + F(0.7152) * img[hit, 1]) + F(0.0722) * img[hit, 2]
    true = float(np.log2(lum.astype(np.float64)).mean())
    low = true - log_sum / count / (1 << 23)
    print(f"the measure reads {low:.4f} stops low on a log-normal image")
    assert 0.0 <= low <= 0.0861


@pytest.mark.parametrize("curve", tr.CURVES)
def test_bytes_are_monotone_in_the_input(tref, curve):
    """2 000 001 inputs over [0, 64]; the f32 values themselves are not monotone in the last ulp, the bytes are."""
    n = 2000001
    for white in (4.0, 0.75):
        b = tr.curve_bytes(tref, curve, white, float(F(64.0 / (n - 1))), n).astype(np.int16)
        assert b[0] == 0 and (np.diff(b) >= 0).all(), (curve, white)
        assert b[-1] == 255


@pytest.mark.parametrize("frame", tc.FRAMES, ids=lambda f: tc.label(*f))
def test_the_gpu_file_s_scenes_hold_what_it_relies_on(rwr, orc, eref, tref, ref_loader, suzanne, cube, frame):
    name, w, h = frame
    s = tc.sized(rwr, ref_loader, suzanne, cube, name, w, h)
    for spp in ((1, 33) if w * h < 2000 else (1,)):
        r = ec.reference(eref, rwr, orc, s, 13, spp, tc.label(name, w, h))
        c = r["color_f32"]
        hit = c[..., 3] != 0                                                 # the measure's rule: a sample of the pixel hit something
        assert hit.any() and (~hit).any(), (frame, spp)                      # background and hit pixels
        assert (r["obj_id"][~hit] == -1).all() and not c[~hit].any()         # a background pixel holds zeros
        assert float(c[..., :3].max()) > 1.0, (frame, spp, float(c[..., :3].max()))   # the plain store saturates somewhere
        plain = tr.tonemap(tref, c, curve=tr.CLAMP)["color"]
        assert plain.tobytes() == r["color"].tobytes()                       # the clamp at E = 1 is the plain store
        # at least a tenth of the hit pixels get another byte under ACES than under the plain store: with the measured exposure in
        # every frame, with E = 1 in every frame but `clamped`'s, whose floor of radiance 64 is 255 under ACES at E = 1 as it is in
        # the plain store (4 of 97 hit pixels differ at 1 spp, 16 of 109 at 33) - that frame is there for the measure's range
        auto = tr.tonemap(tref, c, curve=tr.ACES, auto_exposure=1)
        assert auto["count"] == int(hit.sum()) and auto["exposure"] != 1.0
        for aces in [auto["color"]] + ([] if name == "clamped" else [tr.tonemap(tref, c, curve=tr.ACES)["color"]]):
            differ = (aces[..., :3] != plain[..., :3]).any(axis=2) & hit
            print(f"{tc.label(*frame)} spp {spp}: {int(differ.sum())} of {int(hit.sum())} hit pixels change under ACES")
            assert differ.sum() * 10 >= hit.sum(), (frame, spp, int(differ.sum()), int(hit.sum()))
            assert not aces[~hit].any()                                      # background pixels are 0 under the curve
