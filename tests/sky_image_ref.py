"""The tests' CPU reference of the sky's image (RWR_FLAG_SKY_IMAGE): S_img(D) from sky_image_ref.c — the header's definition, built
once per session with the oracle's own compiler flags — and the frame reference, which is the latest path reference (mis_ref.c's
chain) under a black sky plus the image's terms.

The frame.  The flag changes no ray: a path that ends in the sky ends there under any sky, so the chain's frame under a black sky
(zenith = horizon = 0) holds every other term, and its miss records give {D, T, k} of the one sky term a sample can have.  The
image's terms are formed as the integrator forms its sums: per term f32 T * S_img(D) per channel, converted to 2^-22 fixed point
(NaN and negatives as 0), clamped to 64, summed as integers; the pixel is the black-sky pixel plus that sum / 2^22 / spp."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import mis_ref
import sky_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "sky_image_ref.c")
MISS_ARG = 34           # sky_render_path's miss_out among its arguments, and every later entry's of the chain
BLACK = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))

_lib = None


def lib(tmp_path_factory) -> C.CDLL:
    """Compiles sky_image_ref.c on first use (one build per session) and loads it."""
    global _lib
    if _lib is None:
        out = os.path.join(str(tmp_path_factory.mktemp("sky_image_ref")), "libsky_image_ref.so")
        cmd = [sky_ref.compiler()] + sky_ref.oracle_cflags() + ["-shared", "-o", out, SOURCE, "-lm"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("sky_image_ref.c build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        lib_ = C.CDLL(out)
        lib_.sky_image_ref_uv.restype = None
        lib_.sky_image_ref_uv.argtypes = [C.c_void_p, C.c_void_p]
        lib_.sky_image_ref_radiance.restype = None
        lib_.sky_image_ref_radiance.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
        _lib = lib_
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def uv(L, dirs) -> np.ndarray:
    """(u, v) of every row of dirs, float32 (N, 2)."""
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    out = np.zeros((len(d), 2), np.float32)
    for k in range(len(d)):
        L.sky_image_ref_uv(_p(d[k]), _p(out[k]))
    return out


def radiance(L, image, dirs) -> np.ndarray:
    """S_img of every row of dirs on the (n, n, 3) image, float32 (N, 3)."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    assert img.ndim == 3 and img.shape[0] == img.shape[1] and img.shape[2] == 3
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    out = np.zeros_like(d)
    L.sky_image_ref_radiance(_p(img), img.shape[0], _p(d), len(d), _p(out))
    return out


def special_directions() -> np.ndarray:
    """The six axes, the four diamond edges at D.y = +0 and at D.y = -0, and the eight diagonals."""
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    edges = [(sx, y, sz) for y in (0.0, -0.0) for sx in (1, -1) for sz in (1, -1)]
    diagonals = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    return np.array(axes + edges + diagonals, np.float32)


def direction_of_uv(u, v) -> np.ndarray:
    """The inverse mapping, in float64: the direction (not normalised: |x| + |y| + |z| = 1) whose (u, v) this is."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    px, pz = 2.0 * u - 1.0, 2.0 * v - 1.0
    y = 1.0 - np.abs(px) - np.abs(pz)
    low = y < 0
    x = np.where(low, (1.0 - np.abs(pz)) * np.copysign(1.0, px), px)
    z = np.where(low, (1.0 - np.abs(px)) * np.copysign(1.0, pz), pz)
    return np.stack([x, y, z], axis=-1)


def texel_centre_directions(n: int) -> np.ndarray:
    """float32 (n * n, 3): the direction of every texel centre, row by row."""
    c = (np.arange(n) + 0.5) / n
    vv, uu = np.meshgrid(c, c, indexing="ij")
    return direction_of_uv(uu.ravel(), vv.ravel()).astype(np.float32)


def random_directions(count: int, seed: int) -> np.ndarray:
    d = np.random.default_rng(seed).normal(size=(count, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def make_image(n: int, seed: int = 5) -> np.ndarray:
    """Random texels in [0, 4], one component at 64 (the range's end), several texels at 0."""
    rng = np.random.default_rng(seed + n)
    img = rng.uniform(0.0, 4.0, size=(n, n, 3)).astype(np.float32)
    flat = img.reshape(-1, 3)
    flat[rng.choice(n * n, size=max(1, n * n // 8), replace=False)] = 0.0
    flat[int(rng.integers(n * n)), int(rng.integers(3))] = 64.0
    return img


class _WithMisses:
    """mis_ref.render_path's library argument: its call of mis_render_path gets `miss` as miss_out."""

    def __init__(self, L, miss):
        self.L, self.miss = L, miss

    def mis_render_path(self, *args):
        assert args[MISS_ARG] is None
        return self.L.mis_render_path(*args[:MISS_ARG], _p(self.miss), *args[MISS_ARG + 1:])


def _fixed_mean(term, live, miss, spp: int) -> np.ndarray:
    """float64 (H, W, 3): the live samples' f32 terms as 2^-22 fixed point (NaN and negatives as 0), clamped to 64, summed as integers, / spp."""
    fix = np.floor((term * np.float32(2.0 ** 22)).astype(np.float32).astype(np.float64))
    fix = np.where(np.isfinite(fix) | (fix > 0), fix, 0.0)             # NaN as 0 (+inf stays, for the clamp)
    fix = np.clip(fix, 0.0, 64.0 * 2.0 ** 22).astype(np.int64)
    per_sample = np.zeros((live.size, 3), np.int64)
    per_sample[live] = fix
    h, w = miss.shape[0], miss.shape[1]
    return per_sample.reshape(h, w, spp, 3).sum(axis=2).astype(np.float64) / 2.0 ** 22 / spp


def sky_terms(L, image, miss, spp: int) -> np.ndarray:
    """float64 (H, W, 3): per pixel the mean of its samples' image terms, formed as the module's text says."""
    m = miss.reshape(-1, 8)
    live = m[:, 7] != 0
    s = radiance(L, image, m[live, 0:3])
    return _fixed_mean((m[live, 3:6] * s).astype(np.float32), live, miss, spp)


def gradient_terms(sky, miss, spp: int) -> np.ndarray:
    """The same for RWR_FLAG_SKY's gradient (zenith, horizon): S = horizon + (zenith - horizon) * clamp(0.5 D.y + 0.5, 0, 1) in f32."""
    m = miss.reshape(-1, 8)
    live = m[:, 7] != 0
    z, hz = np.asarray(sky[0], np.float32), np.asarray(sky[1], np.float32)
    u = np.clip(np.float32(0.5) * m[live, 1] + np.float32(0.5), np.float32(0.0), np.float32(1.0))[:, None]
    s = (hz + ((z - hz) * u).astype(np.float32)).astype(np.float32)
    return _fixed_mean((m[live, 3:6] * s).astype(np.float32), live, miss, spp)


def with_terms(base: dict, terms) -> dict:
    """base (render_path's result) with `terms` added to its colour planes."""
    color_f = base["black_f32"].copy()
    color_f[..., :3] = (base["black_f32"][..., :3].astype(np.float64) + terms).astype(np.float32)
    color = base["color"].copy()
    color[..., :3] = np.rint(np.clip(color_f[..., :3], 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)   # (the oracle's unorm8)
    return dict(base, color_f32=color_f, color=color)


def render_path(L, Lmis, orc, cam_inv, screen, params, spheres, model, image, gradient=None, **kw) -> dict:
    """The frame under the image: mis_ref.render_path's arguments without its light flags (the chain with mis, light and parts
    off is the path loop of every earlier flag) and the (n, n, 3) image.  The result has the chain's entries — the planes, "rays",
    "shadow_rays", "occluded", "sky_terms", ... — with "color_f32" and "color" under the image, "misses" (H, W, spp, 8),
    "black_f32" (the frame under the black sky) and, with gradient = (zenith, horizon), "gradient_f32": the colour under that
    gradient, formed from the same records."""
    w, h = int(screen["width"][0]), int(screen["height"][0])
    spp = max(1, int(params["spp"][0]))
    miss = np.zeros((h, w, spp, 8), np.float32)
    out = mis_ref.render_path(_WithMisses(Lmis, miss), orc, cam_inv, screen, params, spheres, model, light=False, parts=False, mis=False,
                              sky=BLACK, **kw)
    out.update(black_f32=out["color_f32"].copy(), misses=miss)
    if gradient is not None:
        out["gradient_f32"] = with_terms(out, gradient_terms(gradient, miss, spp))["color_f32"]
    return with_terms(out, sky_terms(L, image, miss, spp))
