"""The tests' CPU reference of the light rays aimed at the sky's image (RWR_FLAG_LIGHT_SKY): sky_light_ref.c — mis_ref.c's chain with
the flag's items evaluated literally — built once per session into a pytest temporary directory with the oracle's own compiler
flags, and called like mis_ref.render_path.  sobol=True builds the same source the way sobol_ref.py builds mis_ref.c: preprocessed,
its one rng_hash renamed, the sequence and a dispatching rng_hash put in front."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np

import emission_ref
import glass_ref
import sobol_ref
import soft_shadow_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "sky_light_ref.c")
MAX_SPHERES = emission_ref.MAX_SPHERES
BLACK = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))

_libs = {}


def _declare(L):
    L.sky_light_render_path.restype = C.c_int
    L.sky_light_table.restype = C.c_double
    L.sky_light_table.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.sky_light_samples.restype = None
    L.sky_light_samples.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p]
    L.sky_image_ref_radiance.restype = None
    L.sky_image_ref_radiance.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    return L


def lib(tmp_path_factory, sobol: bool = False) -> C.CDLL:
    """Compiles sky_light_ref.c on first use (one build per session and kind) and loads it."""
    if sobol not in _libs:
        tmp = str(tmp_path_factory.mktemp("sky_light_ref_sobol" if sobol else "sky_light_ref"))
        cc, flags = glass_ref.compiler(), glass_ref.oracle_cflags()
        src = SOURCE
        if sobol:
            r = subprocess.run([cc] + flags + ["-E", "-P", SOURCE], capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("preprocessing sky_light_ref.c failed:\n" + r.stderr)
            text, n = re.subn(r"\brng_hash(\s*\(\s*uint32_t\s+pixel\s*,\s*uint32_t\s+sample\s*,\s*uint32_t\s+dim\s*,\s*uint32_t\s+seed\s*\)\s*\{)",
                              r"rng_hash_plain\1", r.stdout)
            assert n == 1, f"{n} definitions of rng_hash in the preprocessed reference, expected one"
            src = os.path.join(tmp, "sky_light_ref_generated.c")
            with open(src, "w") as f:
                f.write(sobol_ref.PRELUDE + text)
        out = os.path.join(tmp, "libsky_light_ref.so")
        cmd = [cc] + flags + ["-shared", "-o", out, src, "-lm"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("sky_light_ref.c build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        L = _declare(C.CDLL(out))
        if sobol:
            L.sobol_ref_set.restype = None
            L.sobol_ref_set.argtypes = [C.c_int]
            L.sobol_ref_set(1)
        _libs[sobol] = L
    return _libs[sobol]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def sun_map(n: int = 16, sky: float = 0.05, sun: float = 40.0) -> np.ndarray:
    """float32 (n, n, 3): `sky` everywhere, a 2 x 2 sun of `sun` in the upper hemisphere (rows 5-6, columns 9-10 at n = 16)."""
    img = np.full((n, n, 3), sky, np.float32)
    j, i = (5 * n) // 16, (9 * n) // 16
    img[j:j + 2, i:i + 2] = sun
    return img


def table(L, image):
    """(W, float32 table of n + n * n entries): item 1 on the (n, n, 3) image."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    n = img.shape[0]
    t = np.zeros(n + n * n, np.float32)
    W = float(L.sky_light_table(_p(img), n, _p(t)))
    return W, t


def samples(L, tab, n: int, u4, normal=(0.0, 1.0, 0.0), n_lights: int = 1) -> dict:
    """Items 3 and 4 for every row of u4: {"omega" (N, 3), "drawn" (N, 2) column and row of the drawn texel, "texel" (N, 2) of the texel
    omega maps back to, "P", "g", "ndw"}."""
    u = np.ascontiguousarray(u4, dtype=np.float32).reshape(-1, 4)
    nrm = np.ascontiguousarray(normal, dtype=np.float32).reshape(3)
    out = np.zeros((len(u), 12), np.float32)
    L.sky_light_samples(_p(tab), n, _p(u), len(u), _p(nrm), n_lights, _p(out))
    return {"omega": out[:, 0:3].copy(), "drawn": out[:, 3:5].astype(np.uint32), "texel": out[:, 5:7].astype(np.uint32), "P": out[:, 7].copy(),
            "g": out[:, 8].copy(), "ndw": out[:, 9].copy()}


def radiance(L, image, dirs) -> np.ndarray:
    img = np.ascontiguousarray(image, dtype=np.float32)
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    out = np.zeros_like(d)
    L.sky_image_ref_radiance(_p(img), img.shape[0], _p(d), len(d), _p(out))
    return out


class _WithSkyLight:
    """soft_shadow_ref.render_path's library argument: its call of soft_render_path becomes sky_light_render_path with the same
    arguments and `extra` behind them."""

    def __init__(self, L, extra):
        self.L, self.extra = L, extra

    def soft_render_path(self, *args):
        return self.L.sky_light_render_path(*args, *self.extra)


def render_path(L, orc, cam_inv, screen, params, spheres, model, image=None, sky_light=True, mis=True, emissive_parts=None,
                emissive_spheres=None, light=False, parts=False, **kw) -> dict:
    """sky_light_render_path with mis_ref.render_path's arguments, the (n, n, 3) image (None: the chain's frame) and the flag.  The
    result has mis_ref's entries and "sky_light": (light rays aimed at the image, reached, misses silenced or weighted),
    "sky_dropped", "sky_capped", "sky_weighted"."""
    n_mat = len(model) if isinstance(model, (list, tuple)) else 1
    bounces = int(params["max_bounces"][0])
    glow = None
    if emissive_parts is not None or emissive_spheres is not None:
        glow = np.ascontiguousarray(emission_ref.emission_table(n_mat, emissive_parts, emissive_spheres), dtype=np.float32)
    gen_glow = np.zeros(bounces + 1, np.uint64)
    glow_occluded = np.zeros(1, np.uint64)
    capped = np.zeros(2, np.uint64)
    by_surface = np.zeros(n_mat + MAX_SPHERES, np.uint64)
    light_gen = np.zeros((bounces + 1, 3), np.uint64)
    part_gen = np.zeros((bounces + 1, 3), np.uint64)
    light_capped = np.zeros(1, np.uint64)
    mis_out = np.zeros(4, np.uint64)
    sky_out = np.zeros(6, np.uint64)
    img = None if image is None else np.ascontiguousarray(image, dtype=np.float32)
    kw.setdefault("shadows", False)
    kw.setdefault("sky", BLACK)
    extra = (_p(glow), _p(gen_glow), _p(glow_occluded), _p(capped), _p(by_surface), C.c_int(1 if light else 0), _p(light_gen), None, None,
             C.c_int(1 if parts else 0), _p(part_gen), _p(light_capped), C.c_int(1 if mis else 0), _p(mis_out),
             _p(img), C.c_uint32(0 if img is None else img.shape[0]), C.c_int(1 if sky_light else 0), _p(sky_out))
    out = soft_shadow_ref.render_path(_WithSkyLight(L, extra), orc, cam_inv, screen, params, spheres, model, coverage=False, **kw)
    lg, pg = light_gen.astype(np.int64), part_gen.astype(np.int64)
    out.update(gen_glow=gen_glow.astype(np.int64), emissive_hits=int(gen_glow.sum()), glow_occluded=int(glow_occluded[0]),
               capped=(int(capped[0]), int(capped[1])), glow_by_surface=by_surface.astype(np.int64), light_gen=lg,
               light_rays=int(lg[:, 0].sum()), reached=int(lg[:, 1].sum()), suppressed=int(lg[:, 2].sum()), part_gen=pg,
               part_light=(int(pg[:, 0].sum()), int(pg[:, 1].sum()), int(pg[:, 2].sum())), light_capped=int(light_capped[0]),
               mis=tuple(int(v) for v in mis_out), sky_light=(int(sky_out[0]), int(sky_out[1]), int(sky_out[2])),
               sky_dropped=int(sky_out[3]), sky_capped=int(sky_out[4]), sky_weighted=int(sky_out[5]))
    return out
