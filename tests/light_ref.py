"""The tests' CPU reference of light sampling (light_ref.c, which includes emission_ref.c unchanged and with it the whole stack
down to the oracle): built once per session into a pytest temporary directory with the oracle's own compiler flags, the way
emission_ref.py builds its own, and called like emission_ref.render_path."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import emission_ref
import glass_ref
import soft_shadow_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "light_ref.c")
MAX_SPHERES = emission_ref.MAX_SPHERES

_lib = None


def lib(tmp_path_factory) -> C.CDLL:
    """Compiles light_ref.c on first use (one build per session) and loads it."""
    global _lib
    if _lib is None:
        out = os.path.join(str(tmp_path_factory.mktemp("light_ref")), "liblight_ref.so")
        cmd = [glass_ref.compiler()] + glass_ref.oracle_cflags() + ["-shared", "-o", out, SOURCE, "-lm"]   # (-fopenmp is among the oracle's flags)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("light_ref.c build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        lib_ = C.CDLL(out)
        for name in ("light_render_path", "emission_render_path", "soft_render_path", "gloss_render_path"):
            getattr(lib_, name).restype = C.c_int
        _lib = lib_
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _WithLight:
    """soft_shadow_ref.render_path's library argument: its call of soft_render_path becomes light_render_path with the same
    arguments and `extra` behind them."""

    def __init__(self, L, extra):
        self.L, self.extra = L, extra

    def soft_render_path(self, *args):
        return self.L.light_render_path(*args, *self.extra)


def render_path(L, orc, cam_inv, screen, params, spheres, model, emissive_parts=None, emissive_spheres=None, light=True, entry="light",
                samples=False, **kw) -> dict:
    """light_render_path with emission_ref.render_path's arguments and the flag (light).  entry="emission": emission_render_path
    with the same arguments - what a frame the flag does nothing to must equal.  The result has emission_ref's entries and
    "light_gen" (int64[bounces + 1, 3]: per generation the light rays traced from its hits, those that reached their sphere, and the
    hits of its rays that were silenced), "light_rays", "reached", "suppressed" (their sums) and, with samples=True, "light_samples"
    (float32[h, w, spp, bounces, 4]: each light ray's direction and g, zeros where none was traced) and "light_hits"
    (float32[h, w, spp, bounces, 8]: each eligible hit's O, n and 1 / 2 / 3 - no sample from inside the sphere, no ray since n . w <= 0, a
    ray traced)."""
    if entry == "emission":
        return emission_ref.render_path(L, orc, cam_inv, screen, params, spheres, model, emissive_parts=emissive_parts,
                                        emissive_spheres=emissive_spheres, **kw)
    n_mat = len(model) if isinstance(model, (list, tuple)) else 1
    bounces = int(params["max_bounces"][0])
    spp = int(params["spp"][0])
    w, h = int(screen["width"][0]), int(screen["height"][0])
    glow = None
    if emissive_parts is not None or emissive_spheres is not None:
        glow = np.ascontiguousarray(emission_ref.emission_table(n_mat, emissive_parts, emissive_spheres), dtype=np.float32)
    gen_glow = np.zeros(bounces + 1, np.uint64)
    glow_occluded = np.zeros(1, np.uint64)
    capped = np.zeros(2, np.uint64)
    by_surface = np.zeros(n_mat + MAX_SPHERES, np.uint64)
    light_gen = np.zeros((bounces + 1, 3), np.uint64)
    sample_out = np.zeros((h, w, spp, max(bounces, 1), 4), np.float32) if samples else None
    hit_out = np.zeros((h, w, spp, max(bounces, 1), 8), np.float32) if samples else None
    kw.setdefault("shadows", False)
    extra = (_p(glow), _p(gen_glow), _p(glow_occluded), _p(capped), _p(by_surface), C.c_int(1 if light else 0), _p(light_gen), _p(sample_out), _p(hit_out))
    out = soft_shadow_ref.render_path(_WithLight(L, extra), orc, cam_inv, screen, params, spheres, model, coverage=False, **kw)
    lg = light_gen.astype(np.int64)
    out.update(gen_glow=gen_glow.astype(np.int64), emissive_hits=int(gen_glow.sum()), glow_occluded=int(glow_occluded[0]),
               capped=(int(capped[0]), int(capped[1])), glow_by_surface=by_surface.astype(np.int64), light_gen=lg,
               light_rays=int(lg[:, 0].sum()), reached=int(lg[:, 1].sum()), suppressed=int(lg[:, 2].sum()))
    if samples:
        out["light_samples"] = sample_out
        out["light_hits"] = hit_out
    return out
