"""The tests' CPU reference of emissive surfaces (emission_ref.c, which includes soft_shadow_ref.c unchanged and with it the whole
stack down to the oracle): built once per session into a pytest temporary directory with the oracle's own compiler flags, the way
soft_shadow_ref.py builds its own, and called like soft_shadow_ref.render_path."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import glass_ref
import gloss_ref
import soft_shadow_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "emission_ref.c")
MAX_SPHERES = gloss_ref.MAX_SPHERES

_lib = None


def lib(tmp_path_factory) -> C.CDLL:
    """Compiles emission_ref.c on first use (one build per session) and loads it."""
    global _lib
    if _lib is None:
        out = os.path.join(str(tmp_path_factory.mktemp("emission_ref")), "libemission_ref.so")
        cmd = [glass_ref.compiler()] + glass_ref.oracle_cflags() + ["-shared", "-o", out, SOURCE, "-lm"]   # (-fopenmp is among the oracle's flags)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("emission_ref.c build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        lib_ = C.CDLL(out)
        lib_.emission_render_path.restype = C.c_int
        lib_.soft_render_path.restype = C.c_int
        lib_.gloss_render_path.restype = C.c_int
        _lib = lib_
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def emission_table(n_parts, emissive_parts=None, emissive_spheres=None) -> np.ndarray:
    """The table emission_render_path reads: {r, g, b, 0} per part, then per sphere index."""
    t = np.zeros((n_parts + MAX_SPHERES, 4), np.float32)
    for k, le in (emissive_parts or {}).items():
        t[k, :3] = le
    for k, le in (emissive_spheres or {}).items():
        t[n_parts + k, :3] = le
    return t


class _WithTable:
    """soft_shadow_ref.render_path's library argument: its call of soft_render_path becomes emission_render_path with the same
    arguments and `extra` behind them."""

    def __init__(self, L, extra):
        self.L, self.extra = L, extra

    def soft_render_path(self, *args):
        return self.L.emission_render_path(*args, *self.extra)


def render_path(L, orc, cam_inv, screen, params, spheres, model, emissive_parts=None, emissive_spheres=None, table=None, entry="emission", **kw) -> dict:
    """emission_render_path with soft_shadow_ref.render_path's arguments (shadows defaults to False here) and the emitters
    ({index: (r, g, b)}; table: the emission table itself, in their place; all None: no table at all).  entry="soft":
    soft_render_path with the same arguments (and no table) - what a frame without an emitter must equal.  The result has
    soft_shadow_ref's entries (the coverage measure is not taken) and "gen_glow" (emitting hits per generation, 0 = h0),
    "emissive_hits" (their sum), "glow_occluded", "capped" ((at h0, at k >= 1)) and "glow_by_surface" (emitting hits per table record)."""
    n_mat = len(model) if isinstance(model, (list, tuple)) else 1
    bounces = int(params["max_bounces"][0])
    glow = table
    if glow is None and (emissive_parts is not None or emissive_spheres is not None):
        glow = emission_table(n_mat, emissive_parts, emissive_spheres)
    if glow is not None:
        glow = np.ascontiguousarray(glow, dtype=np.float32)
        assert glow.shape == (n_mat + MAX_SPHERES, 4)
    gen_glow = np.zeros(bounces + 1, np.uint64)
    glow_occluded = np.zeros(1, np.uint64)
    capped = np.zeros(2, np.uint64)
    by_surface = np.zeros(n_mat + MAX_SPHERES, np.uint64)
    kw.setdefault("shadows", False)
    if entry == "soft":
        assert glow is None
        return soft_shadow_ref.render_path(L, orc, cam_inv, screen, params, spheres, model, coverage=False, **kw)
    out = soft_shadow_ref.render_path(_WithTable(L, (_p(glow), _p(gen_glow), _p(glow_occluded), _p(capped), _p(by_surface))), orc, cam_inv, screen,
                                      params, spheres, model, coverage=False, **kw)
    out.update(gen_glow=gen_glow.astype(np.int64), emissive_hits=int(gen_glow.sum()), glow_occluded=int(glow_occluded[0]),
               capped=(int(capped[0]), int(capped[1])), glow_by_surface=by_surface.astype(np.int64))
    return out
