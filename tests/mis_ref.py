"""The tests' CPU reference of multiple importance sampling for the light rays (mis_ref.c, which includes part_light_ref.c unchanged
and with it the whole stack down to the oracle): built once per session into a pytest temporary directory with the oracle's own
compiler flags, the way part_light_ref.py builds its own, and called like part_light_ref.render_path."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import emission_ref
import glass_ref
import part_light_ref
import soft_shadow_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "mis_ref.c")
MAX_SPHERES = emission_ref.MAX_SPHERES

_lib = None


def lib(tmp_path_factory) -> C.CDLL:
    """Compiles mis_ref.c on first use (one build per session) and loads it."""
    global _lib
    if _lib is None:
        out = os.path.join(str(tmp_path_factory.mktemp("mis_ref")), "libmis_ref.so")
        cmd = [glass_ref.compiler()] + glass_ref.oracle_cflags() + ["-shared", "-o", out, SOURCE, "-lm"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("mis_ref.c build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        lib_ = C.CDLL(out)
        for name in ("mis_render_path", "part_light_render_path", "part_light_table", "light_render_path", "emission_render_path", "soft_render_path",
                     "gloss_render_path"):
            getattr(lib_, name).restype = C.c_int
        lib_.mis_weight.restype = C.c_float
        lib_.mis_weight.argtypes = [C.c_float]
        _lib = lib_
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _WithMis:
    """soft_shadow_ref.render_path's library argument: its call of soft_render_path becomes mis_render_path with the same arguments
    and `extra` behind them."""

    def __init__(self, L, extra):
        self.L, self.extra = L, extra

    def soft_render_path(self, *args):
        return self.L.mis_render_path(*args, *self.extra)


def weight(L, g) -> float:
    """m(g), item 3, as the reference evaluates it (f32 in, f32 out)."""
    return float(L.mis_weight(C.c_float(g)))


def render_path(L, orc, cam_inv, screen, params, spheres, model, emissive_parts=None, emissive_spheres=None, light=False, parts=True,
                mis=True, entry="mis", **kw) -> dict:
    """mis_render_path with part_light_ref.render_path's arguments and the flag (mis: RWR_FLAG_LIGHT_MIS).  entry="parts":
    part_light_render_path with the same arguments - what a frame without the new flag must equal.  The result has part_light_ref's
    entries and "mis": (sphere hits weighted, face hits weighted, hits from inside an emitting sphere that kept Le, weighted hits
    whose value is not zero)."""
    if entry == "parts":
        return part_light_ref.render_path(L, orc, cam_inv, screen, params, spheres, model, emissive_parts=emissive_parts,
                                          emissive_spheres=emissive_spheres, light=light, parts=parts, **kw)
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
    kw.setdefault("shadows", False)
    extra = (_p(glow), _p(gen_glow), _p(glow_occluded), _p(capped), _p(by_surface), C.c_int(1 if light else 0), _p(light_gen), None, None,
             C.c_int(1 if parts else 0), _p(part_gen), _p(light_capped), C.c_int(1 if mis else 0), _p(mis_out))
    out = soft_shadow_ref.render_path(_WithMis(L, extra), orc, cam_inv, screen, params, spheres, model, coverage=False, **kw)
    lg, pg = light_gen.astype(np.int64), part_gen.astype(np.int64)
    out.update(gen_glow=gen_glow.astype(np.int64), emissive_hits=int(gen_glow.sum()), glow_occluded=int(glow_occluded[0]),
               capped=(int(capped[0]), int(capped[1])), glow_by_surface=by_surface.astype(np.int64), light_gen=lg,
               light_rays=int(lg[:, 0].sum()), reached=int(lg[:, 1].sum()), suppressed=int(lg[:, 2].sum()), part_gen=pg,
               part_light=(int(pg[:, 0].sum()), int(pg[:, 1].sum()), int(pg[:, 2].sum())), light_capped=int(light_capped[0]),
               mis=tuple(int(v) for v in mis_out))
    return out
