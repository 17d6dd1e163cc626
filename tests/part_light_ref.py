"""The tests' CPU reference of light sampling towards emitting mesh parts (part_light_ref.c, which includes light_ref.c unchanged and
with it the whole stack down to the oracle): built once per session into a pytest temporary directory with the oracle's own compiler
flags, the way light_ref.py builds its own, and called like light_ref.render_path."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import emission_ref
import glass_ref
import light_ref
import soft_shadow_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "part_light_ref.c")
MAX_SPHERES = emission_ref.MAX_SPHERES
TABLE_DTYPE = np.dtype([("cdf", "<f4"), ("face", "<u4"), ("inv_pdf", "<f4"), ("pad", "<u4")])   # rwr_part_lights.h PartLightRec

_lib = None


def lib(tmp_path_factory) -> C.CDLL:
    """Compiles part_light_ref.c on first use (one build per session) and loads it."""
    global _lib
    if _lib is None:
        out = os.path.join(str(tmp_path_factory.mktemp("part_light_ref")), "libpart_light_ref.so")
        cmd = [glass_ref.compiler()] + glass_ref.oracle_cflags() + ["-shared", "-o", out, SOURCE, "-lm"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("part_light_ref.c build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        lib_ = C.CDLL(out)
        for name in ("part_light_render_path", "part_light_table", "light_render_path", "emission_render_path", "soft_render_path", "gloss_render_path"):
            getattr(lib_, name).restype = C.c_int
        _lib = lib_
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _WithParts:
    """soft_shadow_ref.render_path's library argument: its call of soft_render_path becomes part_light_render_path with the same
    arguments and `extra` behind them."""

    def __init__(self, L, extra):
        self.L, self.extra = L, extra

    def soft_render_path(self, *args):
        return self.L.part_light_render_path(*args, *self.extra)


def render_path(L, orc, cam_inv, screen, params, spheres, model, emissive_parts=None, emissive_spheres=None, light=False, parts=True,
                entry="parts", **kw) -> dict:
    """part_light_render_path with light_ref.render_path's arguments and the two flags (light: RWR_FLAG_LIGHT_SAMPLING, parts:
    RWR_FLAG_LIGHT_PARTS).  entry="light": light_render_path with the same arguments - what a frame without the new flag must equal.
    The result has light_ref's entries - "light_gen", "light_rays", "reached", "suppressed" are the light stage's totals - and
    "part_gen" (int64[bounces + 1, 3]), "part_light" (the mesh light's share: rays, reached, suppressed) and "light_capped" (light
    terms with a channel at or above the cap of 64)."""
    if entry == "light":
        return light_ref.render_path(L, orc, cam_inv, screen, params, spheres, model, emissive_parts=emissive_parts,
                                     emissive_spheres=emissive_spheres, light=light, **kw)
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
    kw.setdefault("shadows", False)
    extra = (_p(glow), _p(gen_glow), _p(glow_occluded), _p(capped), _p(by_surface), C.c_int(1 if light else 0), _p(light_gen), None, None,
             C.c_int(1 if parts else 0), _p(part_gen), _p(light_capped))
    out = soft_shadow_ref.render_path(_WithParts(L, extra), orc, cam_inv, screen, params, spheres, model, coverage=False, **kw)
    lg, pg = light_gen.astype(np.int64), part_gen.astype(np.int64)
    out.update(gen_glow=gen_glow.astype(np.int64), emissive_hits=int(gen_glow.sum()), glow_occluded=int(glow_occluded[0]),
               capped=(int(capped[0]), int(capped[1])), glow_by_surface=by_surface.astype(np.int64), light_gen=lg,
               light_rays=int(lg[:, 0].sum()), reached=int(lg[:, 1].sum()), suppressed=int(lg[:, 2].sum()), part_gen=pg,
               part_light=(int(pg[:, 0].sum()), int(pg[:, 1].sum()), int(pg[:, 2].sum())), light_capped=int(light_capped[0]))
    return out


def scene_arrays(orc, model, instances=None):
    """The arrays of a model (one or a list of parts) as the reference takes them: vertices, faces, the part of every face, instances."""
    scene = orc.concat_parts(list(model) if isinstance(model, (list, tuple)) else [model])    # (as every reference's render_path)
    inst = None if instances is None or len(instances) == 0 else np.ascontiguousarray(instances, dtype=orc.INSTANCE_DTYPE)
    return (np.ascontiguousarray(scene["vertices"]), np.ascontiguousarray(scene["faces"]), np.ascontiguousarray(scene["face_material"], dtype=np.uint32), inst)


def table(L, orc, model, emissive_parts, instances=None) -> np.ndarray:
    """The reference's host table of a scene (part_light_table): a TABLE_DTYPE array, one record per listed face."""
    verts, faces, face_part, inst = scene_arrays(orc, model, instances)
    n_mat = len(model) if isinstance(model, (list, tuple)) else 1
    glow = np.ascontiguousarray(emission_ref.emission_table(n_mat, emissive_parts, {}), dtype=np.float32)
    cap = len(faces) * (len(inst) if inst is not None and len(inst) else 1)
    out = np.zeros(max(cap, 1), TABLE_DTYPE)
    n = L.part_light_table(_p(verts), C.c_uint32(len(verts)), _p(faces), C.c_uint32(len(faces)), _p(inst), C.c_uint32(0 if inst is None else len(inst)),
                           C.c_uint32(n_mat), _p(face_part), _p(glow), _p(out), C.c_uint32(cap))
    assert 0 <= n <= cap, n
    return out[:n]
