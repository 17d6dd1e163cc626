"""The tests' CPU reference of glossy surfaces (gloss_ref.c, which includes glass_ref.c unchanged and with it mirror_ref.c,
sky_ref.c, shadow_ref.c, path_ref.c and the oracle): built once per session into a pytest temporary directory with the oracle's
own compiler flags, the way glass_ref.py builds its own, and called like glass_ref.render_path."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import glass_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "gloss_ref.c")
MAX_SPHERES = glass_ref.MAX_SPHERES

_lib = None


def lib(tmp_path_factory) -> C.CDLL:
    """Compiles gloss_ref.c on first use (one build per session) and loads it."""
    global _lib
    if _lib is None:
        out = os.path.join(str(tmp_path_factory.mktemp("gloss_ref")), "libgloss_ref.so")
        cmd = [glass_ref.compiler()] + glass_ref.oracle_cflags() + ["-shared", "-o", out, SOURCE, "-lm"]   # (-fopenmp is among the oracle's flags)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("gloss_ref.c build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        lib_ = C.CDLL(out)
        lib_.glass_render_path.restype = C.c_int
        lib_.gloss_render_path.restype = C.c_int
        lib_.gloss_ref_scatter.restype = None
        lib_.gloss_ref_scatter.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib_.pr_bounce_direction.restype = None
        _lib = lib_
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def roughness_of(rough) -> np.float32:
    """The roughness a surface set with `rough` has: (1.0f + rough) - 1.0f, as the surface table keeps it (a multiple of 2^-23)."""
    return np.float32(np.float32(1.0) + np.float32(rough)) - np.float32(1.0)


def scatter(L, n, d, rho, pixel=0, sample=0, dim=2, seed=0):
    """gloss_ref.c's gloss_scatter: (S, Rf) of a hit with HitRecord normal n by a ray of direction d on a surface of roughness rho."""
    out, refl = np.zeros(3, np.float32), np.zeros(3, np.float32)
    L.gloss_ref_scatter(_p(np.ascontiguousarray(n, dtype=np.float32)), _p(np.ascontiguousarray(d, dtype=np.float32)), float(np.float32(rho)),
                        pixel, sample, dim, seed, _p(out), _p(refl))
    return out, refl


def bounce_direction(L, n, pixel=0, sample=0, dim=2, seed=0) -> np.ndarray:
    """path_ref.c's bounce direction of the same dimensions: the diffuse ray the hit would have sent."""
    out = np.zeros(3, np.float32)
    L.pr_bounce_direction(_p(np.ascontiguousarray(n, dtype=np.float32)), C.c_uint32(pixel), C.c_uint32(sample), C.c_uint32(seed), C.c_uint32(dim), _p(out))
    return out


def surface_table(n_parts: int, mirror_parts=None, mirror_spheres=None, glass_parts=None, glass_spheres=None, gloss_parts=None,
                  gloss_spheres=None) -> np.ndarray:
    """glass_ref.surface_table plus {index: (roughness, (r, g, b))} glossy surfaces: w = 1.0f + roughness."""
    t = glass_ref.surface_table(n_parts, mirror_parts, mirror_spheres, glass_parts, glass_spheres)
    for base, items in ((0, gloss_parts), (n_parts, gloss_spheres)):
        for k, (rough, refl) in (items or {}).items():
            t[base + k, :3] = np.asarray(refl, np.float32); t[base + k, 3] = np.float32(1.0) + np.float32(rough)
    return t


def render_path(L, orc, cam_inv, screen, params, spheres, model, instances=None, rows=None, shadows=False, sky=None,
                mirror_parts=None, mirror_spheres=None, glass_parts=None, glass_spheres=None, gloss_parts=None, gloss_spheres=None,
                use_glass_ref=False, thr_unorm16=False) -> dict:
    """gloss_render_path with glass_ref.render_path's arguments and the glossy surfaces, {part: (roughness, reflectance)} and
    {sphere index: (roughness, reflectance)} (None: none).  The result has glass_ref's entries and "gen_gloss": the glossy rays per
    generation, "glossy": their sum.  use_glass_ref=True calls glass_render_path of the same library instead (no glossy surface):
    what the reference must equal without one."""
    scene = orc.concat_parts(list(model) if isinstance(model, (list, tuple)) else [model])
    w, h = int(screen["width"][0]), int(screen["height"][0])
    r0, r1 = rows if rows is not None else (0, h)
    color = np.zeros((h, w, 4), np.uint8)
    depth = np.zeros((h, w), np.float32)
    color_f = np.zeros((h, w, 4), np.float32)
    obj_id = np.full((h, w), -1, np.int32)
    hit_t = np.zeros((h, w), np.float32)
    texs = scene["textures"]
    n_mat = len(texs)
    ptrs = (C.c_void_p * n_mat)(*[t.ctypes.data for t in texs])
    ws = np.array([t.shape[1] for t in texs], np.uint32)
    hs = np.array([t.shape[0] for t in texs], np.uint32)
    n_inst = 0 if instances is None else len(instances)
    inst = None if n_inst == 0 else np.ascontiguousarray(instances, dtype=orc.INSTANCE_DTYPE)
    mats = np.ascontiguousarray(scene["materials"])
    fmat = np.ascontiguousarray(scene["face_material"], dtype=np.uint32)
    nts = scene.get("normal_textures") or [None] * n_mat
    nptrs = (C.c_void_p * n_mat)(*[None if t is None else t.ctypes.data for t in nts])
    nws = np.array([0 if t is None else t.shape[1] for t in nts], np.uint32)
    nhs = np.array([0 if t is None else t.shape[0] for t in nts], np.uint32)
    rays = np.zeros(1, np.uint64)
    shadow_rays = np.zeros(1, np.uint64)
    occluded = np.zeros(1, np.uint64)
    occl0 = np.zeros((h, w), np.uint8)
    sky_terms = np.zeros(1, np.uint64)
    bounces = int(params["max_bounces"][0])
    sky_a = None if sky is None else glass_ref.sky_array(sky)
    table = None
    if mirror_parts or mirror_spheres or glass_parts or glass_spheres or gloss_parts or gloss_spheres:
        table = np.ascontiguousarray(surface_table(n_mat, mirror_parts, mirror_spheres, glass_parts, glass_spheres, gloss_parts, gloss_spheres))
    events = np.zeros(3, np.uint64)
    multi = np.zeros(1, np.uint64)
    deep = np.zeros(1, np.uint64)
    gen_glass = np.zeros(bounces + 1, np.uint64)
    gen_mirror = np.zeros(bounces + 1, np.uint64)
    gen_rays = np.zeros(bounces + 1, np.uint64)
    gen_gloss = np.zeros(bounces + 1, np.uint64)
    args = [_p(cam_inv), _p(screen), _p(params), _p(spheres), C.c_uint32(len(spheres)),
            _p(scene["vertices"]), C.c_uint32(len(scene["vertices"])), _p(scene["faces"]), C.c_uint32(len(scene["faces"])),
            _p(inst), C.c_uint32(n_inst), _p(mats), C.c_uint32(n_mat), _p(fmat), ptrs, _p(ws), _p(hs), nptrs, _p(nws), _p(nhs),
            C.c_uint32(r0), C.c_uint32(r1), _p(color), _p(depth), _p(color_f), _p(obj_id), _p(hit_t), _p(rays),
            C.c_int(int(shadows)), _p(shadow_rays), _p(occluded), _p(occl0), _p(sky_a), _p(sky_terms), None,
            _p(table), _p(gen_mirror), _p(gen_rays), None, _p(events), _p(multi), _p(deep), _p(gen_glass), C.c_int(int(thr_unorm16))]
    if use_glass_ref:
        assert not gloss_parts and not gloss_spheres
        rc = L.glass_render_path(*args)
    else:
        rc = L.gloss_render_path(*args, _p(gen_gloss))
    if rc != 0:
        raise MemoryError("gloss_render_path")
    return {"color": color, "depth": depth, "color_f32": color_f, "obj_id": obj_id, "hit_t": hit_t, "rays": int(rays[0]),
            "shadow_rays": int(shadow_rays[0]), "occluded": int(occluded[0]), "occluded0": occl0, "sky_terms": int(sky_terms[0]),
            "gen_mirror": gen_mirror.astype(np.int64), "gen_rays": gen_rays.astype(np.int64),
            "events": tuple(int(v) for v in events), "multi": int(multi[0]), "deep": int(deep[0]), "gen_glass": gen_glass.astype(np.int64),
            "gen_gloss": gen_gloss.astype(np.int64), "glossy": int(gen_gloss.sum())}
