"""The tests' CPU reference of soft shadows (soft_shadow_ref.c, which includes gloss_ref.c unchanged and with it the whole stack
down to the oracle): built once per session into a pytest temporary directory with the oracle's own compiler flags, the way
gloss_ref.py builds its own, and called like gloss_ref.render_path."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import glass_ref
import gloss_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "soft_shadow_ref.c")

_lib = None


def lib(tmp_path_factory) -> C.CDLL:
    """Compiles soft_shadow_ref.c on first use (one build per session) and loads it."""
    global _lib
    if _lib is None:
        out = os.path.join(str(tmp_path_factory.mktemp("soft_shadow_ref")), "libsoft_shadow_ref.so")
        cmd = [glass_ref.compiler()] + glass_ref.oracle_cflags() + ["-shared", "-o", out, SOURCE, "-lm"]   # (-fopenmp is among the oracle's flags)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("soft_shadow_ref.c build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        lib_ = C.CDLL(out)
        lib_.soft_render_path.restype = C.c_int
        lib_.gloss_render_path.restype = C.c_int
        lib_.sr_render_path.restype = C.c_int
        lib_.soft_ref_direction.restype = None
        lib_.soft_ref_direction.argtypes = [C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        _lib = lib_
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def direction(L, light, r, pixel=0, sample=0, k=0, seed=0) -> np.ndarray:
    """soft_shadow_ref.c's ss_direction: S for the shadow ray of hit h_k towards the light of radius r about the unit vector `light`."""
    out = np.zeros(3, np.float32)
    L.soft_ref_direction(_p(np.ascontiguousarray(light, dtype=np.float32)), float(np.float32(r)), pixel, sample, k, seed, _p(out))
    return out


def render_path(L, orc, cam_inv, screen, params, spheres, model, instances=None, rows=None, shadows=True, radii=None, sky=None, coverage=True,
                mirror_parts=None, mirror_spheres=None, glass_parts=None, glass_spheres=None, gloss_parts=None, gloss_spheres=None) -> dict:
    """soft_render_path with gloss_ref.render_path's arguments and radii = (mesh light, sphere light); None: the hard shadow ray.
    The result has gloss_ref's entries and "changed_to_lit", "changed_to_dark" (shadow rays whose visibility differs from the hard
    ray's from the same origin; coverage=False: the hard ray is not traced and both are 0) and "primary": (H, W, 2) uint32 {primary hits, lit primary hits} over the frame's samples."""
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
        table = np.ascontiguousarray(gloss_ref.surface_table(n_mat, mirror_parts, mirror_spheres, glass_parts, glass_spheres, gloss_parts, gloss_spheres))
    events = np.zeros(3, np.uint64)
    multi = np.zeros(1, np.uint64)
    deep = np.zeros(1, np.uint64)
    gen_glass = np.zeros(bounces + 1, np.uint64)
    gen_mirror = np.zeros(bounces + 1, np.uint64)
    gen_rays = np.zeros(bounces + 1, np.uint64)
    gen_gloss = np.zeros(bounces + 1, np.uint64)
    radii_a = None if radii is None else np.ascontiguousarray(radii, dtype=np.float32).reshape(2)
    changed = np.zeros(2, np.uint64)
    primary = np.zeros((h, w, 2), np.uint32)
    rc = L.soft_render_path(
        _p(cam_inv), _p(screen), _p(params), _p(spheres), C.c_uint32(len(spheres)),
        _p(scene["vertices"]), C.c_uint32(len(scene["vertices"])), _p(scene["faces"]), C.c_uint32(len(scene["faces"])),
        _p(inst), C.c_uint32(n_inst), _p(mats), C.c_uint32(n_mat), _p(fmat), ptrs, _p(ws), _p(hs), nptrs, _p(nws), _p(nhs),
        C.c_uint32(r0), C.c_uint32(r1), _p(color), _p(depth), _p(color_f), _p(obj_id), _p(hit_t), _p(rays),
        C.c_int(int(shadows)), _p(shadow_rays), _p(occluded), _p(occl0), _p(sky_a), _p(sky_terms), None,
        _p(table), _p(gen_mirror), _p(gen_rays), None, _p(events), _p(multi), _p(deep), _p(gen_glass), C.c_int(0),
        _p(gen_gloss), _p(radii_a), _p(changed) if coverage else None, _p(primary))
    if rc != 0:
        raise MemoryError("soft_render_path")
    return {"color": color, "depth": depth, "color_f32": color_f, "obj_id": obj_id, "hit_t": hit_t, "rays": int(rays[0]),
            "shadow_rays": int(shadow_rays[0]), "occluded": int(occluded[0]), "occluded0": occl0, "sky_terms": int(sky_terms[0]),
            "gen_rays": gen_rays.astype(np.int64), "gen_gloss": gen_gloss.astype(np.int64), "glossy": int(gen_gloss.sum()),
            "changed_to_lit": int(changed[0]), "changed_to_dark": int(changed[1]), "primary": primary,
            "events": tuple(int(v) for v in events), "gen_mirror": gen_mirror.astype(np.int64), "gen_glass": gen_glass.astype(np.int64)}


def reference(L, orc, sc, cam_inv, w, h, spp, bounces, seed=7, radii=None, shadows=True, rows=None, **kw):
    """shadow_common.reference's call shape: sc = (model or parts, spheres, instances, eye, target, extra flags)."""
    model, spheres, inst, _, _, flags = sc
    return render_path(L, orc, cam_inv, orc.make_screen(w, h), orc.make_params(spp, bounces, seed=seed, flags=flags), spheres, model,
                       instances=inst, rows=rows, shadows=shadows, radii=radii, **kw)
