"""The tests' CPU reference of glass surfaces (glass_ref.c, which includes mirror_ref.c and with it sky_ref.c, shadow_ref.c,
path_ref.c and the oracle): built once per session into a pytest temporary directory with the oracle's own compiler flags, the
way mirror_ref.py builds its own, and called like mirror_ref.render_path."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCE = os.path.join(HERE, "glass_ref.c")

_lib = None


def compiler() -> str:
    """$CC, else gcc, else ROCm's clang."""
    cc = os.environ.get("CC")
    if cc:
        return cc
    if shutil.which("gcc"):
        return "gcc"
    return "/opt/rocm/llvm/bin/clang"


def oracle_cflags() -> list:
    """CFLAGS exactly as oracle/Makefile sets them (continuation lines joined)."""
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^CFLAGS\s*\?=\s*(.*)$", text, re.M)
    return m.group(1).split()


def lib(tmp_path_factory) -> C.CDLL:
    """Compiles glass_ref.c on first use (one build per session) and loads it."""
    global _lib
    if _lib is None:
        out = os.path.join(str(tmp_path_factory.mktemp("glass_ref")), "libglass_ref.so")
        cmd = [compiler()] + oracle_cflags() + ["-shared", "-o", out, SOURCE, "-lm"]   # (-fopenmp is among the oracle's flags)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("glass_ref.c build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        lib_ = C.CDLL(out)
        lib_.sky_render_path.restype = C.c_int
        lib_.mirror_render_path.restype = C.c_int
        lib_.glass_render_path.restype = C.c_int
        lib_.glass_ref_scatter.restype = None
        lib_.glass_ref_scatter.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
        lib_.or_rng_hash.restype = C.c_uint32
        lib_.or_rng_hash.argtypes = [C.c_uint32] * 4
        lib_.mirror_ref_reflect.restype = None
        lib_.mirror_ref_reflect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib_.sky_ref_radiance.restype = None
        lib_.sky_ref_radiance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = lib_
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


DEFAULT_ZENITH, DEFAULT_HORIZON = (0.5, 0.7, 1.0), (1.0, 1.0, 1.0)   # include/rwr_hip.h rwr_sky_params


def sky_array(sky) -> np.ndarray:
    """(zenith, horizon) -> the six floats of rwr_sky_params."""
    return np.ascontiguousarray(np.concatenate([np.asarray(sky[0], np.float32), np.asarray(sky[1], np.float32)]))


def radiance(L, sky, d) -> np.ndarray:
    """S(d) of the sky (zenith, horizon), by the reference's own routine."""
    out = np.zeros(3, np.float32)
    L.sky_ref_radiance(_p(sky_array(sky)), _p(np.ascontiguousarray(d, dtype=np.float32)), _p(out))
    return out


MAX_SPHERES = 8   # include/rwr_hip.h RWR_MAX_SPHERES


def scatter(L, n, d, face, face_entering, eta, pixel=0, sample=0, dim=2, seed=0):
    """glass_ref.c's glass_scatter: (D', m, event) of a hit with HitRecord normal n by a ray of direction d on glass of index eta;
    event 0 reflected, 1 transmitted, 2 totally reflected."""
    out, side, ev = np.zeros(3, np.float32), np.zeros(3, np.float32), C.c_int(-1)
    L.glass_ref_scatter(_p(np.ascontiguousarray(n, dtype=np.float32)), _p(np.ascontiguousarray(d, dtype=np.float32)), int(face), int(face_entering),
                        float(eta), pixel, sample, dim, seed, _p(out), _p(side), C.byref(ev))
    return out, side, ev.value


def surface_table(n_parts: int, mirror_parts=None, mirror_spheres=None, glass_parts=None, glass_spheres=None) -> np.ndarray:
    """{index: (r, g, b)} mirrors and {index: (ior, (r, g, b))} glass -> the reference's table: a record {r, g, b, w} per part, then per
    sphere index; w = 1 a mirror, w = -ior glass."""
    t = np.zeros((n_parts + MAX_SPHERES, 4), np.float32)
    for base, items in ((0, mirror_parts), (n_parts, mirror_spheres)):
        for k, r in (items or {}).items():
            t[base + k, :3] = np.asarray(r, np.float32); t[base + k, 3] = 1.0
    for base, items in ((0, glass_parts), (n_parts, glass_spheres)):
        for k, (ior, tint) in (items or {}).items():
            t[base + k, :3] = np.asarray(tint, np.float32); t[base + k, 3] = -np.float32(ior)
    return t


def render_path(L, orc, cam_inv, screen, params, spheres, model, instances=None, rows=None, shadows=False, sky=None, misses=False,
                mirror_parts=None, mirror_spheres=None, first=False, glass_parts=None, glass_spheres=None, use_mirror_ref=False, thr_unorm16=False) -> dict:
    """glass_render_path with mirror_ref.render_path's arguments and the glass surfaces, {part: (ior, tint)} and
    {sphere index: (ior, tint)} (None: none).  The result has mirror_ref's entries and "events": (reflected, transmitted, totally
    reflected), "multi": the paths with two or more transmissions, "deep": those with four or more, "gen_glass": the glass events
    per generation.  thr_unorm16=True rounds the throughput every bounce ray carries to unorm16, as the product's ray record does.
    use_mirror_ref=True calls mirror_render_path of the same library instead (no glass): what the reference must equal without it."""
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
    spp = max(1, int(params["spp"][0]))
    bounces = int(params["max_bounces"][0])
    miss = np.zeros((h, w, spp, 8), np.float32) if misses else None
    sky_a = None if sky is None else sky_array(sky)
    table = None
    if mirror_parts or mirror_spheres or glass_parts or glass_spheres:
        table = np.ascontiguousarray(surface_table(n_mat, mirror_parts, mirror_spheres, glass_parts, glass_spheres))
    events = np.zeros(3, np.uint64)
    multi = np.zeros(1, np.uint64)
    deep = np.zeros(1, np.uint64)
    gen_glass = np.zeros(bounces + 1, np.uint64)
    gen_mirror = np.zeros(bounces + 1, np.uint64)
    gen_rays = np.zeros(bounces + 1, np.uint64)
    first_a = np.zeros((h, w, spp, 8), np.float32) if first else None
    args = [_p(cam_inv), _p(screen), _p(params), _p(spheres), C.c_uint32(len(spheres)),
            _p(scene["vertices"]), C.c_uint32(len(scene["vertices"])), _p(scene["faces"]), C.c_uint32(len(scene["faces"])),
            _p(inst), C.c_uint32(n_inst), _p(mats), C.c_uint32(n_mat), _p(fmat), ptrs, _p(ws), _p(hs), nptrs, _p(nws), _p(nhs),
            C.c_uint32(r0), C.c_uint32(r1), _p(color), _p(depth), _p(color_f), _p(obj_id), _p(hit_t), _p(rays),
            C.c_int(int(shadows)), _p(shadow_rays), _p(occluded), _p(occl0), _p(sky_a), _p(sky_terms), _p(miss)]
    if use_mirror_ref:
        assert not glass_parts and not glass_spheres
        rc = L.mirror_render_path(*args, _p(table), _p(gen_mirror), _p(gen_rays), _p(first_a))
    else:
        rc = L.glass_render_path(*args, _p(table), _p(gen_mirror), _p(gen_rays), _p(first_a), _p(events), _p(multi), _p(deep), _p(gen_glass), C.c_int(int(thr_unorm16)))
    if rc != 0:
        raise MemoryError("glass_render_path")
    return {"color": color, "depth": depth, "color_f32": color_f, "obj_id": obj_id, "hit_t": hit_t, "rays": int(rays[0]),
            "shadow_rays": int(shadow_rays[0]), "occluded": int(occluded[0]), "occluded0": occl0, "sky_terms": int(sky_terms[0]), "misses": miss,
            "gen_mirror": gen_mirror.astype(np.int64), "gen_rays": gen_rays.astype(np.int64), "first": first_a,
            "events": tuple(int(v) for v in events), "multi": int(multi[0]), "deep": int(deep[0]), "gen_glass": gen_glass.astype(np.int64)}
