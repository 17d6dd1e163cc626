"""The tests' CPU reference of the a-trous denoiser (denoise_ref.c, which includes the oracle): built once per session into a
pytest temporary directory with the oracle's own compiler flags (-ffp-contract=off among them), like path_ref.py."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import path_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "denoise_ref.c")
DEFAULTS = {"iterations": 5, "sigma_color": 0.04, "normal_cos_min": 0.95, "depth_rel": 0.05}   # include/rwr_hip.h rwr_denoise_params

_lib = None


def lib(tmp_path_factory) -> C.CDLL:
    """Compiles denoise_ref.c on first use (one build per session) and loads it."""
    global _lib
    if _lib is None:
        flags = path_ref.oracle_cflags()
        assert "-ffp-contract=off" in flags, flags
        out = os.path.join(str(tmp_path_factory.mktemp("denoise_ref")), "libdenoise_ref.so")
        cmd = [path_ref.compiler()] + flags + ["-shared", "-o", out, SOURCE, "-lm"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("denoise_ref.c build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        lib_ = C.CDLL(out)
        lib_.dr_face_normals.restype = None
        lib_.dr_denoise.restype = C.c_int
        _lib = lib_
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def face_normals(L, orc, model, instances=None) -> np.ndarray:
    """nhat of every face in object-id order (one model dict or a list of parts; instances: the oracle's dtype or None)."""
    scene = orc.concat_parts(list(model) if isinstance(model, (list, tuple)) else [model])
    verts, faces = np.ascontiguousarray(scene["vertices"]), np.ascontiguousarray(scene["faces"])
    n_inst = 0 if instances is None else len(instances)
    inst = None if n_inst == 0 else np.ascontiguousarray(instances, dtype=orc.INSTANCE_DTYPE)
    out = np.zeros((len(faces) * max(1, n_inst), 3), np.float32)
    L.dr_face_normals(_p(verts), _p(faces), C.c_uint32(len(faces)), _p(inst), C.c_uint32(n_inst), _p(out))
    return out


def denoise(L, color_f32, obj_id, hit_t, nhat, iterations=5, sigma_color=0.04, normal_cos_min=0.95, depth_rel=0.05) -> dict:
    """The definition applied to the planes of a frame; {"color_f32", "color"}."""
    color_f32 = np.ascontiguousarray(color_f32, dtype=np.float32)
    obj_id = np.ascontiguousarray(obj_id, dtype=np.int32)
    hit_t = np.ascontiguousarray(hit_t, dtype=np.float32)
    nhat = np.ascontiguousarray(nhat, dtype=np.float32)
    h, w = obj_id.shape
    assert color_f32.shape == (h, w, 4) and hit_t.shape == (h, w)
    assert obj_id.max(initial=-1) < len(nhat)
    out = np.zeros_like(color_f32)
    out8 = np.zeros((h, w, 4), np.uint8)
    rc = L.dr_denoise(C.c_uint32(w), C.c_uint32(h), _p(color_f32), _p(obj_id), _p(hit_t), _p(nhat), C.c_uint32(iterations),
                      C.c_float(sigma_color), C.c_float(normal_cos_min), C.c_float(depth_rel), _p(out), _p(out8))
    if rc != 0:
        raise MemoryError("dr_denoise")
    return {"color_f32": out, "color": out8}
