"""The tests' CPU reference of temporal reprojection (reproject_ref.c, which includes the oracle): built once per session into a
pytest temporary directory with the oracle's own compiler flags (-ffp-contract=off among them), like denoise_ref.py."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import path_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "reproject_ref.c")
DEFAULTS = {"max_history": 32, "normal_cos_min": 0.95, "depth_rel": 0.05}   # include/rwr_hip.h rwr_reproject_params
CAMERA_DTYPE = np.dtype([("o", "<f4", 3), ("c0", "<f4", 3), ("cx", "<f4", 3), ("cy", "<f4", 3), ("nrm", "<f4", 3), ("nc0", "<f4"), ("nn", "<f4")])
# rr_frame's per-pixel diagnostics
DIAG = ("counting", "outside", "refused_id", "refused_depth", "by_normal", "behind", "reused")

_lib = None


def lib(tmp_path_factory, source=SOURCE, defines=()) -> C.CDLL:
    """Compiles reproject_ref.c on first use (one build per session) and loads it.  (source / defines: a variant of the reference
    built beside it, never cached.)"""
    global _lib
    if _lib is not None and source == SOURCE and not defines:
        return _lib
    flags = path_ref.oracle_cflags()
    assert "-ffp-contract=off" in flags, flags
    out = os.path.join(str(tmp_path_factory.mktemp("reproject_ref")), "libreproject_ref.so")
    cmd = [path_ref.compiler()] + flags + list(defines) + ["-shared", "-o", out, source, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("reproject_ref.c build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
    lib_ = C.CDLL(out)
    lib_.rr_camera.restype = None
    lib_.rr_centre_point.restype = None
    lib_.rr_project.restype = C.c_int
    lib_.rr_frame.restype = None
    if source == SOURCE and not defines:
        _lib = lib_
    return lib_


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def camera(L, cam_inv) -> np.ndarray:
    """What the history keeps of a frame's camera: c0, cx, cy, nrm, the origin and the two dot products."""
    cam_inv = np.ascontiguousarray(cam_inv)
    assert cam_inv.dtype.itemsize == 144
    out = np.zeros(1, CAMERA_DTYPE)
    L.rr_camera(_p(cam_inv), _p(out))
    return out


def centre_point(L, cam_inv, w, h, x, y, t) -> np.ndarray:
    """P = O + t Dc of pixel (x, y), f32."""
    out = np.zeros(3, np.float32)
    L.rr_centre_point(_p(np.ascontiguousarray(cam_inv)), C.c_uint32(w), C.c_uint32(h), C.c_uint32(x), C.c_uint32(y), C.c_float(t), _p(out))
    return out


def project(L, rc, P, w, h):
    """(fx, fy, te) of world point P in the frame of camera record rc, or None when mu > 0 fails."""
    out = np.zeros(3, np.float32)
    ok = L.rr_project(_p(rc), _p(np.ascontiguousarray(P, np.float32)), C.c_uint32(w), C.c_uint32(h), _p(out))
    return (float(out[0]), float(out[1]), float(out[2])) if ok else None


def frame(L, planes, nhat, cam_inv, prev=None, max_history=32, normal_cos_min=0.95, depth_rel=0.05) -> dict:
    """One frame of the definition.  planes: {"color_f32", "obj_id", "hit_t"} of the frame as traced (c_now); prev: the result of
    the frame before (None: frame 0).  The result: "color_f32" (out), "color", "n" (n'), "obj_id", "hit_t", "camera",
    "counts" (reused, fresh, background), "diag" {name: (H, W) int32} (DIAG)."""
    c_now = np.ascontiguousarray(planes["color_f32"], dtype=np.float32)
    obj_id = np.ascontiguousarray(planes["obj_id"], dtype=np.int32)
    hit_t = np.ascontiguousarray(planes["hit_t"], dtype=np.float32)
    nhat = np.ascontiguousarray(nhat, dtype=np.float32).reshape(-1, 3)
    h, w = obj_id.shape
    assert c_now.shape == (h, w, 4) and hit_t.shape == (h, w)
    assert obj_id.max(initial=-1) < len(nhat)
    if len(nhat) == 0:
        nhat = np.zeros((1, 3), np.float32)   # (a scene whose faces are never seen: never read)
    cam_inv = np.ascontiguousarray(cam_inv)
    out = np.zeros_like(c_now)
    out8 = np.zeros((h, w, 4), np.uint8)
    n1 = np.zeros((h, w), np.float32)
    counts = np.zeros(3, np.uint64)
    diag = np.zeros((h, w, len(DIAG)), np.int32)
    if prev is not None:
        assert prev["obj_id"].shape == (h, w)
        pa = [_p(prev["camera"]), _p(np.ascontiguousarray(prev["color_f32"])), _p(np.ascontiguousarray(prev["n"])),
              _p(np.ascontiguousarray(prev["obj_id"])), _p(np.ascontiguousarray(prev["hit_t"]))]
    else:
        pa = [None] * 5
    L.rr_frame(C.c_uint32(w), C.c_uint32(h), _p(c_now), _p(obj_id), _p(hit_t), _p(nhat), _p(cam_inv), C.c_uint32(max_history),
               C.c_float(normal_cos_min), C.c_float(depth_rel), *pa, _p(out), _p(out8), _p(n1), _p(counts), _p(diag))
    return {"color_f32": out, "color": out8, "n": n1, "obj_id": obj_id, "hit_t": hit_t, "camera": camera(L, cam_inv),
            "counts": tuple(int(v) for v in counts), "diag": {k: diag[..., i] for i, k in enumerate(DIAG)}}


def chain(L, frames, nhat, cams, **params) -> list:
    """The definition over a sequence: frames[k] are the planes of frame k as traced, cams[k] its camera uniform."""
    out, prev = [], None
    for planes, cam in zip(frames, cams):
        prev = frame(L, planes, nhat, cam, prev, **params)
        out.append(prev)
    return out
