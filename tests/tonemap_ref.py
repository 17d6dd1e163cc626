"""The tests' CPU reference of the tone-mapping stage (tonemap_ref.c, RWR_FLAG_TONEMAP items 3-5): built once per session into a
pytest temporary directory with the oracle's own compiler flags (-ffp-contract=off among them), like denoise_ref.py."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import path_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "tonemap_ref.c")
CLAMP, REINHARD, ACES = 0, 1, 2
CURVES = (CLAMP, REINHARD, ACES)
DEFAULTS = {"curve": ACES, "auto_exposure": 0, "exposure": 1.0, "key": 0.18, "white": 4.0}   # include/rwr_hip.h rwr_tonemap_params

_lib = None


def lib(tmp_path_factory) -> C.CDLL:
    """Compiles tonemap_ref.c on first use (one build per session) and loads it."""
    global _lib
    if _lib is None:
        flags = path_ref.oracle_cflags()
        assert "-ffp-contract=off" in flags, flags
        out = os.path.join(str(tmp_path_factory.mktemp("tonemap_ref")), "libtonemap_ref.so")
        cmd = [path_ref.compiler()] + flags + ["-shared", "-o", out, SOURCE, "-lm"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("tonemap_ref.c build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        L = C.CDLL(out)
        f32, u32, vp = C.c_float, C.c_uint32, C.c_void_p
        L.tr_luma_bits.restype, L.tr_luma_bits.argtypes = C.c_int32, [f32, f32, f32]
        L.tr_measure.restype, L.tr_measure.argtypes = None, [vp, C.c_uint64, vp, vp]
        L.tr_exposure.restype, L.tr_exposure.argtypes = f32, [C.c_int64, u32, u32, f32, f32]
        L.tr_curve.restype, L.tr_curve.argtypes = f32, [f32, f32, u32, f32]
        L.tr_byte.restype, L.tr_byte.argtypes = C.c_uint8, [f32]
        L.tr_tonemap.restype, L.tr_tonemap.argtypes = f32, [vp, C.c_uint64, u32, u32, f32, f32, f32, vp, vp, vp]
        L.tr_curve_bytes.restype, L.tr_curve_bytes.argtypes = None, [u32, f32, f32, C.c_uint64, vp]
        _lib = L
    return _lib


def bits(v) -> int:
    """The 32 bits of a float32 value."""
    return int(np.float32(v).view(np.uint32))


def measure(L, color_f32) -> tuple[int, int]:
    """(log_sum, count) of a (..., 4) float32 plane."""
    plane = np.ascontiguousarray(color_f32, dtype=np.float32).reshape(-1, 4)
    s, c = C.c_int64(0), C.c_uint32(0)
    L.tr_measure(plane.ctypes.data, len(plane), C.addressof(s), C.addressof(c))
    return int(s.value), int(c.value)


def tonemap(L, color_f32, curve=ACES, auto_exposure=0, exposure=1.0, key=0.18, white=4.0) -> dict:
    """The definition applied to a frame's color_f32 plane: {"color": the rgba8 plane, "log_sum", "count", "exposure": E as float32}."""
    plane = np.ascontiguousarray(color_f32, dtype=np.float32)
    assert plane.shape[-1] == 4
    out8 = np.zeros(plane.shape, np.uint8)
    s, c = C.c_int64(0), C.c_uint32(0)
    E = L.tr_tonemap(plane.ctypes.data, plane.size // 4, curve, auto_exposure, exposure, key, white, out8.ctypes.data, C.addressof(s), C.addressof(c))
    return {"color": out8, "log_sum": int(s.value), "count": int(c.value), "exposure": np.float32(E)}


def curve_bytes(L, curve, white, step, n) -> np.ndarray:
    """The bytes of x_i = i * step, i < n, under one curve with E = 1."""
    out = np.zeros(n, np.uint8)
    L.tr_curve_bytes(curve, white, step, n, out.ctypes.data)
    return out
