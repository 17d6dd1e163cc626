"""The tests' CPU reference of the Owen-scrambled Sobol sample sequence (RWR_FLAG_SOBOL, include/rwr_hip.h item 1):

  * rng_sobol / rng_hash here, in numpy, written from the header's definition line by line (sobol1 as its 32-step loop);
  * the stacked path references (mis_ref.c and everything it includes, down to the oracle) with rng_hash answering by the sequence
    when a switch is set.  The chain includes rt_oracle.c without guards, so no macro can redirect the calls alone: mis_ref.c is
    preprocessed into the pytest temporary directory, the one definition of rng_hash there is renamed, and the sequence and a
    dispatching rng_hash are put in front of it.  Nothing generated is kept.  With the switch off the library is mis_ref's."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np

import glass_ref
import mis_ref

U32 = np.uint32
_lib = None

PRELUDE = r"""
typedef unsigned int sob_u32;
static int sobol_ref_on = 0;
static inline sob_u32 rng_hash_plain(sob_u32 pixel, sob_u32 sample, sob_u32 dim, sob_u32 seed);
static sob_u32 sob_mix(sob_u32 x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
static sob_u32 sob_rev(sob_u32 x)
{
    sob_u32 r = 0u;
    for (int i = 0; i < 32; i++) { r = (r << 1) | (x & 1u); x >>= 1; }
    return r;
}
static sob_u32 sob_lk(sob_u32 x, sob_u32 s)
{
    x += s; x ^= x * 0x6c50b47cu; x ^= x * 0xb82f1e52u; x ^= x * 0xc7afe638u; x ^= x * 0x8d22f6e6u;
    return x;
}
static sob_u32 sob_owen(sob_u32 x, sob_u32 s) { return sob_rev(sob_lk(sob_rev(x), s)); }
static sob_u32 sob_sobol1(sob_u32 i)
{
    sob_u32 r = 0u, v = 1u << 31;
    while (i) { if (i & 1u) r ^= v; i >>= 1; v ^= v >> 1; }
    return r;
}
static sob_u32 sob_rng(sob_u32 pixel, sob_u32 sample, sob_u32 dim, sob_u32 seed)
{
    const sob_u32 h0 = sob_mix((seed ^ 0x9E3779B9u) ^ pixel);
    const sob_u32 s = sob_mix(h0 ^ ((dim >> 1) * 0xC2B2AE35u));
    const sob_u32 idx = sob_owen(sample, s);
    const sob_u32 x = (dim & 1u) ? sob_sobol1(idx) : sob_rev(idx);
    return sob_owen(x, sob_mix(s ^ (0x85EBCA6Bu + (dim & 1u))));
}
static inline sob_u32 rng_hash(sob_u32 pixel, sob_u32 sample, sob_u32 dim, sob_u32 seed)
{
    return sobol_ref_on ? sob_rng(pixel, sample, dim, seed) : rng_hash_plain(pixel, sample, dim, seed);
}
__attribute__((visibility("default"))) void sobol_ref_set(int on) { sobol_ref_on = on; }
__attribute__((visibility("default"))) sob_u32 sobol_ref_word(sob_u32 pixel, sob_u32 sample, sob_u32 dim, sob_u32 seed) { return sob_rng(pixel, sample, dim, seed); }
"""


def _u32(a):
    return np.asarray(a, dtype=np.uint64).astype(U32)


def mix(x):
    x = _u32(x).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U32(16); x *= U32(0x7feb352d); x ^= x >> U32(15); x *= U32(0x846ca68b); x ^= x >> U32(16)
    return x


def rev(x):
    x = _u32(x)
    r = np.zeros_like(x)
    for i in range(32):
        r |= ((x >> U32(i)) & U32(1)) << U32(31 - i)
    return r


def lk(x, s):
    with np.errstate(over="ignore"):
        x = _u32(x) + _u32(s)
        for c in (0x6c50b47c, 0xb82f1e52, 0xc7afe638, 0x8d22f6e6):
            x = x ^ (x * U32(c))
    return x


def owen(x, s):
    return rev(lk(rev(x), s))


def sobol1(i):
    """The definition's loop, all 32 steps (a step whose index bit is clear adds nothing)."""
    i = _u32(i)
    r = np.zeros_like(i)
    v = U32(1 << 31)
    for k in range(32):
        r = np.where((i >> U32(k)) & U32(1), r ^ v, r)
        v = v ^ (v >> U32(1))
    return r


def rng_sobol(pixel, sample, dim, seed):
    """RWR_FLAG_SOBOL's 32-bit word, elementwise over arrays (or scalars) of u32."""
    pixel, sample, dim, seed = np.broadcast_arrays(_u32(pixel), _u32(sample), _u32(dim), _u32(seed))
    with np.errstate(over="ignore"):
        h0 = mix((seed ^ U32(0x9E3779B9)) ^ pixel)
        s = mix(h0 ^ ((dim >> U32(1)) * U32(0xC2B2AE35)))
        idx = owen(sample, s)
        odd = dim & U32(1)
        x = np.where(odd != 0, sobol1(idx), rev(idx))
        return owen(x, mix(s ^ (U32(0x85EBCA6B) + odd)))


def uniform(word):
    """(u32 >> 8) * 2^-24, the integrator's conversion, as float64 (exact)."""
    return (_u32(word) >> U32(8)).astype(np.float64) / 16777216.0


def lib(tmp_path_factory) -> C.CDLL:
    """Builds the switched reference on first use (one build per session) and loads it; the switch starts off."""
    global _lib
    if _lib is None:
        tmp = str(tmp_path_factory.mktemp("sobol_ref"))
        cc, flags = glass_ref.compiler(), glass_ref.oracle_cflags()
        r = subprocess.run([cc] + flags + ["-E", "-P", mis_ref.SOURCE], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("preprocessing mis_ref.c failed:\n" + r.stderr)
        text, n = re.subn(r"\brng_hash(\s*\(\s*uint32_t\s+pixel\s*,\s*uint32_t\s+sample\s*,\s*uint32_t\s+dim\s*,\s*uint32_t\s+seed\s*\)\s*\{)", r"rng_hash_plain\1", r.stdout)
        assert n == 1, f"{n} definitions of rng_hash in the preprocessed reference, expected one"
        src = os.path.join(tmp, "sobol_ref_generated.c")
        with open(src, "w") as f:
            f.write(PRELUDE + text)
        out = os.path.join(tmp, "libsobol_ref.so")
        r = subprocess.run([cc] + flags + ["-shared", "-o", out, src, "-lm"], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("the switched reference's build failed:\n" + r.stdout + r.stderr)
        L = C.CDLL(out)
        for name in ("mis_render_path", "part_light_render_path", "part_light_table", "light_render_path", "emission_render_path", "soft_render_path",
                     "gloss_render_path"):
            getattr(L, name).restype = C.c_int
        L.mis_weight.restype = C.c_float
        L.mis_weight.argtypes = [C.c_float]
        L.or_rng_hash.restype = C.c_uint32
        L.or_rng_hash.argtypes = [C.c_uint32] * 4
        L.sobol_ref_word.restype = C.c_uint32
        L.sobol_ref_word.argtypes = [C.c_uint32] * 4
        L.sobol_ref_set.restype = None
        L.sobol_ref_set.argtypes = [C.c_int]
        _lib = L
    return _lib


def render_path(L, *args, sobol=True, **kw) -> dict:
    """mis_ref.render_path (same arguments) by the switched library, with every number drawn from the sequence (sobol=True) or from
    the hash."""
    L.sobol_ref_set(1 if sobol else 0)
    try:
        return mis_ref.render_path(L, *args, **kw)
    finally:
        L.sobol_ref_set(0)
