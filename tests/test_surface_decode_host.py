"""The kernels' decode of a surface record (csrc/rwr_surface.h decode_surface<SURF>) against the host's statement of it
(surface_model, surface_param), on every record a setter can store and under each of the seven sets of surface flags
(surface_host.cpp).  CPU only; built once per session the way bvh_host.py builds bvh_host.cpp."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import pytest

import bvh_host

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "surface_host.cpp")


@pytest.fixture(scope="session")
def surface_lib(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("surface_host")), "libsurface_host.so")
    cmd = [bvh_host.compiler(), "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-Wall", "-Wextra", "-I", bvh_host.CSRC, "-shared", "-o", out, SOURCE]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("surface_host.cpp build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
    lib = C.CDLL(out)
    lib.surface_host_check.restype = None
    lib.surface_host_check.argtypes = [C.POINTER(C.c_uint64)]
    return lib


def test_decode_agrees_with_the_host_statement_on_every_storable_record(surface_lib):
    out = (C.c_uint64 * 5)()
    surface_lib.surface_host_check(out)
    checked, bad, first_on, first_modes, values = (int(v) for v in out)
    # on in {0, 1}, every float in [-4, -1] (2 * 2^23 + 1 of them), every 1 + k 2^-23 for k = 2^13 ... 2^23
    assert values == 2 + (2 * (1 << 23) + 1) + ((1 << 23) - (1 << 13) + 1)
    assert checked == 7 * values
    assert bad == 0, f"{bad} disagreements, the first at on = bits 0x{first_on:08x}, modes {first_modes}"
