"""Progressive accumulation (RWR_FLAG_ACCUMULATE) at the boundary, without a GPU: the header declares the flag and both
calls, the library exports them, NULL arguments are refused before anything touches a device, and the host program
offers --accumulate."""
import ctypes as C
import os
import re
import subprocess


def _header(rwr):
    with open(rwr.HEADER_PATH) as fh:
        return fh.read()


def test_header_declares_flag_and_calls(rwr):
    text = _header(rwr)
    assert re.search(r"\bRWR_FLAG_ACCUMULATE\s*=\s*1u\s*<<\s*5\b", text)
    assert re.search(r"RWR_API\s+int\s+rwr_accum_reset\s*\(\s*rwr_context\s*\*\s*ctx\s*\)\s*;", text)
    assert re.search(r"RWR_API\s+int\s+rwr_accum_samples\s*\(\s*rwr_context\s*\*\s*ctx\s*,\s*uint64_t\s*\*\s*samples\s*\)\s*;", text)
    assert "RWR_ACCUM_MAX_SAMPLES" in text
    assert rwr.FLAG_ACCUMULATE == 1 << 5
    # the render parameters keep their 16-byte layout
    assert rwr.PARAMS_DTYPE.itemsize == 16


def test_library_exports_accumulation_calls(rwr):
    names = rwr.exported_symbols_declared_in_header()
    assert "rwr_accum_reset" in names and "rwr_accum_samples" in names
    lib = rwr.lib()
    assert hasattr(lib, "rwr_accum_reset") and hasattr(lib, "rwr_accum_samples")


def test_null_arguments_are_invalid(rwr):
    lib = rwr.lib()
    n = C.c_uint64(7)
    assert lib.rwr_accum_reset(None) == rwr.ERR_INVALID_ARGUMENT
    assert lib.rwr_accum_samples(None, C.byref(n)) == rwr.ERR_INVALID_ARGUMENT
    assert n.value == 7                                  # untouched
    assert lib.rwr_accum_samples(None, None) == rwr.ERR_INVALID_ARGUMENT
    # a non-NULL context with a NULL output: refused before the context is looked at (any non-NULL pointer will do)
    dummy = C.create_string_buffer(64)
    assert lib.rwr_accum_samples(C.cast(dummy, C.c_void_p), None) == rwr.ERR_INVALID_ARGUMENT
    assert b"NULL" in lib.rwr_last_error_string()


def test_cli_help_lists_accumulate(rwr):
    exe = os.path.abspath(os.path.join(os.path.dirname(rwr.LIB_PATH), "..", "bin", "rwr_render"))
    if not os.path.exists(exe):
        rwr.build()
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--accumulate" in r.stdout
