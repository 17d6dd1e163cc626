#!/usr/bin/env python3
"""Every form of the trace kernels beside the same form of the parent's build, and every IMG form (RWR_FLAG_SKY_IMAGE: forms of their
own of the SKY forms) beside the SKY form it is a twin of, from the compiler's own remarks.

usage: tools/sky_image_resources.py BEFORE_DIR AFTER_DIR   (each holds the stderr of `hipcc --offload-arch=gfx950 --cuda-device-only
       -S -Rpass-analysis=kernel-resource-usage` with the Makefile's flags, kernels_wf_bounce.txt; the parsing is
       tools/glow_resources.py's)

Forms are paired by demangled name, the parent's names given what the change added to every name (the last template argument IMG =
false, the trailing argument type rwr::WfSkyImage).  Per SKY form that existed before one line: VGPRs (v), SGPRs (s), scratch bytes
per lane (scr), waves per SIMD (occ), spilled SGPRs / VGPRs, before -> after, starting with same when no figure moved, OCC when the
form lost a wave per SIMD, SCR when it holds more scratch, else ok; the forms without SKY are counted.  Per IMG form one line
starting with IMG: its gradient twin's figures -> its own.  Exit status 1 on any OCC or SCR in a form that existed before."""
import os
import re
import shutil
import subprocess
import sys

from glow_resources import kernels

HEAD = re.compile(r"void rwr::(k_wf_trace_lane|k_wf_trace_packet)<([^>]*)>")


def args_of(name):
    m = HEAD.match(name)
    return (m.group(1), [a.strip() for a in m.group(2).split(",")]) if m else (None, [])


def is_sky(name):
    k, a = args_of(name)
    return bool(k) and a[6 if k == "k_wf_trace_lane" else 3] == "true"


def main():
    before_dir, after_dir = sys.argv[1:3]
    cxxfilt = "/opt/rocm/llvm/bin/llvm-cxxfilt" if shutil.which("/opt/rocm/llvm/bin/llvm-cxxfilt") else shutil.which("c++filt")
    fmt = lambda r: f"v {r['v']} s {r['s']} scr {r['scr']} occ {r['occ']} spill {r['sspill']}/{r['vspill']}"
    sides = []
    for d in (before_dir, after_dir):
        ks = kernels(os.path.join(d, "kernels_wf_bounce.txt"))
        syms = sorted(ks)
        names = subprocess.run([cxxfilt], input="\n".join(syms) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        sides.append({n.split("(")[0]: ks[s] for s, n in zip(syms, names)})
    before = {re.sub(r"(k_wf_trace_(?:lane|packet)<[^>]*)>", r"\1, false>", n): r for n, r in sides[0].items()}
    after = sides[1]
    assert set(before) <= set(after), sorted(set(before) - set(after))[:4]
    n = {True: {"same": 0, "ok": 0, "OCC": 0, "SCR": 0}, False: {"same": 0, "ok": 0, "OCC": 0, "SCR": 0}}
    for name in sorted(before):
        b, a = before[name], after[name]
        tag = "same" if a == b else "OCC" if a["occ"] < b["occ"] else "SCR" if a["scr"] > b["scr"] else "ok"
        sky = is_sky(name)
        n[sky][tag] += 1
        if sky or tag in ("OCC", "SCR"):
            print(f"{tag:4} {name}: {fmt(b)} -> {fmt(a)}")
    new = sorted(set(after) - set(before))
    fewer = more = 0
    for name in new:
        twin = re.sub(r", true>$", ", false>", name)
        assert twin in after and is_sky(twin), name
        fewer += after[name]["occ"] < after[twin]["occ"]
        more += after[name]["scr"] > after[twin]["scr"]
        print(f"IMG  {name}: {fmt(after[twin])} -> {fmt(after[name])}")
    for sky in (True, False):
        c = n[sky]
        print(f"# {'SKY forms that existed before' if sky else 'forms without SKY, k_wf_sort'}: {sum(c.values())}: {c['same']} with the same figures, "
              f"{c['ok']} changed at the same occupancy and no more scratch, {c['OCC']} lost a wave per SIMD, {c['SCR']} gained scratch")
    print(f"# IMG forms (new): {len(new)}: {fewer} a wave per SIMD below their gradient twin, {more} with more scratch than it")
    return 1 if any(n[s]["OCC"] or n[s]["SCR"] for s in n) else 0


if __name__ == "__main__":
    sys.exit(main())
