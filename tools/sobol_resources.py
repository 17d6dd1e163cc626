#!/usr/bin/env python3
"""Every kernel form of the wavefront kernel files beside the same form of another build, from the compiler's own remarks.

usage: tools/sobol_resources.py [--all] BEFORE_DIR AFTER_DIR   (each holds the stderr of `hipcc --offload-arch=gfx950
       --cuda-device-only -S -Rpass-analysis=kernel-resource-usage` with the Makefile's flags, one *.txt per kernel file; the
       parsing is tools/glow_resources.py's)

Per form whose figures differ one line: VGPRs (v), SGPRs (s), scratch bytes per lane (scr), waves per SIMD (occ), spilled SGPRs /
VGPRs, before -> after.  A line starts with OCC when the form lost a wave per SIMD, with SCR when it holds more scratch, else with
ok; --all prints the unchanged forms too.  Then per file the counts.  Exit status 1 on any OCC or SCR."""
import glob
import os
import shutil
import subprocess
import sys

from glow_resources import kernels


def main():
    dirs = [a for a in sys.argv[1:] if a != "--all"]
    show_all = "--all" in sys.argv
    cxxfilt = "/opt/rocm/llvm/bin/llvm-cxxfilt" if shutil.which("/opt/rocm/llvm/bin/llvm-cxxfilt") else shutil.which("c++filt")
    fmt = lambda r: f"v {r['v']} s {r['s']} scr {r['scr']} occ {r['occ']} spill {r['sspill']}/{r['vspill']}"
    bad = 0
    for path in sorted(glob.glob(os.path.join(dirs[0], "*.txt"))):
        name = os.path.basename(path)
        before, after = kernels(path), kernels(os.path.join(dirs[1], name))
        syms = sorted(set(before) | set(after))
        names = subprocess.run([cxxfilt], input="\n".join(syms) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        n = {"same": 0, "ok": 0, "OCC": 0, "SCR": 0, "new": 0, "gone": 0}
        for sym, pretty in zip(syms, names):
            if sym not in before or sym not in after:
                n["new" if sym in after else "gone"] += 1
                print(f"{'new ' if sym in after else 'gone'} {pretty}: {fmt(after.get(sym) or before[sym])}")
                continue
            b, a = before[sym], after[sym]
            tag = "same" if a == b else "OCC" if a["occ"] < b["occ"] else "SCR" if a["scr"] > b["scr"] else "ok"
            n[tag] += 1
            bad += tag in ("OCC", "SCR")
            if tag != "same" or show_all:
                print(f"{tag:4} {pretty}: {fmt(b)} -> {fmt(a)}")
        print(f"# {name}: {len(syms)} forms: {n['same']} with the same figures, {n['ok']} changed at the same occupancy and no more scratch, "
              f"{n['OCC']} lost a wave per SIMD, {n['SCR']} gained scratch, {n['new']} new, {n['gone']} gone")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
