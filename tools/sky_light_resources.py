#!/usr/bin/env python3
"""RWR_FLAG_LIGHT_SKY's kernel forms beside their twins, from the compiler's own remarks.

usage: tools/sky_light_resources.py BEFORE_DIR AFTER_DIR   (each holds the stderr of `hipcc --offload-arch=gfx950 --cuda-device-only
       -S -Rpass-analysis=kernel-resource-usage` with the Makefile's flags: kernels_wf_light.txt and kernels_wf_bounce.txt; the
       parsing is tools/glow_resources.py's)

k_wf_light: each of the parent's 8 forms -> the same form of this build (`same` when no figure moved), then each SKY form beside the
form without SKY it is a twin of.  Trace kernels: every form that existed beside the parent's (counted; printed only when a figure
moved), then each LSKY form (the silencing of marked misses: forms of their own of the IMG x GLOW forms) beside its twin without it.
Figures: VGPRs (v), SGPRs (s), scratch bytes per lane (scr), waves per SIMD (occ), spilled SGPRs / VGPRs.  A line starts with OCC when
the form runs at fewer waves per SIMD than the form beside it, SCR when it holds more scratch, else ok.  Exit status 1 when a form
that existed before moved."""
import os
import re
import shutil
import subprocess
import sys

from glow_resources import kernels


def named(path):
    ks = kernels(path)
    cxxfilt = "/opt/rocm/llvm/bin/llvm-cxxfilt" if shutil.which("/opt/rocm/llvm/bin/llvm-cxxfilt") else shutil.which("c++filt")
    syms = sorted(ks)
    names = subprocess.run([cxxfilt], input="\n".join(syms) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return {n.split("(")[0]: ks[s] for s, n in zip(syms, names)}


def main():
    before_dir, after_dir = sys.argv[1:3]
    fmt = lambda r: f"v {r['v']} s {r['s']} scr {r['scr']} occ {r['occ']} spill {r['sspill']}/{r['vspill']}"
    tag = lambda b, a: "same" if a == b else "OCC" if a["occ"] < b["occ"] else "SCR" if a["scr"] > b["scr"] else "ok"
    moved = 0
    for unit, pattern in (("kernels_wf_light", r"(k_wf_light<[^>]*)>"), ("kernels_wf_bounce", r"(k_wf_trace_(?:lane|packet)<[^>]*)>")):
        before = {re.sub(pattern, r"\1, false>", n): r for n, r in named(os.path.join(before_dir, unit + ".txt")).items()}
        after = named(os.path.join(after_dir, unit + ".txt"))
        assert set(before) <= set(after), sorted(set(before) - set(after))[:4]
        counts = {}
        for name in sorted(before):
            t = tag(before[name], after[name])
            counts[t] = counts.get(t, 0) + 1
            moved += t != "same"
            if unit == "kernels_wf_light" or t != "same":
                print(f"{t:4} {name}: {fmt(before[name])} -> {fmt(after[name])}")
        new = sorted(set(after) - set(before))
        fewer = more = 0
        for name in new:
            twin = re.sub(r", true>$", ", false>", name)
            assert twin in after, name
            t = tag(after[twin], after[name])
            fewer += t == "OCC"
            more += after[name]["scr"] > after[twin]["scr"]
            print(f"{'SKY ' if unit == 'kernels_wf_light' else 'LSKY'} {t:4} {name}: {fmt(after[twin])} -> {fmt(after[name])}")
        print(f"# {unit}: {len(before)} forms that existed before: {counts}; {len(new)} new forms: {fewer} a wave per SIMD below their twin, "
              f"{more} with more scratch than it")
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
