#!/usr/bin/env python3
"""The GLOW forms of the wavefront kernels in two builds, from the compiler's own remarks: what the run-time switch for light sampling
(RWR_FLAG_LIGHT_SAMPLING; rwr_surface.h WfGlow::light) costs the forms that carry it.

usage: tools/light_resources.py [--all] --parent REMARKS.txt... --change REMARKS.txt...   (the stderr of `hipcc --offload-arch=gfx950
       --cuda-device-only -S -Rpass-analysis=kernel-resource-usage` with the Makefile's flags, of kernels_wf_primary.hip and
       kernels_wf_bounce.hip at the parent commit and at this one; of kernels_wf_light.hip at this one)

Per GLOW form (last template argument true) of k_wf_primary, k_wf_trace_lane and k_wf_trace_packet one line: VGPRs (v), SGPRs (s),
scratch bytes per lane (scr), waves per SIMD (occ), spilled SGPRs / VGPRs (spill), then the parent's.  A line starts with SPILL when
the form spills vector registers or holds scratch where the parent's holds none, with MORE when it holds more scratch than a parent
that holds some already, with OCC when it runs at a lower occupancy, else with OK; the OK lines are printed with --all only.  Then
per tag the number of forms, per kernel the ranges of the figures and of their differences, and every form of k_wf_light.  Exit
status 1 on any SPILL or OCC."""
import re
import sys

from glow_resources import kernels
import shutil
import subprocess


def named(paths):
    ks = {}
    for p in paths:
        ks.update(kernels(p))
    cxxfilt = "/opt/rocm/llvm/bin/llvm-cxxfilt" if shutil.which("/opt/rocm/llvm/bin/llvm-cxxfilt") else shutil.which("c++filt")
    syms = sorted(ks)
    names = subprocess.run([cxxfilt], input="\n".join(syms) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for sym, name in zip(syms, names):
        m = re.match(r"void rwr::(k_wf_primary|k_wf_trace_lane|k_wf_trace_packet|k_wf_light)<(.*)>\(", name)
        if m:
            out[(m.group(1), m.group(2))] = ks[sym]
    return out


def main():
    args = [x for x in sys.argv[1:] if x != "--all"]
    at_p, at_c = args.index("--parent"), args.index("--change")
    parent, change = named(args[at_p + 1:at_c]), named(args[at_c + 1:])
    fmt = lambda r: f"v {r['v']} s {r['s']} scr {r['scr']} occ {r['occ']} spill {r['sspill']}/{r['vspill']}"
    bad = 0
    counts, rows = {}, {}
    for (kernel, targs), r in sorted(change.items()):
        if kernel == "k_wf_light" or not targs.endswith(", true"):
            continue
        was = parent[(kernel, targs)]
        tag = "OK   "
        if (r["vspill"] > 0 and was["vspill"] == 0) or (r["scr"] > 0 and was["scr"] == 0):
            tag, bad = "SPILL", bad + 1
        elif r["occ"] < was["occ"]:
            tag, bad = "OCC  ", bad + 1
        elif r["scr"] > was["scr"]:
            tag = "MORE "
        counts[(kernel, tag.strip())] = counts.get((kernel, tag.strip()), 0) + 1
        if tag != "OK   " or "--all" in sys.argv:
            print(f"{tag} {kernel}<{targs}>: {fmt(r)} | parent: {fmt(was)}")
        rows.setdefault(kernel, []).append((r, was))
    for (kernel, tag), n in sorted(counts.items()):
        print(f"# {kernel}: {n} GLOW forms {tag}")
    for kernel, rt in sorted(rows.items()):
        span = lambda f: f"{min(f(r, t) for r, t in rt)}..{max(f(r, t) for r, t in rt)}"
        print(f"# {kernel}: GLOW v {span(lambda r, t: r['v'])}, v - parent's {span(lambda r, t: r['v'] - t['v'])}, scr - parent's "
              f"{span(lambda r, t: r['scr'] - t['scr'])}, occ {span(lambda r, t: r['occ'])}, occ - parent's {span(lambda r, t: r['occ'] - t['occ'])}, "
              f"spilled VGPRs {span(lambda r, t: r['vspill'])}, - parent's {span(lambda r, t: r['vspill'] - t['vspill'])}")
    for (kernel, targs), r in sorted(change.items()):
        if kernel == "k_wf_light":
            print(f"# k_wf_light<{targs}>: {fmt(r)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
