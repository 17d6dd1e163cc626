#!/usr/bin/env python3
"""The GLOW forms (RWR_FLAG_EMISSIVE) of the wavefront kernels beside their twins without GLOW, from the compiler's own remarks.

usage: tools/glow_resources.py [--all] REMARKS.txt...   (the stderr of `hipcc --offload-arch=gfx950 --cuda-device-only -S
       -Rpass-analysis=kernel-resource-usage` with the Makefile's flags, of kernels_wf_primary.hip and kernels_wf_bounce.hip)

GLOW is the last template argument of k_wf_primary, k_wf_trace_lane and k_wf_trace_packet; a form's twin is the kernel whose other
arguments are the same.  Per GLOW form one line: VGPRs (v), SGPRs (s), scratch bytes per lane (scr), waves per SIMD (occ), spilled
SGPRs / VGPRs (spill), then the twin's.  A line starts with SPILL when the GLOW form spills vector registers or holds scratch where
its twin holds none, with MORE when it holds more scratch than a twin that holds some already, with OCC when it runs at a lower
occupancy than its twin, else with OK; the OK lines are printed with --all only.  Then per tag the number of forms, and per kernel
the ranges of the figures and of their differences to the twins'.  Exit status 1 on any SPILL."""
import re
import shutil
import subprocess
import sys

FIELDS = (("v", "VGPRs"), ("s", "TotalSGPRs"), ("scr", r"ScratchSize \[bytes/lane\]"), ("occ", r"Occupancy \[waves/SIMD\]"),
          ("sspill", "SGPRs Spill"), ("vspill", "VGPRs Spill"))


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, pat in FIELDS:
            m = re.search(r"remark:\s+" + pat + r": (\d+)", line)
            if m:
                cur[key] = int(m.group(1))
    return out


def main():
    ks = {}
    for p in (x for x in sys.argv[1:] if x != "--all"):
        ks.update(kernels(p))
    cxxfilt = "/opt/rocm/llvm/bin/llvm-cxxfilt" if shutil.which("/opt/rocm/llvm/bin/llvm-cxxfilt") else shutil.which("c++filt")
    syms = sorted(ks)
    names = subprocess.run([cxxfilt], input="\n".join(syms) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    by_name = {}
    for sym, name in zip(syms, names):
        m = re.match(r"void rwr::(k_wf_primary|k_wf_trace_lane|k_wf_trace_packet)<(.*)>\(", name)
        if m:
            by_name[(m.group(1), m.group(2))] = ks[sym]
    fmt = lambda r: f"v {r['v']} s {r['s']} scr {r['scr']} occ {r['occ']} spill {r['sspill']}/{r['vspill']}"
    bad = 0
    counts, rows = {}, {}
    for (kernel, args), r in sorted(by_name.items()):
        if not args.endswith(", true"):
            continue
        twin = by_name[(kernel, args[:-len("true")] + "false")]
        tag = "OK   "
        if (r["vspill"] > 0 and twin["vspill"] == 0) or (r["scr"] > 0 and twin["scr"] == 0):
            tag, bad = "SPILL", bad + 1
        elif r["scr"] > twin["scr"]:
            tag = "MORE "
        elif r["occ"] < twin["occ"]:
            tag = "OCC  "
        counts[(kernel, tag.strip())] = counts.get((kernel, tag.strip()), 0) + 1
        if tag != "OK   " or "--all" in sys.argv:   # (the forms that hold their twin's scratch and occupancy: counted, and their ranges, below)
            print(f"{tag} {kernel}<{args}>: {fmt(r)} | twin: {fmt(twin)}")
        rows.setdefault(kernel, []).append((r, twin))
    for (kernel, tag), n in sorted(counts.items()):
        print(f"# {kernel}: {n} GLOW forms {tag}")
    for kernel, rt in sorted(rows.items()):
        span = lambda f: f"{min(f(r, t) for r, t in rt)}..{max(f(r, t) for r, t in rt)}"
        print(f"# {kernel}: GLOW v {span(lambda r, t: r['v'])}, v - twin's {span(lambda r, t: r['v'] - t['v'])}, scr - twin's "
              f"{span(lambda r, t: r['scr'] - t['scr'])}, occ {span(lambda r, t: r['occ'])}, occ - twin's {span(lambda r, t: r['occ'] - t['occ'])}, "
              f"spilled VGPRs {span(lambda r, t: r['vspill'])}, - twin's {span(lambda r, t: r['vspill'] - t['vspill'])}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
