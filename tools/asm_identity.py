#!/usr/bin/env python3
"""Compare the device code of two builds of one kernel file, kernel by kernel, as text.

usage: tools/asm_identity.py PARENT.s CHANGE.s [--rename OLD=NEW ...] [--skip REGEX] [--diff-summary] [--cxxfilt PATH]   (ROCm's llvm-cxxfilt, else c++filt)

The inputs are listings of `hipcc --offload-arch=gfx950 --cuda-device-only -S` with the Makefile's HIPFLAGS (tools/isa_stats.sh).
A kernel is every function with an .amdhsa_kernel block; its text runs from its .type line to the end of its `; Kernel info`
comments: instructions, the kernel descriptor and the resource comments.  Kernels are paired by demangled name, after --rename has
replaced OLD by NEW in the parent's names (a type of the signature that the change renamed); kernels whose demangled name matches --skip
are left out on both sides and counted (forms that are meant to change, such as the GLOW forms: ", true>\(").  Normalised before the comparison, since
another function earlier in the file shifts them: the kernel's own symbol, the block labels (.LBB<n>_, BB<n>_ in loop comments),
the .Lfunc_begin / .Lfunc_end ordinals and the column at which a trailing comment starts.  Nothing else is touched.

Prints the totals - only in parent, only in change, identical, differing - and per differing kernel the instruction count, the
descriptor's next_free_vgpr / next_free_sgpr / private_segment_fixed_size, the occupancy of the `; Occupancy:` comment and the spill
counts of the code object's metadata, parent -> change.  Exit status 1 when a kernel exists on one side only."""
import argparse
import os
import re
import shutil
import subprocess
import sys

TYPE = re.compile(r"^\t\.type\t(\S+),@function")
INSTRUCTION = re.compile(r"^\t[a-z][a-z0-9]*_[a-z0-9_]+(\s|$)")


def kernels(path):
    """{symbol: raw text} of every kernel of the listing, and {symbol: (sgpr_spill_count, vgpr_spill_count)} of its metadata."""
    lines = open(path).read().split("\n")
    starts = [(i, TYPE.match(l).group(1)) for i, l in enumerate(lines) if TYPE.match(l)]
    out = {}
    for n, (i, sym) in enumerate(starts):
        end = starts[n + 1][0] if n + 1 < len(starts) else len(lines)
        body = lines[i:end]
        if not any(l.startswith("\t.amdhsa_kernel ") for l in body):
            continue
        info = next((k for k, l in enumerate(body) if l.startswith("; Kernel info:")), None)
        if info is not None:   # ends with the resource comments; what follows is the next function's preamble
            k = info
            while k < len(body) and body[k].startswith(";"):
                k += 1
            body = body[:k]
        out[sym] = body
    spills = {}
    text = "\n".join(lines)
    at = text.find("amdhsa.kernels:")
    if at >= 0:
        for blk in text[at:].split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            spills[name] = tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in ("sgpr_spill_count", "vgpr_spill_count"))
    return out, spills


def normalise(sym, body):
    text = "\n".join(body).replace(sym, "<kernel>")
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    text = re.sub(r"\bBB\d+_", "BB_", text)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    return re.sub(r"[ \t]+;", " ;", text)


def figures(body):
    def field(pat):
        for l in body:
            m = re.search(pat, l)
            if m:
                return int(m.group(1))
        return -1
    return {"instructions": sum(1 for l in body if INSTRUCTION.match(l)),
            "vgpr": field(r"\.amdhsa_next_free_vgpr (\d+)"), "sgpr": field(r"\.amdhsa_next_free_sgpr (\d+)"),
            "scratch": field(r"\.amdhsa_private_segment_fixed_size (\d+)"), "occupancy": field(r"^; Occupancy: (\d+)")}


def demangle(symbols, cxxfilt):
    if not symbols:
        return {}
    r = subprocess.run([cxxfilt], input="\n".join(symbols) + "\n", capture_output=True, text=True, check=True)
    return dict(zip(symbols, r.stdout.split("\n")))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("change")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    llvm = "/opt/rocm/llvm/bin/llvm-cxxfilt"
    ap.add_argument("--cxxfilt", default=llvm if os.path.exists(llvm) else shutil.which("c++filt"))
    ap.add_argument("--skip", metavar="REGEX", help="leave out the kernels whose demangled name matches, on both sides")
    ap.add_argument("--diff-summary", action="store_true", help="print which lines the differing kernels differ in, as a histogram; kernels only in change by template, differing kernels by name only where a figure moved")
    a = ap.parse_args()
    renames = [r.split("=", 1) for r in a.rename]
    sides, skipped = [], [0, 0]
    for path, is_parent in ((a.parent, True), (a.change, False)):
        ks, spills = kernels(path)
        names = demangle(sorted(ks), a.cxxfilt)
        by_name = {}
        for sym, body in ks.items():
            name = names[sym]
            if a.skip and re.search(a.skip, name):
                skipped[0 if is_parent else 1] += 1
                continue
            if is_parent:
                for old, new in renames:
                    name = name.replace(old, new)
            assert name not in by_name, name
            by_name[name] = (normalise(sym, body), figures(body), spills.get(sym, (-1, -1)))
        sides.append(by_name)
    parent, change = sides
    only_parent, only_change = sorted(set(parent) - set(change)), sorted(set(change) - set(parent))
    both = sorted(set(parent) & set(change))
    differing = [n for n in both if parent[n][0] != change[n][0]]
    lines = sum(parent[n][1]["instructions"] for n in both)
    print(f"{a.parent} -> {a.change}: parent {len(parent)} kernels, change {len(change)} kernels, {lines} instruction lines compared; "
          f"only in parent {len(only_parent)}, only in change {len(only_change)}, identical {len(both) - len(differing)}, differing {len(differing)}")
    if a.skip:
        print(f"  left out by --skip '{a.skip}': {skipped[0]} of the parent's kernels, {skipped[1]} of the change's")
    for n in only_parent:
        print("  only in parent: " + n)
    if a.diff_summary and only_change:   # (by template: a summary names no kernel that has no counterpart to differ from)
        by_template = {}
        for n in only_change:
            t = n.split("<")[0]
            by_template[t] = by_template.get(t, 0) + 1
        print("  only in change: " + ", ".join(f"{k} {t}" for t, k in sorted(by_template.items())))
    else:
        for n in only_change:
            print("  only in change: " + n)
    if a.diff_summary and differing:
        # what the differing kernels differ in, line by line: every (parent line -> change line) pair with the scalar register
        # numbers taken out, and in how many kernels it occurs; a kernel whose texts do not pair up line by line is named
        pairs, unpaired = {}, []
        for n in differing:
            pl, cl = parent[n][0].split("\n"), change[n][0].split("\n")
            if len(pl) != len(cl):
                unpaired.append(n)
                continue
            seen = set()
            for x, y in zip(pl, cl):
                if x != y:
                    seen.add((re.sub(r"\bs\d+\b", "sN", x.strip()), re.sub(r"\bs\d+\b", "sN", y.strip())))
            for k in seen:
                pairs[k] = pairs.get(k, 0) + 1
        print(f"  line pairs the {len(differing) - len(unpaired)} differing kernels of equal length differ in (kernels: parent line -> change line):")
        for (x, y), k in sorted(pairs.items(), key=lambda kv: (-kv[1], kv[0])):
            print(f"    {k:4d}: {x}  ->  {y}")
        for n in unpaired:
            print("  differs in length: " + n)
    same_figures = [n for n in differing if parent[n][1:] == change[n][1:]]
    if a.diff_summary and same_figures:   # (... and only the differing kernels whose figures moved, below)
        print(f"  {len(same_figures)} of the {len(differing)} differing kernels: instructions, vgpr, sgpr, scratch, occupancy and spill counts unchanged")
        differing = [n for n in differing if n not in set(same_figures)]
    for n in differing:
        p, c = parent[n], change[n]
        cols = "  ".join(f"{k} {p[1][k]}->{c[1][k]}" for k in ("instructions", "vgpr", "sgpr", "scratch", "occupancy"))
        print(f"  differs: {n}\n           {cols}  sgpr_spills {p[2][0]}->{c[2][0]}  vgpr_spills {p[2][1]}->{c[2][1]}")
    return 1 if only_parent or only_change else 0


if __name__ == "__main__":
    sys.exit(main())
