"""Writes tests/golden/render_refusals.json: the (return code, error message) pair of every call of tests/refusals_common.py.

Run on a GPU against a build of the commit BEFORE csrc/render.cpp was split into units (its library named by RWR_HIP_LIB, the
Python package and this script from the current tree) — never against the code under test: the file is the record the split
is held to.

    RWR_HIP_LIB=<parent build>/lib/librwr_hip.so python tests/golden/make_render_refusals.py [output path]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402
import refusals_common as rc  # noqa: E402


def main():
    if not os.environ.get("RWR_HIP_LIB"):
        sys.exit("RWR_HIP_LIB must name the parent commit's library")
    rwr = graft.load_package()
    ctx = rc.make_scene(rwr)
    pairs = rc.run_sweep(rwr, ctx)
    distinct = sorted({tuple(p) for p in pairs}, key=lambda p: (p[0] != 0, p[1]))
    index = {p: i for i, p in enumerate(distinct)}
    doc = {
        "library": "the parent of the commit that split csrc/render.cpp",
        "pairs": [list(p) for p in distinct],
        "indices": [index[tuple(p)] for p in pairs],
        "arguments": rc.run_argument_cases(rwr, ctx),
        "surfaces": {e: rc.run_surface_errors(ctx, e) for e in rc.SURFACE_ENTRY_POINTS},
    }
    ctx.close()
    out = sys.argv[1] if len(sys.argv) > 1 else rc.FIXTURE
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(pairs)} calls, {len(distinct)} distinct pairs, {sum(1 for p in pairs if p[0])} refused -> {out}")


if __name__ == "__main__":
    main()
