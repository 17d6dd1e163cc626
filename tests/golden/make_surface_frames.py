"""Writes tests/golden/surface_frames.json: per frame of tests/surface_frames_common.py a SHA-256 of each plane and the four event
counters.

Run on a GPU against a build of the commit BEFORE the surface table's decode, fetch and counters moved into csrc/rwr_surface.h (its
library named by RWR_HIP_LIB, the Python package and this script from the current tree) - never against the code under test: the
file is the record that move is held to.

    RWR_HIP_LIB=<parent build>/lib/librwr_hip.so python tests/golden/make_surface_frames.py [output path]

Asserts while it records, so that the file cannot pin frames that exercise nothing: both pool classes occur over the set (the
contexts' own account, RWR_WF_STATS=1, in a pass of its own), every event counter is non-zero somewhere, and the frame with all
three surface flags differs - in its colour plane's hash and in its counters - from each frame of the same camera, shadows and sky
that lacks one of them."""
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402
import surface_frames_common as sf  # noqa: E402

_POOLS = re.compile(r"rwr wavefront pools: packets (\d+) pools / (\d+) rays, per-lane (\d+) pools / (\d+) rays")


def pool_classes(rwr, frame):
    """(packet pools, per-lane pools) of one frame in a context of its own with RWR_WF_STATS=1, read from what the context prints
    when it is destroyed (tools/gloss_probe.py packet_share)."""
    sys.stderr.flush()
    keep = os.dup(2)
    try:
        with tempfile.TemporaryFile() as f:
            os.dup2(f.fileno(), 2)
            try:
                ctx = sf.make_ctx(rwr, sf.context_key(frame), stats=True)
                sf.render(rwr, ctx, frame)
                ctx.close()
            finally:
                os.dup2(keep, 2)
            f.seek(0)
            m = _POOLS.search(f.read().decode("utf-8", "replace"))
    finally:
        os.close(keep)
    assert m, "the context printed no pool account"
    return int(m.group(1)), int(m.group(3))


def main():
    if not os.environ.get("RWR_HIP_LIB"):
        sys.exit("RWR_HIP_LIB must name the parent commit's library")
    os.environ.pop("RWR_WF_STATS", None)
    rwr = graft.load_package()
    frames = sf.frames()
    ctxs, record = {}, {}
    for f in frames:
        key = sf.context_key(f)
        if key not in ctxs:
            ctxs[key] = sf.make_ctx(rwr, key)
        record[f["name"]] = sf.render(rwr, ctxs[key], f)
        print(f["name"], record[f["name"]]["counters"], record[f["name"]]["planes"]["color"][:12], flush=True)
    for ctx in ctxs.values():
        ctx.close()

    pools = {f["name"]: pool_classes(rwr, f) for f in frames if f["surfaces"] == sf.SURFACE_SETS[-1] and not (f["shadows"] or f["aux"])}
    print("pools (packet, per-lane):", pools, flush=True)
    assert any(p[0] for p in pools.values()) and any(p[1] for p in pools.values()), pools
    for k, what in enumerate(sf.COUNTERS):
        assert any(r["counters"][k] for r in record.values()), f"no frame counts a {what} event"
    by_key = {(f["camera"], f["packets"], f["surfaces"], f["shadows"], f["sky"]): record[f["name"]] for f in frames if f["scene"] != "cube.obj" and not f["aux"]}
    for (camera, packets, surfaces, shadows, sky), full in by_key.items():
        if surfaces != sf.SURFACE_SETS[-1]:
            continue
        for fewer in sf.SURFACE_SETS[:-1]:
            other = by_key[(camera, packets, fewer, shadows, sky)]
            assert other["planes"]["color"] != full["planes"]["color"], (camera, packets, fewer, shadows, sky, "the same colour plane as with all flags")
            assert other["counters"] != full["counters"], (camera, packets, fewer, shadows, sky, "the same counters as with all flags")

    doc = {"library": "the parent of the commit that added csrc/rwr_surface.h", "frames": record}
    out = sys.argv[1] if len(sys.argv) > 1 else sf.FIXTURE
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(record)} frames -> {out}")


if __name__ == "__main__":
    main()
