"""The surface forms' frames against a record of the library as it was before the surface table's decode, fetch and event counters
moved into csrc/rwr_surface.h (tests/golden/surface_frames.json, written by tests/golden/make_surface_frames.py from a build of that
commit; never regenerated from the code under test).  The frames are tests/surface_frames_common.py's: both pool classes, the three
sets of surface flags with and without shadows and sky, a normal-mapped one and one with the auxiliary planes; each must give the
recorded SHA-256 of every plane and the recorded event counters.

The record itself is checked without a GPU, so that the comparison cannot pass by covering nothing."""
import json

import pytest

import surface_frames_common as sf


@pytest.fixture(scope="module")
def record():
    with open(sf.FIXTURE) as f:
        return json.load(f)["frames"]


@pytest.fixture(scope="module")
def contexts(rwr):
    """One context per scene, schedule and part 0 (context_key), made by the first frame that needs it."""
    ctxs = {}
    yield lambda key: ctxs.get(key) or ctxs.setdefault(key, sf.make_ctx(rwr, key))
    for ctx in ctxs.values():
        ctx.close()


def test_record_covers_the_list(record):
    frames = sf.frames()
    assert len(frames) == 42 and sorted(record) == sorted(f["name"] for f in frames)
    for f in frames:
        r = record[f["name"]]
        assert sorted(r["planes"]) == (["color", "depth", "hit_t", "obj_id"] if f["aux"] else ["color", "depth"]), f["name"]
        assert len(r["counters"]) == len(sf.COUNTERS)
        # a frame counts only what its flags switch on
        assert ("glass" in f["surfaces"]) or r["counters"][:3] == [0, 0, 0], f["name"]
        assert ("glossy" in f["surfaces"]) or r["counters"][3] == 0, f["name"]
    for k, what in enumerate(sf.COUNTERS):
        assert any(r["counters"][k] for r in record.values()), what
    # from the side every flag changes the frame and its counters
    side = [record[f["name"]] for f in frames if f["camera"] == "side"]
    assert len(side) == 3 == len({r["planes"]["color"] for r in side}) == len({tuple(r["counters"]) for r in side})
    # the schedule changes no byte; the auxiliary planes come on top of the same frame
    for f in frames:
        if f["packets"]:
            assert record[f["name"]] == record[f["name"].replace("-packets", "")], f["name"]
    assert record["inside-aux"]["planes"]["color"] == record["inside-mirrors+glass+glossy"]["planes"]["color"]
    assert record["inside-aux"]["counters"] == record["inside-mirrors+glass+glossy"]["counters"]


@pytest.mark.gpu
@pytest.mark.parametrize("frame", sf.frames(), ids=lambda f: f["name"])
def test_frame_matches_the_record(rwr, contexts, record, frame):
    got = sf.render(rwr, contexts(sf.context_key(frame)), frame)
    assert got == record[frame["name"]]
