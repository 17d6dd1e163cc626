"""Glass taken with the other path extensions, on the GPU: tests/glass_cases.py's list (64 stratified random cases, 48 of them with
RWR_FLAG_GLASS, and 10 directed ones) against the tests' CPU reference, glass_ref.c - every case on a context of its own, with AUX
outputs:
  * sample-0 planes (object id, distance, depth) bit-exact, the ray and shadow-ray counts and the three glass event counts equal,
    RGBA8 within one code, colour within the bar tests/test_gpu_multi_bounce.py holds deeper paths to (scaled by the sky's largest
    component as tests/test_gpu_sky.py scales it), the worst error printed per block; every frame in flight the same bytes and
    counts;
  * the same bytes and counts under the forced-packet schedule of tests/test_gpu_fuzz.py (every eighth case, every directed case)
    and with the wide per-lane kernel asked for (one block);
  * accumulated frames are one frame of all samples, strips of two ranks assemble the frame, event counts included;
  * with glass surfaces set and the flag off, the frame of a context on which no glass setter was ever called.
tests/test_glass_cases_host.py asserts with the reference alone that the list exercises all this.  The counts are the list's."""
import re

import numpy as np
import pytest

import glass_cases as gc
import glass_ref
import path_cases as pc

pytestmark = pytest.mark.gpu
BLOCK = 8
_default = {}     # case index -> the default context's frame (never modified)


@pytest.fixture(scope="module")
def gref(tmp_path_factory):
    return glass_ref.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def cases(ref_loader, orc, cube, suzanne):
    return [gc.glass_case(g, ref_loader, orc, cube, suzanne) for g in range(gc.N_GLASS_CASES)]


def _frame(rwr, c):
    if c["index"] not in _default:
        _default[c["index"]] = gc.gpu_frame(rwr, c)
    return _default[c["index"]]


def _forced(rwr, c):
    with pc.environment(pc.FORCED_SCHEDULE):
        return gc.gpu_frame(rwr, c)


@pytest.mark.parametrize("block", range(gc.N_GLASS_CASES // BLOCK))
def test_block_matches_the_reference(rwr, orc, gref, cases, block):
    worst, worst_ratio, at, events = 0.0, 0.0, None, np.zeros(3, np.int64)
    for c in cases[BLOCK * block:BLOCK * (block + 1)]:
        got = _frame(rwr, c)
        err = gc.compare(got, gc.reference(gref, orc, c), c)
        events += np.asarray(got["glass"])
        if err / pc.color_bar(c) >= worst_ratio:
            worst, worst_ratio, at = err, err / pc.color_bar(c), c["g"]
        if c["g"] % BLOCK == 0:
            gc.same(_forced(rwr, c), got, c, "forced packets, groups of 5")
        if not c["glass"]:      # glass set, the flag off: the bytes of a context that never heard of glass
            gc.same(gc.gpu_frame(rwr, c, glass=False), got, c, "no glass setter ever called")
    print(f"glass cases {BLOCK * block}-{BLOCK * block + BLOCK - 1}: worst colour error {worst:.3g} (case {at}, {worst_ratio:.2f} of its bar; the bar is "
          f"{pc.COLOR_TOL:.3g} times the sky's largest component above 1); glass events {tuple(events.tolist())}")


@pytest.mark.parametrize("name", list(gc.DIRECTED))
def test_directed_case_matches_the_reference(rwr, orc, gref, ref_loader, cube, suzanne, name):
    c = gc.directed(name, ref_loader, orc, cube, suzanne)
    got = _frame(rwr, c)
    err = gc.compare(got, gc.reference(gref, orc, c), c)
    print(f"glass case {name}: colour error {err:.3g} ({err / pc.color_bar(c):.2f} of its bar, {pc.color_bar(c):.3g}); glass events {got['glass']}")
    gc.same(_forced(rwr, c), got, c, "forced packets, groups of 5")


@pytest.mark.parametrize("g", gc.ROUNDED_THROUGHPUT)
def test_walk_case_against_the_rounded_reference(rwr, orc, gref, ref_loader, cube, suzanne, g):
    """Cases 1145 and 7953 of the walk: the cube as glass of ior 4 and tint (1, 1, 0.9989), and of ior 2.4 and tint (0.49, 0.99981,
    0.37), at B = 8, local terms up to 9.9 and 7.3.  Every integer equals the plain reference's.  The product's ray record carries
    the throughput as unorm16; the plain reference carries it in f32, and the two references differ from each other by 1.03e-4 and
    1.56e-4 here.  Against the reference that rounds as the record does the frame is held to the unchanged bar; the error against
    the plain one is printed."""
    c = gc.glass_case(g, ref_loader, orc, cube, suzanne)
    got = gc.gpu_frame(rwr, c)
    err, against_plain = gc.compare_rounded(got, gref, orc, c)
    print(f"glass case {g}: colour error {against_plain:.3g} against the plain reference, {err:.3g} against the one that rounds the throughput to unorm16 "
          f"({err / pc.color_bar(c):.2f} of its bar, {pc.color_bar(c):.3g})")


_LAUNCHES = re.compile(r"rwr wavefront launches: packet (\d+), per-lane (\d+), per-lane wide (\d+)")


def test_block_with_the_wide_per_lane_kernel(rwr, cases, capfd):
    """The block with the wide per-lane kernel asked for, and again with every pool left to the per-lane kernels: the same bytes
    and counts.  That the wide kernel did run is read from the contexts' own account (RWR_WF_STATS=1, printed when one is
    destroyed): per-lane launches wherever there are bounce rays in the second pass, and wide launches in the block."""
    n_wide = 0
    for c in cases[BLOCK * gc.WIDE_LANE_BLOCK:BLOCK * (gc.WIDE_LANE_BLOCK + 1)]:
        with pc.environment({"RWR_WF_WIDE_LANE": "1"}):
            wide = gc.gpu_frame(rwr, c)
        gc.same(wide, _frame(rwr, c), c, "wide per-lane kernel")
        capfd.readouterr()
        with pc.environment(gc.WIDE_LANE_ALONE):
            alone = gc.gpu_frame(rwr, c)
        gc.same(alone, _frame(rwr, c), c, "per-lane kernels alone, the wide one asked for")
        m = _LAUNCHES.search(capfd.readouterr().err)
        assert m, gc.describe(c)
        packet, lane, wide_launches = map(int, m.groups())
        with capfd.disabled():
            print(f"glass case {c['g']} per-lane alone: launches packet {packet} / per-lane {lane} / wide {wide_launches}")
        assert (lane + wide_launches > 0) == (alone["stats"][1] > 0), (packet, lane, wide_launches, gc.describe(c))
        n_wide += wide_launches
    assert n_wide > 0


def test_accumulated_frames_are_one_frame_of_all_samples(rwr, cases):
    for c in (cases[g] for g in gc.ACCUMULATION):
        full = _frame(rwr, c)
        acc = gc.accumulated_frame(rwr, c)
        gc.same(acc, full, c, "%d x %d spp accumulated" % pc.accumulation_steps(c), stats=False)
        assert acc["glass"] == full["glass"], (acc["glass"], full["glass"], gc.describe(c))       # the K frames' events, summed


def test_strips_of_two_ranks_assemble_the_frame(rwr, cases):
    for c in (cases[g] for g in gc.SPLITS):
        full = _frame(rwr, c)
        asm, gathered = gc.strips_frame(rwr, c)
        gc.same(asm, full, c, "strips of 2 ranks")
        assert np.array_equal(gathered, full["color"]), gc.describe(c)
