"""The path tracer's extensions taken together, on the GPU: tests/path_cases.py's list (64 stratified random cases, 8 directed
ones) against the tests' CPU reference, mirror_ref.c - every case on a context of its own, with AUX outputs:
  * sample-0 planes (object id, distance, depth) bit-exact, the ray and shadow-ray counts equal, RGBA8 within one code, colour
    within the bar tests/test_gpu_multi_bounce.py holds deeper paths to (scaled by the sky's largest component as
    tests/test_gpu_sky.py scales it), the worst error printed per block;
  * the same bytes under the forced-packet schedule of tests/test_gpu_fuzz.py (every eighth case, every directed case) and with
    the wide per-lane kernel asked for (one block);
  * accumulated frames are one frame of all samples, strips of two ranks assemble the frame - on rotated instances and mirrors.
tests/test_path_cases_host.py asserts with the reference alone that the list exercises all this.  The counts are the list's."""
import numpy as np
import pytest

import mirror_ref
import path_cases as pc

pytestmark = pytest.mark.gpu
BLOCK = 8
_default = {}     # case index -> the default context's frame (never modified)


@pytest.fixture(scope="module")
def mref(tmp_path_factory):
    return mirror_ref.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def cases(ref_loader, orc, cube, suzanne):
    return [pc.case(i, ref_loader, orc, cube, suzanne) for i in range(pc.N_CASES)]


def _frame(rwr, c):
    if c["index"] not in _default:
        _default[c["index"]] = pc.gpu_frame(rwr, c)
    return _default[c["index"]]


def _forced(rwr, c):
    with pc.environment(pc.FORCED_SCHEDULE):
        return pc.gpu_frame(rwr, c)


@pytest.mark.parametrize("block", range(pc.N_CASES // BLOCK))
def test_block_matches_the_reference(rwr, orc, mref, cases, block):
    worst, worst_ratio, at = 0.0, 0.0, None
    for c in cases[BLOCK * block:BLOCK * (block + 1)]:
        got = _frame(rwr, c)
        err = pc.compare(got, pc.reference(mref, orc, c), c)
        if err / pc.color_bar(c) >= worst_ratio:
            worst, worst_ratio, at = err, err / pc.color_bar(c), c["index"]
        if c["index"] % BLOCK == 0:
            pc.same(_forced(rwr, c), got, c, "forced packets, groups of 5")
    print(f"path cases {BLOCK * block}-{BLOCK * block + BLOCK - 1}: worst colour error {worst:.3g} (case {at}, {worst_ratio:.2f} of its bar; the bar is {pc.COLOR_TOL:.3g} "
          f"times the sky's largest component above 1)")


@pytest.mark.parametrize("name", list(pc.DIRECTED))
def test_directed_case_matches_the_reference(rwr, orc, mref, ref_loader, cube, suzanne, name):
    c = pc.directed(name, ref_loader, orc, cube, suzanne)
    got = _frame(rwr, c)
    err = pc.compare(got, pc.reference(mref, orc, c), c)
    print(f"path case {name}: colour error {err:.3g} (bar {pc.color_bar(c):.3g})")
    pc.same(_forced(rwr, c), got, c, "forced packets, groups of 5")


def test_block_with_the_wide_per_lane_kernel(rwr, cases):
    for c in cases[3 * BLOCK:4 * BLOCK]:
        with pc.environment({"RWR_WF_WIDE_LANE": "1"}):
            wide = pc.gpu_frame(rwr, c)
        pc.same(wide, _frame(rwr, c), c, "wide per-lane kernel")


def test_accumulated_frames_are_one_frame_of_all_samples(rwr, cases):
    for c in (cases[i] for i in pc.ACCUMULATION):
        pc.same(pc.accumulated_frame(rwr, c), _frame(rwr, c), c, "%d x %d spp accumulated" % pc.accumulation_steps(c), stats=False)


def test_strips_of_two_ranks_assemble_the_frame(rwr, cases):
    for c in (cases[i] for i in pc.SPLITS):
        full = _frame(rwr, c)
        asm, gathered = pc.strips_frame(rwr, c)
        pc.same(asm, full, c, "strips of 2 ranks")
        assert np.array_equal(gathered, full["color"]), pc.describe(c)
