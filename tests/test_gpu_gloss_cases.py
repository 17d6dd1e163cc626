"""Glossy surfaces taken with the other path extensions, on the GPU: tests/gloss_cases.py's list (96 stratified random cases, 64 of
them with RWR_FLAG_GLOSSY, and 12 directed ones) against the tests' CPU reference, gloss_ref.c - every case on a context of its
own, with AUX outputs:
  * sample-0 planes (object id, distance, depth) bit-exact, the bounce-ray, shadow-ray, occluded, glass event and glossy-ray counts
    equal, RGBA8 within one code, colour within the bar tests/test_gpu_multi_bounce.py holds deeper paths to (scaled by the sky's
    largest component as tests/test_gpu_sky.py scales it), the worst error printed per block; every frame in flight the same bytes
    and counts;
  * the same bytes and counts under the forced-packet schedule of tests/test_gpu_fuzz.py (the first and the last case of every block,
    every directed case) and with the wide per-lane kernel asked for (one block);
  * accumulated frames are one frame of all samples, strips of two ranks assemble the frame, glossy-ray counts included;
  * with glossy surfaces set and the flag off, the frame of a context on which no gloss setter was ever called.
tests/test_gloss_cases_host.py asserts with the reference alone that the list exercises all this.  The counts are the list's."""
import re

import numpy as np
import pytest

import gloss_cases as sc
import gloss_ref
import path_cases as pc

pytestmark = pytest.mark.gpu
BLOCK = 8
_default = {}     # case index -> the default context's frame (never modified)


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return gloss_ref.lib(tmp_path_factory)


@pytest.fixture(scope="module")
def cases(ref_loader, orc, cube, suzanne):
    return [sc.gloss_case(q, ref_loader, orc, cube, suzanne) for q in range(sc.N_GLOSS_CASES)]


def _frame(rwr, c):
    if c["index"] not in _default:
        _default[c["index"]] = sc.gpu_frame(rwr, c)
    return _default[c["index"]]


def _forced(rwr, c, **kw):
    with pc.environment(pc.FORCED_SCHEDULE):
        return sc.gpu_frame(rwr, c, **kw)


def _compare(got, sref, orc, c) -> tuple:
    """(the colour error the case is held by, the bar): against the plain reference, or for a case of ROUNDED_THROUGHPUT against
    the one that rounds the throughput, every integer against the plain one."""
    if c.get("q", c["index"]) in sc.ROUNDED_THROUGHPUT:
        err, against_plain = sc.compare_rounded(got, sref, orc, c)
        print(f"gloss case {c['index']}: colour error {against_plain:.3g} against the plain reference, {err:.3g} against the one that rounds the throughput "
              f"to unorm16 ({err / pc.color_bar(c):.2f} of its bar, {pc.color_bar(c):.3g})")
        return err, pc.color_bar(c)
    return sc.compare(got, sc.reference(sref, orc, c), c), pc.color_bar(c)


@pytest.mark.parametrize("block", range(sc.N_GLOSS_CASES // BLOCK))
def test_block_matches_the_reference(rwr, orc, sref, cases, block):
    worst, worst_ratio, at, glossy, events = 0.0, 0.0, None, 0, np.zeros(3, np.int64)
    for c in cases[BLOCK * block:BLOCK * (block + 1)]:
        got = _frame(rwr, c)
        err, bar = _compare(got, sref, orc, c)
        glossy += got["glossy"]
        events += np.asarray(got["glass"])
        if err / bar >= worst_ratio:
            worst, worst_ratio, at = err, err / bar, c["q"]
        if c["q"] % BLOCK in sc.FORCED:
            sc.same(_forced(rwr, c), got, c, "forced packets, groups of 5")
        if not c["gloss"]:      # gloss set, the flag off: the bytes of a context that never heard of gloss
            sc.same(sc.gpu_frame(rwr, c, gloss=False), got, c, "no gloss setter ever called")
    print(f"gloss cases {BLOCK * block}-{BLOCK * block + BLOCK - 1}: worst colour error {worst:.3g} (case {at}, {worst_ratio:.2f} of its bar; the bar is "
          f"{pc.COLOR_TOL:.3g} times the sky's largest component above 1); glossy rays {glossy}, glass events {tuple(events.tolist())}")


@pytest.mark.parametrize("name", list(sc.DIRECTED))
def test_directed_case_matches_the_reference(rwr, orc, sref, ref_loader, cube, suzanne, name):
    c = sc.directed(name, ref_loader, orc, cube, suzanne)
    got = _frame(rwr, c)
    err, bar = _compare(got, sref, orc, c)
    print(f"gloss case {name}: colour error {err:.3g} ({err / bar:.2f} of its bar, {bar:.3g}); glossy rays {got['glossy']}, glass events {got['glass']}")
    sc.same(_forced(rwr, c), got, c, "forced packets, groups of 5")
    if name == "rough_one":     # rho = 1 sends the diffuse ray: the bounce rays of the same case with the flag off, one for one
        off = sc.gpu_frame(rwr, c, flag=False)
        assert off["glossy"] == 0 and got["glossy"] > 0 and off["stats"] == got["stats"], (off["stats"], got["stats"])
        assert off["color_f32"].tobytes() != got["color_f32"].tobytes()


@pytest.mark.parametrize("q", [q for q in sc.ROUNDED_THROUGHPUT if isinstance(q, int) and q >= sc.N_GLOSS_CASES])
def test_walk_case_against_the_rounded_reference(rwr, orc, sref, ref_loader, cube, suzanne, q):
    """The cases of the walk that tests/glass_cases.py's walk met before: gloss case q lies on glass case 64 + q, and where the
    glossy draw leaves the glass cube of a high index at B = 8 as it was (1081 on 1145: ior 4, tint (1, 1, 0.9989), local terms up
    to 9.9) the ray record's unorm16 throughput is the same whole bar away from the plain reference's f32 one.  Every integer,
    the glossy-ray count among them, equals the plain reference's; against the reference that rounds as the record does the frame
    is held to the unchanged bar; the error against the plain one is printed."""
    c = sc.gloss_case(q, ref_loader, orc, cube, suzanne)
    assert c["glass"] and c["glass_parts"] and c["bounces"] == 8
    _compare(sc.gpu_frame(rwr, c), sref, orc, c)


_LAUNCHES = re.compile(r"rwr wavefront launches: packet (\d+), per-lane (\d+), per-lane wide (\d+)")


def test_block_with_the_wide_per_lane_kernel(rwr, cases, capfd):
    """The block with the wide per-lane kernel asked for, and again with every pool left to the per-lane kernels: the same bytes
    and counts.  That the wide kernel did run is read from the contexts' own account (RWR_WF_STATS=1, printed when one is
    destroyed): per-lane launches wherever there are bounce rays in the second pass, and wide launches in the block."""
    n_wide = 0
    for c in cases[BLOCK * sc.WIDE_LANE_BLOCK:BLOCK * (sc.WIDE_LANE_BLOCK + 1)]:
        with pc.environment({"RWR_WF_WIDE_LANE": "1"}):
            wide = sc.gpu_frame(rwr, c)
        sc.same(wide, _frame(rwr, c), c, "wide per-lane kernel")
        capfd.readouterr()
        with pc.environment(sc.WIDE_LANE_ALONE):
            alone = sc.gpu_frame(rwr, c)
        sc.same(alone, _frame(rwr, c), c, "per-lane kernels alone, the wide one asked for")
        m = _LAUNCHES.search(capfd.readouterr().err)
        assert m, sc.describe(c)
        packet, lane, wide_launches = map(int, m.groups())
        with capfd.disabled():
            print(f"gloss case {c['q']} per-lane alone: launches packet {packet} / per-lane {lane} / wide {wide_launches}, glossy rays {alone['glossy']}")
        assert (lane + wide_launches > 0) == (alone["stats"][1] > 0), (packet, lane, wide_launches, sc.describe(c))
        n_wide += wide_launches
    assert n_wide > 0


def test_accumulated_frames_are_one_frame_of_all_samples(rwr, cases):
    for c in (cases[q] for q in sc.ACCUMULATION):
        full = _frame(rwr, c)
        acc = sc.accumulated_frame(rwr, c)
        sc.same(acc, full, c, "%d x %d spp accumulated" % pc.accumulation_steps(c), stats=False)
        assert acc["glass"] == full["glass"] and acc["glossy"] == full["glossy"] > 0, (acc["glossy"], full["glossy"], sc.describe(c))     # the K frames', summed


def test_strips_of_two_ranks_assemble_the_frame(rwr, cases):
    for c in (cases[q] for q in sc.SPLITS):
        full = _frame(rwr, c)
        asm, gathered = sc.strips_frame(rwr, c)
        sc.same(asm, full, c, "strips of 2 ranks")
        assert asm["glossy"] > 0 and np.array_equal(gathered, full["color"]), sc.describe(c)
