"""Every refusal of a render call and of the surface entry points, and which one a call with several faults gets, against a
record of the library as it was before csrc/render.cpp was split into units (tests/golden/render_refusals.json, written by
tests/golden/make_render_refusals.py from a build of that commit; never regenerated from the code under test).

The sweep (tests/refusals_common.py): one context, the cube at 64 x 16 with sphere 0 a mirror, sphere 1 glass and part 0 glossy;
4 096 calls at spp 1 — every subset of ACCUMULATE, SHADOWS, DENOISE, REPROJECT, SKY, MIRRORS, GLASS, GLOSSY x {nothing,
RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH, one single-triangle pass} x {whole frame, rows 0..8} x max_bounces {0, 1} — synchronised
every 256 calls; the pair (return code, message) of each call must be the recorded one.

The record itself is checked without a GPU, so that the comparison cannot pass by covering nothing: it holds every refusal of
validate that depends on flags, rows and bounces; it holds calls that two and more rules refuse; and every recorded pair is the
one a model of the rules' order (refusals_common.rules_refusing, written from the header) predicts."""
import json

import pytest

import refusals_common as rc


@pytest.fixture(scope="module")
def record():
    with open(rc.FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def scene(rwr):
    ctx = rc.make_scene(rwr)
    yield ctx
    ctx.close()


def test_record_covers_every_flag_refusal(record):
    assert len(record["indices"]) == 4096 == len(rc.sweep_cases())
    recorded = {msg for code, msg in record["pairs"] if code != 0}
    assert recorded == set(rc.FLAG_REFUSALS)
    used = {tuple(record["pairs"][i]) for i in record["indices"]}
    assert used == {tuple(p) for p in record["pairs"]}   # no pair that no call has
    assert (0, "") in used


def test_record_follows_the_rules_order(record, rwr):
    several = 0
    for case, i in zip(rc.sweep_cases(), record["indices"]):
        code, msg = record["pairs"][i]
        rules = rc.rules_refusing(case)
        several += len(set(rules)) >= 2
        if rules:
            assert (code, msg) == (rwr.ERR_UNSUPPORTED, rules[0]), case
        else:
            assert (code, msg) == (0, ""), case
    assert several >= 1000   # calls that two different rules would refuse: the first one's text is the recorded one


@pytest.mark.gpu
def test_render_refusals_match_the_record(rwr, scene, record):
    got = rc.run_sweep(rwr, scene)
    want = [record["pairs"][i] for i in record["indices"]]
    wrong = [(case, g, w) for case, g, w in zip(rc.sweep_cases(), got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(want)} calls differ from the record; the first: {wrong[0]}"


@pytest.mark.gpu
def test_argument_refusals_match_the_record(rwr, scene, record):
    assert set(record["arguments"]) == {name for name, _, _ in rc.ARGUMENT_CASES}
    assert all(code != 0 for code, _ in record["arguments"].values())
    assert rc.run_argument_cases(rwr, scene) == record["arguments"]


@pytest.mark.gpu
@pytest.mark.parametrize("entry", rc.SURFACE_ENTRY_POINTS)
def test_surface_entry_point_refusals_match_the_record(rwr, scene, record, entry):
    """Index out of range for part and sphere and each range check, per entry point; a refused call changes nothing."""
    want = record["surfaces"][entry]
    assert [w[0] for w in want] == [label for label, _ in rc.surface_error_calls(entry)]
    assert all(code == rwr.ERR_INVALID_ARGUMENT and msg for _, code, msg in want)
    assert rc.run_surface_errors(scene, entry) == want
    rough, refl = scene.get_part_gloss(0)
    assert rough == 0.25 and refl.tolist() == pytest.approx([0.8, 0.8, 0.9])
    assert scene.get_sphere_mirror(0) is not None and scene.get_sphere_glass(1) is not None
