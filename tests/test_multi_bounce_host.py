"""Deeper paths (RWR_FLAG_MULTI_BOUNCE), host side: the tests' CPU reference (path_ref.c, built on the oracle) against the oracle
where both define the frame, the definition's consequences, and the public constants.  No GPU."""
import os
import re

import numpy as np
import pytest

import path_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("color", "depth", "color_f32", "obj_id", "hit_t")


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return path_ref.lib(tmp_path_factory)


def _scene(name, rwr, orc, suzanne, cube):
    """(model, spheres, instances, eye, target, flags) of the scenes the tests use."""
    if name == "suzanne":
        return suzanne, orc.make_spheres(), None, (0.3, 0.2, 2.5), (0.2, 0.2, -2.0), 0
    if name == "cube":
        return cube, orc.make_spheres([((1.6, 1.2, 1.4), 0.5)]), None, (2.2, 1.7, 3.1), (0, 0, 0), 0
    if name == "grid":
        return suzanne, orc.make_spheres(), rwr.make_instance_grid(2, 3.0).view(orc.INSTANCE_DTYPE), (1.5, -1.5, 7.0), (1.5, -1.5, 0), 0
    if name == "two_parts":
        return [suzanne, cube], orc.make_spheres(), None, (0.5, 0.5, 4.0), (0, 0, 0), 0
    if name == "cube_nmap":
        return cube, orc.make_spheres([((1.6, 1.2, 1.4), 0.5)]), None, (2.2, 1.7, 3.1), (0, 0, 0), orc.FLAG_NORMAL_MAP
    raise KeyError(name)


def _render(pref, rwr, orc, scene, w, h, spp, bounces, seed=7, ref=False):
    model, spheres, inst, eye, target, flags = scene
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=eye, target=target, aspect=w / h)).view(orc.CAMERA_INV_DTYPE)
    params = orc.make_params(spp, bounces, seed=seed, flags=flags)
    if ref:
        return orc.render_path(cam_inv, orc.make_screen(w, h), params, spheres, model, instances=inst)
    return path_ref.render_path(pref, orc, cam_inv, orc.make_screen(w, h), params, spheres, model, instances=inst)


@pytest.mark.parametrize("name", ["suzanne", "cube", "grid", "two_parts", "cube_nmap"])
@pytest.mark.parametrize("bounces", [0, 1])
def test_reference_equals_the_oracle_up_to_one_bounce(pref, rwr, orc, suzanne, cube, name, bounces):
    scene = _scene(name, rwr, orc, suzanne, cube)
    for spp in (1, 3):
        got = _render(pref, rwr, orc, scene, 48, 32, spp, bounces)
        want = _render(pref, rwr, orc, scene, 48, 32, spp, bounces, ref=True)
        for k in PLANES:
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (name, spp, k)
        assert (got["obj_id"] >= 0).any()
        # one bounce ray per primary hit (alpha / 2 counts them)
        hits = int(round(float(want["color_f32"][..., 3].sum()) / 2.0 * spp))
        assert got["rays"] == (hits if bounces else 0)


def test_bounce_direction_at_dimension_two_is_the_oracles(pref, orc):
    rng = np.random.default_rng(3)
    n = rng.normal(size=(10000, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[:20] = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0]] * 5   # basis edge cases (n.z = +-1, 0)
    keys = rng.integers(0, 2**32, size=(10000, 3), dtype=np.uint64)
    for i in range(len(n)):
        pixel, sample, seed = (int(v) for v in keys[i])
        a = path_ref.bounce_direction(pref, n[i], pixel, sample, seed, 2)
        b = orc.bounce_direction(n[i], pixel, sample, seed)
        assert a.tobytes() == b.tobytes(), i
    # other dimensions draw other directions
    c = path_ref.bounce_direction(pref, n[0], 5, 6, 7, 18)
    assert c.tobytes() != path_ref.bounce_direction(pref, n[0], 5, 6, 7, 2).tobytes()


@pytest.mark.parametrize("name", ["cube", "grid"])
def test_colour_grows_with_depth_and_sample_zero_planes_do_not_change(pref, rwr, orc, suzanne, cube, name):
    scene = _scene(name, rwr, orc, suzanne, cube)
    frames = [_render(pref, rwr, orc, scene, 40, 30, 3, b) for b in range(5)]
    for a, b in zip(frames, frames[1:]):
        assert (b["color_f32"] >= a["color_f32"]).all()
        assert (b["color"] >= a["color"]).all()
        assert b["rays"] >= a["rays"]
        for k in ("depth", "obj_id", "hit_t"):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        assert np.array_equal(a["color_f32"][..., 3], b["color_f32"][..., 3])
    # interreflection really adds light somewhere
    assert (frames[4]["color_f32"][..., :3] > frames[1]["color_f32"][..., :3]).any()


def test_inside_a_closed_room_every_bounce_is_traced(pref, rwr, orc, cube):
    w, h, spp = 32, 24, 2
    scene = (cube, np.zeros(0, orc.SPHERE_DTYPE), None, (0.1, 0.2, 0.3), (0.0, 0.0, -1.0), 0)
    for bounces in (0, 1, 3, 8):
        got = _render(pref, rwr, orc, scene, w, h, spp, bounces)
        assert (got["obj_id"] >= 0).all()
        assert got["rays"] == w * h * spp * bounces


def test_header_and_driver_agree_on_the_constants(rwr):
    text = open(os.path.join(ROOT, "include", "rwr_hip.h")).read()
    m = re.search(r"RWR_FLAG_MULTI_BOUNCE\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and int(m.group(1)) == 6
    m = re.search(r"#define\s+RWR_MAX_BOUNCES\s+(\d+)u?\b", text)
    assert m and int(m.group(1)) == 8
    assert rwr.FLAG_MULTI_BOUNCE == 1 << 6 and rwr.MAX_BOUNCES == 8
    # the new flag takes a bit nobody else has
    others = [int(v) for v in re.findall(r"RWR_FLAG_\w+\s*=\s*1u\s*<<\s*(\d+)", text)]
    assert others.count(6) == 1
