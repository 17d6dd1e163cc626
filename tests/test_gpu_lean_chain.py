"""The lean resting form's shorter chain of loads (kernels_primary_p2.hip k_primary_p2_lean): the tile arrays' strides and the
numerators' address reach the kernel as arguments that launch_primary_p2 computes from the grid it launches, and a wave asks for
its tile's cover word together with the class word, before it knows the class.  What that adds to get wrong: a stride that is not
the launched grid's (a band of rows, every n-th strip, a grid whose last column and row of workgroups are half in the frame), a
stale address after the model's buffers were made again, and a cover word read — and ignored — by a tile of another class.

The method is test_gpu_lean_rest.py's, with its helpers: two fresh contexts that differ in RWR_LEAN_REST alone get the same calls
(=0: the cover form, untouched, renders those frames); colour and depth of every frame are the same bytes, rwr_lean_rest_stats
moves in the "on" context alone, and the cover words both contexts learnt are equal."""
import numpy as np
import pytest

import test_gpu_lean_rest as lr

pytestmark = pytest.mark.gpu

SIZE = (256, 144)


def _same_cover(on, off):
    assert np.array_equal(on.tile_cover(), off.tile_cover())
    assert on.tile_cover_stats()[1] == off.tile_cover_stats()[1]
    return on.tile_cover_stats()[1]


@pytest.mark.parametrize("size", [(64, 8), (96, 12), (65, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_grids(rwr, suzanne, size):
    """One workgroup; a last column and a last row of workgroups half in the frame; an odd width."""
    n = 2
    with lr._pair(rwr, size, n, lr._scene(rwr, suzanne)) as (on, off):
        cam_inv = lr._cam(rwr, size, **lr.CFG2)
        _, cls = lr._fully_one_face(rwr, off, cam_inv, size)
        on.render(cam_inv, rwr.make_params(flags=rwr.FLAG_AUX_OUTPUTS))   # (the same calls in both)
        on.readback(aux=True)
        assert lr._rest(rwr, on, off, cam_inv, n, size) >= 2 * n
        assert np.array_equal(on.tile_classes(), cls)
        tiles = _same_cover(on, off)
        # covered tiles only where the off context's class words show a one-face tile (64x8 has none)
        one = (cls & (lr.FACES | lr.SPHERES)) == 1
        assert one.any() == (size != (64, 8)), (size, int(one.sum()))
        assert (tiles > 0) == bool(one.any()), (size, int(one.sum()), tiles)


@pytest.mark.parametrize("n_slots", [1, 3])
@pytest.mark.parametrize("shape", [dict(rows=(8, 72)), dict(rows=(16, 144)), dict(strips=(0, 2)), dict(strips=(1, 3))],
                         ids=["rows8-72", "rows16-144", "strips0of2", "strips1of3"])
def test_grids_that_are_not_the_frames(rwr, suzanne, shape, n_slots):
    """A band of rows and every n-th strip: the strides are those of the launched grid, not of the frame's."""
    with lr._pair(rwr, SIZE, n_slots, lr._scene(rwr, suzanne)) as (on, off):
        cam_inv = lr._cam(rwr, SIZE, **lr.CFG2)
        assert lr._rest(rwr, on, off, cam_inv, n_slots, (shape, n_slots), **shape) >= 2 * n_slots
        assert _same_cover(on, off) > 0, (shape, n_slots)


def test_new_buffers_and_a_new_size(rwr, suzanne):
    """The same mesh uploaded again (new buffers: a new address of the numerators), then another frame size: the lean form is back
    after each, on the new address and the new strides."""
    n = 2
    with lr._pair(rwr, SIZE, n, lr._scene(rwr, suzanne)) as (on, off):
        cam_inv = lr._cam(rwr, SIZE, **lr.CFG2)
        assert lr._rest(rwr, on, off, cam_inv, n, "start") >= 2 * n
        assert _same_cover(on, off) > 0
        for c in (on, off):
            c.upload_model(suzanne)
        assert lr._rest(rwr, on, off, cam_inv, n, "upload") >= 2 * n
        assert _same_cover(on, off) > 0
        other = (130, 20)
        for c in (on, off):
            c.resize(*other)
        assert lr._rest(rwr, on, off, lr._cam(rwr, other, **lr.CFG2), n, "resize") >= 2 * n
        _same_cover(on, off)


def test_tiles_of_class_none_ignore_their_cover_word(rwr, suzanne):
    """The mesh in the middle of the frame, nothing around it, one slot: the tiles of class "none" read a cover word they have no
    use for."""
    with lr._pair(rwr, SIZE, 1, lr._scene(rwr, suzanne)) as (on, off):
        cam_inv = lr._cam(rwr, SIZE, **lr.CFG2B)
        _, cls = lr._fully_one_face(rwr, off, cam_inv, SIZE)
        on.render(cam_inv, rwr.make_params(flags=rwr.FLAG_AUX_OUTPUTS))
        on.readback(aux=True)
        assert ((cls & (lr.FACES | lr.SPHERES)) == 0).any()
        assert lr._rest(rwr, on, off, cam_inv, 1, "cfg2b") >= 2
        assert np.array_equal(on.tile_classes(), cls)
        _same_cover(on, off)
