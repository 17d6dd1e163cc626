"""The frame kernel's quad form of a diffuse texture (rwr_internal.h QuadTex), built on the host at upload: checked
against a numpy model of its definition, clamp edges and 1-texel-wide textures included.  No GPU."""
import numpy as np
import pytest


def _quads_model(tex):
    h, w = tex.shape[:2]
    t = tex.astype(np.uint32)
    packed = t[..., 0] << 2 | t[..., 1] << 12 | t[..., 2] << 22
    py, px = np.mgrid[0:h + 1, 0:w + 1]
    cx0, cx1 = np.clip(px - 1, 0, w - 1), np.clip(px, 0, w - 1)
    cy0, cy1 = np.clip(py - 1, 0, h - 1), np.clip(py, 0, h - 1)
    return np.stack([packed[cy0, cx0], packed[cy0, cx1], packed[cy1, cx0], packed[cy1, cx1]], -1).astype(np.uint32)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (3, 5), (16, 16), (33, 65)])
def test_quads_match_model(rwr, shape):
    rng = np.random.default_rng(sum(shape))
    tex = rng.integers(0, 256, size=shape + (4,), dtype=np.uint8)
    got = rwr.host_texture_quads(tex)
    assert got.shape == (shape[0] + 1, shape[1] + 1, 4)
    assert np.array_equal(got, _quads_model(tex))
    # every channel is a byte offset into the 256-float decode table, alpha dropped
    assert np.array_equal((got >> 2) & 0xff, np.broadcast_to(got & 0x3fc, got.shape) >> 2)
    assert int(got.max() >> 30) == 0


def test_quads_reject_empty(rwr):
    with pytest.raises(Exception):
        rwr.host_texture_quads(np.zeros((0, 3, 4), np.uint8))
