"""What the tone-mapping tests share: the frames of the GPU file's parity cases (tests/test_gpu_tonemap.py) - emission_common's
scenes at the sizes the stage's kernels can go wrong at - and the parameter sets.  tests/test_tonemap_host.py asserts on the CPU path
reference's frames of the same scenes that they hold what the GPU file relies on."""
import emission_common as ec

# (scene, width, height): 70 x 13 is no multiple of 64 or 8, of 256 or 512 pixels (910: the last workgroup of either kernel is partly
# empty, and the second pixel of some lanes is missing); 64 x 8 is exactly one tile, 512 pixels: one full workgroup of the map;
# 200 x 120 has 94 workgroups of the measure, whose sums meet in the record's two atomics
FRAMES = (("room", 70, 13), ("clamped", 70, 13), ("tiny", 70, 13), ("room", 64, 8), ("room", 200, 120))
SPPS = (1, 33)   # 33 crosses the launch groups of 32 unevenly
# all three curves, manual and auto; the manual exposures are no powers of two, white and key are not the defaults everywhere
PARAMS = (dict(curve=0, auto_exposure=0, exposure=0.37),
          dict(curve=1, auto_exposure=0, exposure=1.0, white=4.0),
          dict(curve=2, auto_exposure=0, exposure=1.0),
          dict(curve=0, auto_exposure=1, exposure=1.0, key=0.18),
          dict(curve=1, auto_exposure=1, exposure=1.7, key=0.25, white=2.5),
          dict(curve=2, auto_exposure=1, exposure=1.0, key=0.18))


def sized(rwr, ref_loader, suzanne, cube, name, w, h) -> dict:
    """emission_common's scene `name` on a w x h screen (a copy: the session's scene stays as it is)."""
    return dict(ec.scene(name, rwr, ref_loader, suzanne, cube), w=w, h=h)


def label(name, w, h) -> str:
    return f"{name}@{w}x{h}"
