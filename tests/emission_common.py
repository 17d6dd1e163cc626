"""The scenes the emission tests share (tests/test_emission_host.py asserts with the CPU reference alone that each of them exercises
what the GPU file, tests/test_gpu_emission.py, relies on), and the reference frames, computed once per session."""
import numpy as np

import emission_ref
import gloss_common
import path_cases

WHITE = (1.0, 1.0, 1.0)
_cache = {}


def _plain(model):
    return {k: v for k, v in model.items() if k != "normal_map"}


def scene(name, rwr, ref_loader, suzanne, cube) -> dict:
    """gloss_common.scene's entries, plus emissive_parts / emissive_spheres ({index: (r, g, b)}) and shadows (the frame casts shadow
    rays).  No scene is larger than 80 x 56; Le components are <= 8 except in `clamped`."""
    key = ("scene", name)
    if key in _cache:
        return _cache[key]
    none = rwr.make_spheres([])
    s = dict(instances=None, fovy=60.0, gloss_parts={}, gloss_spheres={}, glass_parts={}, glass_spheres={}, mirror_parts={}, mirror_spheres={},
             spheres=none, bounces=1, shadows=False, emissive_parts={}, emissive_spheres={})
    floor = gloss_common._floor
    if name == "tiny":             # 5 x 3, one part that emits, no bounce: the primary kernel alone, a partial tile, the scalar read of record 0
        s.update(model=gloss_common._merged(cube, floor(ref_loader, cube)), eye=(2.1, 1.2, 3.3), target=(0.0, -0.4, 0.0), w=5, h=3, bounces=0,
                 emissive_parts={0: (0.5, 0.25, 1.0)})
    elif name == "room":           # one part that does not emit, a lamp: sphere 0 above the floor beside the cube; light arrives by bounce hits on it
        s.update(model=gloss_common._merged(cube, floor(ref_loader, cube)), spheres=rwr.make_spheres([((1.9, 0.3, 0.6), 0.6)]),
                 eye=(2.1, 1.6, 3.9), target=(0.3, -0.5, 0.0), w=64, h=40, bounces=2, emissive_spheres={0: (8.0, 7.0, 5.0)})
    elif name == "two_parts":      # two parts, part 1 (the floor) emits: the per-lane read through ShadeRec::material
        s.update(model=[_plain(cube), floor(ref_loader, cube)], eye=(2.3, 1.5, 3.1), target=(0.0, -0.3, 0.0), w=80, h=56,
                 emissive_parts={1: (2.0, 1.0, 0.5)})
    elif name == "spheres":        # two spheres in front of the cube, sphere 1 emits: records n_parts + k
        s.update(model=cube, spheres=rwr.make_spheres([((0.2, 0.1, 2.0), 0.7), ((-1.5, 0.4, 1.2), 0.5)]), eye=(0.45, 0.3, 3.5), target=(0.1, 0.0, 0.0),
                 w=70, h=45, emissive_spheres={1: (1.0, 4.0, 8.0)})
    elif name == "inside_sphere":  # the eye inside emitting sphere 0: it emits inwards; a plain sphere and the cube outside
        s.update(model=cube, spheres=rwr.make_spheres([((0.3, 0.2, 3.4), 0.9), ((1.6, 0.5, 1.2), 0.5)]), eye=(0.95, 0.3, 3.75), target=(0.3, 0.0, 0.0),
                 fovy=75.0, w=61, h=37, emissive_spheres={0: (0.75, 0.5, 0.25)})
    elif name == "instances":      # an emitting part under three rotated instances, the other part dark: a world face's part is its base face's
        inst = path_cases.instances(rwr, [path_cases._rotation(a, t) for a, t in (((1, 1, 0), 0.7), ((0, 1, 1), 2.1), ((1, 0, 1), 4.0))],
                                    [(-2.2, 0.0, 0.0), (0.0, 0.2, 0.0), (2.2, -0.1, 0.3)])
        s.update(model=gloss_common._split(cube), spheres=rwr.make_spheres([((0.0, 2.3, 0.4), 0.6)]), instances=inst, eye=(0.4, 1.7, 5.2),
                 target=(0.0, 0.0, 0.0), fovy=55.0, w=72, h=40, bounces=2, emissive_parts={1: (3.0, 2.0, 6.0)})
    elif name == "with_models":    # gloss_common's all_three, the mirror part and the glass sphere emitting as well: emission beside every model
        a = gloss_common.scene("all_three", rwr, ref_loader, suzanne, cube)
        s.update({k: a[k] for k in ("model", "spheres", "eye", "target", "w", "h", "bounces", "mirror_parts", "gloss_parts", "glass_spheres")})
        s.update(emissive_parts={0: (0.5, 0.25, 0.125)}, emissive_spheres={0: (2.0, 3.0, 1.0)})
    elif name == "shadowed":       # shadow rays on, an emitting floor under the cube: hits in the cube's shadow keep ambient + Le
        s.update(model=[_plain(cube), floor(ref_loader, cube)], eye=(2.3, 1.9, 3.1), target=(0.0, -0.6, 0.0), w=60, h=44, shadows=True,
                 emissive_parts={1: (0.5, 1.0, 2.0)})
    elif name == "clamped":        # Le = 64 on the floor, seen directly and by the bounce rays of the cube, a white mirror (T = 1: the term reaches its cap)
        s.update(model=[_plain(cube), floor(ref_loader, cube)], eye=(2.3, 1.5, 3.1), target=(0.0, -0.3, 0.0), w=48, h=32, bounces=2,
                 mirror_parts={0: WHITE}, emissive_parts={1: (64.0, 64.0, 64.0)})
    else:
        raise KeyError(name)
    _cache[key] = s
    return s


SCENES = ("tiny", "room", "two_parts", "spheres", "inside_sphere", "instances", "with_models", "shadowed", "clamped")
SPPS = (1, 2, 33)   # 33 crosses the launch groups of 32 unevenly

n_parts = gloss_common.n_parts
camera = gloss_common.camera


def max_le(s) -> float:
    """The scene's largest Le component (the colour bar scales with it)."""
    return max([max(le) for le in list(s["emissive_parts"].values()) + list(s["emissive_spheres"].values())] + [0.0])


def sky_of(s):
    """The frames of a scene with surface models are lit by the default sky too, as the gloss tests' are; the others by nothing else."""
    return (emission_ref.glass_ref.DEFAULT_ZENITH, emission_ref.glass_ref.DEFAULT_HORIZON) if s["gloss_parts"] else None


def flags(rwr, s, bounces=None, emissive=True, extra=0) -> int:
    bounces = s["bounces"] if bounces is None else bounces
    return (rwr.FLAG_AUX_OUTPUTS | extra | (rwr.FLAG_MULTI_BOUNCE if bounces > 1 else 0) | (rwr.FLAG_SHADOWS if s["shadows"] else 0) |
            (rwr.FLAG_SKY if sky_of(s) else 0) | (rwr.FLAG_MIRRORS if s["mirror_parts"] else 0) | (rwr.FLAG_GLASS if s["glass_spheres"] else 0) |
            (rwr.FLAG_GLOSSY if s["gloss_parts"] else 0) | (rwr.FLAG_EMISSIVE if emissive else 0))


def reference(L, rwr, orc, s, seed, spp, name, emissive=True, bounces=None, entry="emission", table=None) -> dict:
    """The CPU reference's frame of scene s, kept for the session (never modified by a test).  emissive=False: the frame without the
    flag (no table); entry="soft": soft_render_path's frame; table: this emission table in place of the scene's."""
    bounces = s["bounces"] if bounces is None else bounces
    key = ("ref", name, seed, spp, bounces, emissive, entry, None if table is None else table.tobytes())
    if key not in _cache:
        inst = None if s["instances"] is None else s["instances"].view(orc.INSTANCE_DTYPE)
        glow = dict(table=table) if table is not None else dict(emissive_parts=s["emissive_parts"], emissive_spheres=s["emissive_spheres"]) if emissive else {}
        _cache[key] = emission_ref.render_path(L, orc, camera(rwr, s).view(orc.CAMERA_INV_DTYPE), orc.make_screen(s["w"], s["h"]),
                                               orc.make_params(spp, bounces, seed=seed), s["spheres"].view(orc.SPHERE_DTYPE), s["model"],
                                               instances=inst, shadows=s["shadows"], sky=sky_of(s) if bounces else None,
                                               mirror_parts=s["mirror_parts"] if bounces else None, glass_spheres=s["glass_spheres"] if bounces else None,
                                               gloss_parts=s["gloss_parts"] if bounces else None, entry=entry, **glow)
    return _cache[key]
