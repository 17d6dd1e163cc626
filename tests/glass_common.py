"""The scenes the glass tests share (tests/test_glass_host.py asserts with the CPU reference alone that each of them exercises what
the GPU file, tests/test_gpu_glass.py, relies on), and the reference frames, computed once per session."""
import numpy as np

import glass_ref
import path_cases
import world_offset_common

CLEAR = (1.0, 1.0, 1.0)
_cache = {}


def _split(cube):
    """The cube's faces dealt to two parts with materials of their own (both carry every vertex)."""
    return [{k: v for k, v in p.items() if k != "normal_map"} for p in path_cases._split(cube)]


def scene(name, rwr, ref_loader, suzanne, cube) -> dict:
    """model (one model or a list of parts), spheres, instances, eye, target, fovy, w, h, bounces, glass_parts / glass_spheres
    ({index: (ior, tint)}), mirror_parts / mirror_spheres, claims: the events the scene is there for."""
    key = ("scene", name)
    if key in _cache:
        return _cache[key]
    none = rwr.make_spheres([])
    s = dict(instances=None, fovy=60.0, glass_parts={}, glass_spheres={}, mirror_parts={}, mirror_spheres={}, spheres=none,
             claims=("reflected", "transmitted"))
    if name == "sphere_cube":      # a glass sphere in front of the textured cube: rays enter and leave it, the cube shows through
        s.update(model=cube, spheres=rwr.make_spheres([((0.2, 0.1, 2.0), 0.7)]), eye=(0.45, 0.3, 3.5), target=(0.1, 0.0, 0.0), w=70, h=45, bounces=4,
                 glass_spheres={0: (1.5, (0.9, 1.0, 0.8))}, claims=("reflected", "transmitted", "multi"))
    elif name == "cube_room":      # the glass cube (a closed part: inner faces met at grazing angles) in the cube scaled to a closed room
        room = world_offset_common.translated(cube, (0.0, 0.0, 0.0), scale=4.0)
        s.update(model=[cube, room], eye=(2.3, 1.5, 3.1), target=(0.0, 0.0, 0.0), w=80, h=56, bounces=6,
                 glass_parts={0: (1.5, CLEAR)}, claims=("reflected", "transmitted", "tir", "multi"))
    elif name == "inside_sphere":  # the eye inside glass sphere 0: h0 is seen from inside, n points outward; a second, diffuse sphere and the cube outside
        s.update(model=cube, spheres=rwr.make_spheres([((0.3, 0.2, 3.4), 0.9), ((1.6, 0.5, 1.2), 0.5)]), eye=(0.95, 0.3, 3.75), target=(0.3, 0.0, 0.0),
                 fovy=75.0, w=61, h=37, bounces=3, glass_spheres={0: (1.33, (0.8, 0.9, 1.0))}, claims=("reflected", "transmitted", "tir"))
    elif name == "instances":      # a glass part under three rotated instances, the other part diffuse: a world face's part is its base face's
        inst = path_cases.instances(rwr, [path_cases._rotation(a, t) for a, t in (((1, 1, 0), 0.7), ((0, 1, 1), 2.1), ((1, 0, 1), 4.0))],
                                    [(-3.1, 0.0, 0.0), (0.0, 0.2, 0.0), (3.1, -0.1, 0.3)])
        s.update(model=_split(cube), spheres=rwr.make_spheres([((0.0, 2.3, 0.4), 0.6)]), instances=inst, eye=(0.4, 1.7, 5.2), target=(0.0, 0.0, 0.0),
                 fovy=55.0, w=72, h=40, bounces=4, glass_parts={1: (1.5, (1.0, 0.8, 0.9))}, claims=("reflected", "transmitted", "tir"))
    elif name == "facing_mirror":  # glass facing a mirror, B = 8: a glass sphere between the eye and a mirror quad, a diffuse cube aside
        tex = cube["texture"]
        wall = path_cases._quad(ref_loader, tex, [(-3.0, -2.0, -1.5), (3.0, -2.0, -1.5), (3.0, 2.5, -1.5), (-3.0, 2.5, -1.5)])
        small = world_offset_common.translated(cube, (1.6, -0.4, 0.2), scale=0.5)
        s.update(model=[wall, small], spheres=rwr.make_spheres([((-0.2, 0.1, 0.4), 0.8)]), eye=(0.4, 0.5, 3.4), target=(0.0, 0.0, -1.0), w=66, h=43,
                 bounces=8, glass_spheres={0: (1.5, CLEAR)}, mirror_parts={0: (0.9, 0.95, 1.0)}, claims=("reflected", "transmitted", "multi"))
    elif name == "black":          # C = 0: the rays that leave the glass carry nothing and are counted all the same
        s.update(model=cube, spheres=rwr.make_spheres([((0.2, 0.1, 2.0), 0.7)]), eye=(0.45, 0.3, 3.5), target=(0.1, 0.0, 0.0), w=45, h=30, bounces=3,
                 glass_spheres={0: (1.5, (0.0, 0.0, 0.0))})
    elif name == "eta_one":        # eta = 1: r0 = 0, F = (1 - c)^5, never a total reflection; rays pass straight through
        s.update(model=cube, spheres=rwr.make_spheres([((0.2, 0.1, 2.0), 0.7)]), eye=(0.45, 0.3, 3.5), target=(0.1, 0.0, 0.0), w=45, h=30, bounces=3,
                 glass_spheres={0: (1.0, CLEAR)}, claims=("reflected", "transmitted", "multi"))
    elif name == "far":            # 1e4 from the origin on every axis: the 1e-4 offsets are below an ulp of the coordinates there
        off = np.asarray(world_offset_common.OFFSETS["1e4"], np.float64)
        s.update(model=world_offset_common.translated(cube, off), spheres=rwr.make_spheres([(tuple(np.array([0.2, 0.1, 2.0]) + off), 0.7)]),
                 eye=tuple(np.array([0.45, 0.3, 3.5]) + off), target=tuple(np.array([0.1, 0.0, 0.0]) + off), w=50, h=33, bounces=4,
                 glass_spheres={0: (1.5, CLEAR)})
    else:
        raise KeyError(name)
    _cache[key] = s
    return s


GPU_SCENES = ("sphere_cube", "cube_room", "inside_sphere", "instances", "facing_mirror", "black", "eta_one", "far")
SPPS = (1, 2, 33, 65)   # 33 and 65 cross the launch groups of 32 unevenly


def n_parts(s) -> int:
    return len(s["model"]) if isinstance(s["model"], (list, tuple)) else 1


def camera(rwr, s, w=None, h=None):
    w, h = w or s["w"], h or s["h"]
    return rwr.camera_build_inv_uniform(rwr.make_camera(eye=s["eye"], target=s["target"], aspect=w / h, fovy=s["fovy"]))


def reference(L, rwr, orc, s, seed, spp, glass=True, mirrors=True, sky=None, shadows=False, bounces=None, name=None) -> dict:
    """The CPU reference's frame of scene s, kept for the session (never modified by a test)."""
    bounces = s["bounces"] if bounces is None else bounces
    key = ("ref", name or id(s), seed, glass, mirrors, sky, shadows, spp, bounces)
    if key not in _cache:
        inst = None if s["instances"] is None else s["instances"].view(orc.INSTANCE_DTYPE)
        _cache[key] = glass_ref.render_path(L, orc, camera(rwr, s).view(orc.CAMERA_INV_DTYPE), orc.make_screen(s["w"], s["h"]),
                                            orc.make_params(spp, bounces, seed=seed), s["spheres"].view(orc.SPHERE_DTYPE), s["model"],
                                            instances=inst, shadows=shadows, sky=sky,
                                            mirror_parts=s["mirror_parts"] if mirrors else None, mirror_spheres=s["mirror_spheres"] if mirrors else None,
                                            glass_parts=s["glass_parts"] if glass else None, glass_spheres=s["glass_spheres"] if glass else None)
    return _cache[key]
