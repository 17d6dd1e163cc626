"""The scenes the gloss tests share (tests/test_gloss_host.py asserts with the CPU reference alone that each of them exercises what
the GPU file, tests/test_gpu_gloss.py, relies on), and the reference frames, computed once per session."""
import numpy as np

import gloss_ref
import path_cases

WHITE = (1.0, 1.0, 1.0)
ROUGHNESSES = (2.0 ** -10, 0.05, 0.25, 1.0)
_cache = {}


def _split(cube):
    """The cube's faces dealt to two parts with materials of their own (both carry every vertex)."""
    return [{k: v for k, v in p.items() if k != "normal_map"} for p in path_cases._split(cube)]


def _merged(a, b):
    """One part of the faces of both models: a's material and texture."""
    faces = b["faces"].copy()
    faces["indices"] += len(a["vertices"])
    m = {k: v for k, v in a.items() if k != "normal_map"}
    m["vertices"] = np.concatenate([a["vertices"], b["vertices"]])
    m["faces"] = np.concatenate([a["faces"], faces])
    return m


def _floor(ref_loader, cube, y=-1.3, r=4.0):
    """A quad under the cube, its normal up."""
    return path_cases._quad(ref_loader, cube["texture"], [(-r, y, r), (r, y, r), (r, y, -r), (-r, y, -r)])


def scene(name, rwr, ref_loader, suzanne, cube) -> dict:
    """model (one model or a list of parts), spheres, instances, eye, target, fovy, w, h, bounces, gloss_parts / gloss_spheres
    ({index: (roughness, reflectance)}), glass_parts / glass_spheres ({index: (ior, tint)}), mirror_parts / mirror_spheres."""
    key = ("scene", name)
    if key in _cache:
        return _cache[key]
    none = rwr.make_spheres([])
    s = dict(instances=None, fovy=60.0, gloss_parts={}, gloss_spheres={}, glass_parts={}, glass_spheres={}, mirror_parts={}, mirror_spheres={},
             spheres=none, bounces=3)
    if name == "floor":            # one part, the cube and a floor under it, all of it glossy: the scalar read of record 0
        s.update(model=_merged(cube, _floor(ref_loader, cube)), eye=(2.1, 1.2, 3.3), target=(0.0, -0.4, 0.0), w=37, h=29,
                 gloss_parts={0: (0.25, (0.9, 0.8, 0.7))})
    elif name == "tiny":           # the same at 5 x 3, a partial tile, and B = 1: h0 alone emits, so the primary kernel alone applies the rule
        s.update(model=_merged(cube, _floor(ref_loader, cube)), eye=(2.1, 1.2, 3.3), target=(0.0, -0.4, 0.0), w=5, h=3, bounces=1,
                 gloss_parts={0: (0.05, WHITE)})
    elif name == "two_parts":      # two parts, one glossy: the per-lane read through ShadeRec::material
        plain = {k: v for k, v in cube.items() if k != "normal_map"}
        s.update(model=[plain, _floor(ref_loader, cube)], eye=(2.3, 1.5, 3.1), target=(0.0, -0.3, 0.0), w=80, h=56,
                 gloss_parts={1: (0.05, (0.8, 0.9, 1.0))})
    elif name == "spheres":        # glossy spheres in front of the mesh, records n_parts + k, at the two ends of the roughness range
        s.update(model=cube, spheres=rwr.make_spheres([((0.2, 0.1, 2.0), 0.7), ((-1.5, 0.4, 1.2), 0.5)]), eye=(0.45, 0.3, 3.5), target=(0.1, 0.0, 0.0),
                 w=70, h=45, gloss_spheres={0: (2.0 ** -10, (1.0, 0.9, 0.8)), 1: (1.0, (0.7, 1.0, 0.9))})
    elif name == "inside_sphere":  # the eye inside glossy sphere 0: h0 is seen from inside, n points outward; a diffuse sphere and the cube outside
        s.update(model=cube, spheres=rwr.make_spheres([((0.3, 0.2, 3.4), 0.9), ((1.6, 0.5, 1.2), 0.5)]), eye=(0.95, 0.3, 3.75), target=(0.3, 0.0, 0.0),
                 fovy=75.0, w=61, h=37, gloss_spheres={0: (0.25, (0.8, 0.9, 1.0))})
    elif name == "instances":      # a glossy part under three rotated instances, the other part diffuse: a world face's part is its base face's
        inst = path_cases.instances(rwr, [path_cases._rotation(a, t) for a, t in (((1, 1, 0), 0.7), ((0, 1, 1), 2.1), ((1, 0, 1), 4.0))],
                                    [(-3.1, 0.0, 0.0), (0.0, 0.2, 0.0), (3.1, -0.1, 0.3)])
        s.update(model=_split(cube), spheres=rwr.make_spheres([((0.0, 2.3, 0.4), 0.6)]), instances=inst, eye=(0.4, 1.7, 5.2), target=(0.0, 0.0, 0.0),
                 fovy=55.0, w=72, h=40, gloss_parts={1: (1.0, (1.0, 0.8, 0.9))})
    elif name == "all_three":      # a glossy part beside a mirror part and a glass sphere: SURF 3 with all three record kinds
        wall = path_cases._quad(ref_loader, cube["texture"], [(-3.0, -2.0, -1.5), (3.0, -2.0, -1.5), (3.0, 2.5, -1.5), (-3.0, 2.5, -1.5)])
        s.update(model=[wall, {k: v for k, v in cube.items() if k != "normal_map"}], spheres=rwr.make_spheres([((-1.4, 0.1, 1.0), 0.6)]),
                 eye=(0.9, 0.8, 3.6), target=(0.0, 0.0, -0.5), w=66, h=43,
                 mirror_parts={0: (0.9, 0.95, 1.0)}, gloss_parts={1: (0.25, (0.9, 0.9, 0.6))}, glass_spheres={0: (1.5, WHITE)})
    else:
        raise KeyError(name)
    _cache[key] = s
    return s


GPU_SCENES = ("floor", "tiny", "two_parts", "spheres", "inside_sphere", "instances", "all_three")
SPPS = (1, 2, 33)   # 33 crosses the launch groups of 32 unevenly


def n_parts(s) -> int:
    return len(s["model"]) if isinstance(s["model"], (list, tuple)) else 1


def camera(rwr, s, w=None, h=None):
    w, h = w or s["w"], h or s["h"]
    return rwr.camera_build_inv_uniform(rwr.make_camera(eye=s["eye"], target=s["target"], aspect=w / h, fovy=s["fovy"]))


def as_mirrors(s) -> dict:
    """Scene s with every glossy surface set as a mirror of the same reflectance instead."""
    parts, spheres = dict(s["mirror_parts"]), dict(s["mirror_spheres"])
    parts.update({k: r for k, (_, r) in s["gloss_parts"].items()})
    spheres.update({k: r for k, (_, r) in s["gloss_spheres"].items()})
    return dict(s, gloss_parts={}, gloss_spheres={}, mirror_parts=parts, mirror_spheres=spheres)


def reference(L, rwr, orc, s, seed, spp, sky=None, shadows=False, bounces=None, name=None, thr_unorm16=False) -> dict:
    """The CPU reference's frame of scene s, kept for the session (never modified by a test)."""
    bounces = s["bounces"] if bounces is None else bounces
    key = ("ref", name or id(s), seed, sky, shadows, spp, bounces, thr_unorm16)
    if key not in _cache:
        inst = None if s["instances"] is None else s["instances"].view(orc.INSTANCE_DTYPE)
        _cache[key] = gloss_ref.render_path(L, orc, camera(rwr, s).view(orc.CAMERA_INV_DTYPE), orc.make_screen(s["w"], s["h"]),
                                            orc.make_params(spp, bounces, seed=seed), s["spheres"].view(orc.SPHERE_DTYPE), s["model"],
                                            instances=inst, shadows=shadows, sky=sky, mirror_parts=s["mirror_parts"], mirror_spheres=s["mirror_spheres"],
                                            glass_parts=s["glass_parts"], glass_spheres=s["glass_spheres"],
                                            gloss_parts=s["gloss_parts"], gloss_spheres=s["gloss_spheres"], thr_unorm16=thr_unorm16)
    return _cache[key]
