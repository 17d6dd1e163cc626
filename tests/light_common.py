"""The scenes the light-sampling tests share (tests/test_light_host.py asserts with the CPU reference alone that each of them
exercises what the GPU file, tests/test_gpu_light_sampling.py, relies on), and the reference frames, computed once per session.
emission_common's `room`, `spheres`, `inside_sphere` and `with_models` are reused as they are; the others are this file's."""
import numpy as np

import emission_common as ec
import gloss_common
import light_ref

_cache = {}


def scene(name, rwr, ref_loader, suzanne, cube) -> dict:
    """emission_common.scene's entries.  No scene is larger than 80 x 56."""
    if name in ("room", "spheres", "inside_sphere", "with_models"):
        return ec.scene(name, rwr, ref_loader, suzanne, cube)
    key = ("scene", name)
    if key in _cache:
        return _cache[key]
    s = dict(ec.scene("room", rwr, ref_loader, suzanne, cube))
    if name == "hidden":           # a small lamp low behind the cube: the cube hides it from the floor in front, so reached < light rays
        s.update(spheres=rwr.make_spheres([((-1.7, -0.7, -1.2), 0.35)]), eye=(2.4, 1.8, 3.6), target=(0.0, -0.6, 0.0), w=72, h=48,
                 emissive_spheres={0: (8.0, 6.0, 4.0)})
    elif name == "two_lamps":      # two emitting spheres and a dark one between them in the order: every lane chooses its own
        s.update(spheres=rwr.make_spheres([((1.9, 0.3, 0.6), 0.5), ((0.0, 1.6, 0.2), 0.3), ((-1.8, 0.1, 1.0), 0.45)]), w=80, h=56,
                 emissive_spheres={0: (6.0, 2.0, 1.0), 2: (1.0, 3.0, 7.0)})
    elif name == "eight_lamps":    # every sphere index emits
        ring = [((2.3 * np.cos(0.8 * k), -0.6 + 0.25 * k, 2.3 * np.sin(0.8 * k)), 0.22 + 0.02 * k) for k in range(8)]
        s.update(spheres=rwr.make_spheres(ring), w=64, h=40, emissive_spheres={k: (1.0 + k, 4.0, 8.0 - k) for k in range(8)})
    elif name == "tiny":           # 5 x 3: a partial tile
        s.update(w=5, h=3, bounces=1)
    elif name == "far":            # a lamp far away: R / d ~ 0.01, the narrow end of the cone
        s.update(spheres=rwr.make_spheres([((6.0, 14.0, 9.0), 0.18)]), w=56, h=36, emissive_spheres={0: (64.0, 60.0, 50.0)})
    elif name == "lamp_around":    # the eye and the cube's near corner inside a large emitting sphere: hits inside it take no sample
        s.update(spheres=rwr.make_spheres([((1.1, 0.6, 1.9), 1.6)]), eye=(1.5, 0.8, 2.6), target=(0.2, -0.2, 0.0), fovy=70.0, w=60, h=40,
                 emissive_spheres={0: (0.5, 0.4, 0.3)})
    elif name == "mirror_lamp":    # the cube is a mirror: its reflected rays hit the lamp and keep Le
        s.update(model=[ec._plain(cube), gloss_common._floor(ref_loader, cube)], mirror_parts={0: (0.9, 0.9, 0.9)})
    elif name == "combo":          # a mirror cube on a diffuse floor, the lamp, a glass sphere, shadow rays: everything in one frame
        s.update(model=[ec._plain(cube), gloss_common._floor(ref_loader, cube)], mirror_parts={0: (0.9, 0.8, 0.7)}, shadows=True,
                 spheres=rwr.make_spheres([((1.9, 0.3, 0.6), 0.6), ((-0.4, -0.7, 1.9), 0.5)]), glass_spheres={1: (1.5, (1.0, 1.0, 1.0))})
    elif name == "grid":           # 4 x 4 instances of suzanne under a lamp: a BVH whose nodelets do not fit LDS (NODES_IN_LDS = false)
        s.update(model=suzanne, instances=rwr.make_instance_grid(4, 3.0), spheres=rwr.make_spheres([((0.5, 3.2, 0.5), 1.1)]), eye=(6.5, 3.0, 6.5),
                 target=(0.0, 0.0, 0.0), w=80, h=56, emissive_spheres={0: (8.0, 7.0, 5.0)})
    else:
        raise KeyError(name)
    _cache[key] = s
    return s


# the scenes of the GPU parity test; test_light_host.py states what each is there for
SCENES = ("room", "hidden", "two_lamps", "eight_lamps", "tiny", "far", "spheres", "inside_sphere", "lamp_around", "mirror_lamp", "with_models", "combo", "grid")
SPPS = ec.SPPS

n_parts = ec.n_parts
camera = ec.camera
max_le = ec.max_le


def n_lights(s) -> int:
    """M: the emitting spheres in use."""
    return sum(1 for k, le in s["emissive_spheres"].items() if k < len(s["spheres"]) and max(le) > 0.0)


def bar_factor(s) -> float:
    """The largest value a light term can take, the factor of the colour bar: max(1, min(64, 2 M max Le))."""
    return max(1.0, min(64.0, 2.0 * n_lights(s) * max_le(s)))


def flags(rwr, s, bounces=None, light=True, emissive=True, extra=0) -> int:
    return ec.flags(rwr, s, bounces=bounces, emissive=emissive, extra=extra | (rwr.FLAG_LIGHT_SAMPLING if light else 0))


def reference(L, rwr, orc, s, seed, spp, name, light=True, bounces=None, entry="light", shadows=None, samples=False, radii=None, sky="scene") -> dict:
    """The CPU reference's frame of scene s, kept for the session (never modified by a test).  light=False: the frame with
    RWR_FLAG_EMISSIVE alone, by the same loop; entry="emission": emission_render_path's frame."""
    bounces = s["bounces"] if bounces is None else bounces
    shadows = s["shadows"] if shadows is None else shadows
    sky = ec.sky_of(s) if sky == "scene" else sky
    key = ("ref", name, seed, spp, bounces, light, entry, shadows, samples, radii, sky)
    if key not in _cache:
        inst = None if s["instances"] is None else s["instances"].view(orc.INSTANCE_DTYPE)
        kw = dict(samples=samples) if entry == "light" else {}
        _cache[key] = light_ref.render_path(L, orc, camera(rwr, s).view(orc.CAMERA_INV_DTYPE), orc.make_screen(s["w"], s["h"]),
                                            orc.make_params(spp, bounces, seed=seed), s["spheres"].view(orc.SPHERE_DTYPE), s["model"],
                                            emissive_parts=s["emissive_parts"], emissive_spheres=s["emissive_spheres"], light=light, entry=entry,
                                            instances=inst, shadows=shadows, radii=radii, sky=sky if bounces else None,
                                            mirror_parts=s["mirror_parts"] if bounces else None, glass_spheres=s["glass_spheres"] if bounces else None,
                                            gloss_parts=s["gloss_parts"] if bounces else None, **kw)
    return _cache[key]
