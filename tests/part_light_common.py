"""The scenes the tests of light sampling towards emitting parts share (tests/test_part_light_host.py asserts with the CPU reference
alone that each of them exercises what the GPU file, tests/test_gpu_part_light.py, relies on), and the reference frames, computed once
per session.  emission_common's and light_common's pieces are reused; a scene here also says whether its frames carry
RWR_FLAG_LIGHT_SAMPLING ("light") beside RWR_FLAG_LIGHT_PARTS."""
import numpy as np

import emission_common as ec
import gloss_common
import large_scenes
import light_common as lc
import part_light_ref
import path_cases

_cache = {}
LAMP = ((1.9, 0.3, 0.6), 0.6)          # emission_common's room lamp
PANEL_LE = (8.0, 7.0, 5.0)


def _panel(ref_loader, cube, x=(-0.8, 0.8), y=2.2, z=(-0.6, 0.6)):
    """A quad hanging clear of floor and cube (the cube's top is at y = 1), its normal down: two faces."""
    return path_cases._quad(ref_loader, cube["texture"], [(x[0], y, z[0]), (x[1], y, z[0]), (x[1], y, z[1]), (x[0], y, z[1])])


def scene(name, rwr, ref_loader, suzanne, cube, orc=None) -> dict:
    """emission_common.scene's entries plus "light".  No scene is larger than 80 x 56."""
    key = ("scene", name)
    if key in _cache:
        return _cache[key]
    s = dict(ec.scene("room", rwr, ref_loader, suzanne, cube))
    room = gloss_common._merged(cube, gloss_common._floor(ref_loader, cube))
    none = rwr.make_spheres([])
    s.update(model=[room, _panel(ref_loader, cube)], spheres=none, emissive_spheres={}, emissive_parts={1: PANEL_LE}, light=False, w=64, h=40, bounces=2)
    if name == "panel":            # the room with a 2-face emitting quad hanging clear of floor and cube: the smallest list
        pass
    elif name == "glow_cube":      # the cube emits onto the floor: half its faces hidden from any hit, reached < rays
        s.update(model=[ec._plain(cube), gloss_common._floor(ref_loader, cube)], emissive_parts={0: (2.0, 1.5, 1.0)}, eye=(2.3, 1.5, 3.1), target=(0.0, -0.3, 0.0),
                 w=72, h=48)
    elif name == "suzanne_lamp":   # suzanne emits: 111 faces, a deep search, concave self-occlusion
        s.update(model=[ec._plain(suzanne), gloss_common._floor(ref_loader, cube)], emissive_parts={0: (1.0, 2.0, 3.0)}, eye=(1.6, 1.2, 3.4),
                 target=(0.0, -0.2, 0.0), w=64, h=40)
    elif name == "two_parts":      # two emitting parts of different Le and area: inv_pdf differs per face
        s.update(model=[room, _panel(ref_loader, cube), _panel(ref_loader, cube, x=(-2.6, -1.8), y=1.4, z=(-0.2, 1.0))],
                 emissive_parts={1: (8.0, 7.0, 5.0), 2: (1.0, 3.0, 9.0)}, w=80, h=56)
    elif name == "panel_and_lamp":  # both flags, one emitting sphere and the panel: cone and face samples diverge within a wave; M = 1, L = 2
        s.update(spheres=rwr.make_spheres([LAMP]), emissive_spheres={0: (8.0, 7.0, 5.0)}, light=True)
    elif name == "panel_two_lamps":  # both flags, two emitting spheres and a dark one between them: L = 3
        s.update(spheres=rwr.make_spheres([LAMP, ((0.0, 1.4, 0.2), 0.3), ((-1.8, 0.1, 1.0), 0.45)]), emissive_spheres={0: (6.0, 2.0, 1.0), 2: (1.0, 3.0, 7.0)},
                 light=True, w=72, h=48)
    elif name == "parts_only":     # the new flag with an emitting sphere present but RWR_FLAG_LIGHT_SAMPLING off: the sphere keeps Le, is not aimed at
        s.update(spheres=rwr.make_spheres([LAMP]), emissive_spheres={0: (8.0, 7.0, 5.0)})
    elif name == "mirror_panel":   # a mirror cube: its rays hit the panel and keep Le
        s.update(model=[ec._plain(cube), gloss_common._floor(ref_loader, cube), _panel(ref_loader, cube)], mirror_parts={0: (0.9, 0.9, 0.9)},
                 emissive_parts={2: PANEL_LE})
    elif name == "tiny":           # 5 x 3, a partial tile
        s.update(w=5, h=3, bounces=1)
    elif name == "bare_panel":     # the floor, the panel and a dark sphere between them, no cube: a BVH small enough for LDS beside 32-bit stacks
        s.update(model=[gloss_common._floor(ref_loader, cube), _panel(ref_loader, cube)], spheres=rwr.make_spheres([((0.2, 0.2, 0.1), 0.6)]), w=48, h=32)
    elif name == "bare_lamp":      # the same without the panel, lit by an emitting sphere: RWR_FLAG_LIGHT_SAMPLING's own scene of that size
        s.update(model=gloss_common._floor(ref_loader, cube), spheres=rwr.make_spheres([LAMP, ((0.2, 0.2, 0.1), 0.6)]), emissive_parts={},
                 emissive_spheres={0: (8.0, 7.0, 5.0)}, light=True, w=48, h=32)
    elif name == "grid":           # 4 x 4 instances of an emitting suzanne: nodelets out of LDS, a list of 16 x 111 faces
        s.update(model=ec._plain(suzanne), instances=rwr.make_instance_grid(4, 3.0), emissive_parts={0: (0.5, 0.4, 0.3)}, eye=(6.5, 3.0, 6.5),
                 target=(0.0, 0.0, 0.0), w=56, h=36)
    elif name == "large":          # large_scenes' parts_large, 13 712 world faces, its cubes emitting: 32-bit stacks chosen by the plan
        model, spheres, inst, eye, target, _ = large_scenes.scene("parts_large", rwr, orc, ref_loader, suzanne, cube)
        s.update(model=[model[0], ec._plain(model[1])], spheres=np.ascontiguousarray(spheres).view(rwr.make_spheres([]).dtype), instances=inst.view(rwr.make_instance_grid(1, 1.0).dtype),
                 eye=eye, target=target, emissive_parts={1: (3.0, 2.0, 1.0)}, w=72, h=48)
    else:
        raise KeyError(name)
    _cache[key] = s
    return s


# the scenes of the GPU parity test; test_part_light_host.py states what each is there for
SCENES = ("panel", "glow_cube", "suzanne_lamp", "two_parts", "panel_and_lamp", "panel_two_lamps", "parts_only", "mirror_panel", "tiny", "bare_panel", "grid", "large")
SPPS = {"grid": (2,), "large": (2,)}     # the others: emission_common.SPPS

n_parts = ec.n_parts
camera = ec.camera
BAR_FACTOR = 64.0     # a frame with the mesh light: g is bounded by the term's cap alone


def spps(name):
    return SPPS.get(name, ec.SPPS)


def flags(rwr, s, bounces=None, parts=True, light=None, emissive=True, extra=0) -> int:
    light = s["light"] if light is None else light
    return lc.flags(rwr, s, bounces=bounces, light=light, emissive=emissive, extra=extra | (rwr.FLAG_LIGHT_PARTS if parts else 0))


def reference(L, rwr, orc, s, seed, spp, name, parts=True, light=None, bounces=None, entry="parts", shadows=None) -> dict:
    """The CPU reference's frame of scene s, kept for the session (never modified by a test).  parts=False: the frame without
    RWR_FLAG_LIGHT_PARTS, by the same loop; entry="light": light_render_path's frame."""
    bounces = s["bounces"] if bounces is None else bounces
    shadows = s["shadows"] if shadows is None else shadows
    light = s["light"] if light is None else light
    key = ("ref", name, seed, spp, bounces, parts, light, entry, shadows)
    if key not in _cache:
        inst = None if s["instances"] is None else s["instances"].view(orc.INSTANCE_DTYPE)
        kw = dict(parts=parts) if entry == "parts" else {}
        _cache[key] = part_light_ref.render_path(L, orc, camera(rwr, s).view(orc.CAMERA_INV_DTYPE), orc.make_screen(s["w"], s["h"]),
                                                 orc.make_params(spp, bounces, seed=seed), s["spheres"].view(orc.SPHERE_DTYPE), s["model"],
                                                 emissive_parts=s["emissive_parts"], emissive_spheres=s["emissive_spheres"], light=light, entry=entry,
                                                 instances=inst, shadows=shadows, sky=ec.sky_of(s) if bounces else None,
                                                 mirror_parts=s["mirror_parts"] if bounces else None, glass_spheres=s["glass_spheres"] if bounces else None,
                                                 gloss_parts=s["gloss_parts"] if bounces else None, **kw)
    return _cache[key]
