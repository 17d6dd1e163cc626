"""The scenes the tests of multiple importance sampling for the light rays share (tests/test_mis_host.py asserts with the CPU reference
alone that each of them exercises what the GPU file, tests/test_gpu_mis.py, relies on), and the reference frames, computed once per
session.  part_light_common's scenes are reused; a scene here also says which of the two light flags its frames carry ("light":
RWR_FLAG_LIGHT_SAMPLING, "parts": RWR_FLAG_LIGHT_PARTS) beside RWR_FLAG_LIGHT_MIS."""
import emission_common as ec
import gloss_common
import light_common as lc
import mis_ref
import part_light_common as pc
import path_cases

_cache = {}
REUSED = ("panel", "glow_cube", "suzanne_lamp", "two_parts", "panel_and_lamp", "panel_two_lamps", "parts_only", "tiny", "bare_panel", "bare_lamp", "grid", "large")
FLOOR_Y = -1.3     # gloss_common._floor's


def scene(name, rwr, ref_loader, suzanne, cube, orc=None) -> dict:
    """part_light_common.scene's entries plus "parts".  No scene is larger than 80 x 56."""
    key = ("scene", name)
    if key in _cache:
        return _cache[key]
    if name in REUSED:
        s = dict(pc.scene(name, rwr, ref_loader, suzanne, cube, orc))
        s["parts"] = bool(s["emissive_parts"])
    else:
        s = dict(pc.scene("panel", rwr, ref_loader, suzanne, cube, orc), parts=True)
        floor = gloss_common._floor(ref_loader, cube, r=2.5)
        if name == "crease":       # an emitting wall that stands on the plain floor's far edge: receivers touch the emitter, g grows as 1 / d2
            wall = path_cases._quad(ref_loader, cube["texture"], [(-2.5, FLOOR_Y, -2.5), (2.5, FLOOR_Y, -2.5), (2.5, 0.7, -2.5), (-2.5, 0.7, -2.5)])
            s.update(model=[floor, wall], emissive_parts={1: (4.0, 3.5, 2.5)}, eye=(0.5, -0.3, -0.3), target=(0.0, -1.0, -2.5))
        elif name == "big_lamp":   # an emitting sphere 1.1 above the floor with R = 1: R / d = 0.91 below it, the cone fills most of the hemisphere
            s.update(model=floor, spheres=rwr.make_spheres([((0.2, FLOOR_Y + 1.1, 0.3), 1.0)]), emissive_parts={}, emissive_spheres={0: (2.0, 1.75, 1.25)},
                     light=True, parts=False, eye=(0.9, -0.6, 2.1), target=(0.2, -1.0, 0.3))
        elif name == "inside":     # an emitting sphere of glass that cuts the floor: refracted rays find the floor inside it, where no sample is taken
            s.update(model=gloss_common._merged(cube, gloss_common._floor(ref_loader, cube)), spheres=rwr.make_spheres([((1.9, FLOOR_Y + 0.3, 0.9), 0.8)]),
                     emissive_parts={}, emissive_spheres={0: (2.0, 1.5, 1.0)}, glass_spheres={0: (1.5, (1.0, 1.0, 1.0))}, light=True, parts=False, bounces=3,
                     eye=(2.3, 0.0, 2.4), target=(1.7, -1.0, 0.7))
        else:
            raise KeyError(name)
    _cache[key] = s
    return s


# the scenes of the GPU parity test; test_mis_host.py states what each is there for
SCENES = REUSED + ("crease", "big_lamp", "inside")

n_parts = ec.n_parts
camera = ec.camera
max_le = ec.max_le


def spps(name):
    return pc.SPPS.get(name, ec.SPPS)


def bar_factor(s) -> float:
    """The largest value a light term can take under the flag, T Le m <= Le (item 4): max(1, largest Le component of the scene)."""
    return max(1.0, max_le(s))


def flags(rwr, s, bounces=None, mis=True, parts=None, light=None, emissive=True, extra=0) -> int:
    light = s["light"] if light is None else light
    parts = s["parts"] if parts is None else parts
    return lc.flags(rwr, s, bounces=bounces, light=light, emissive=emissive,
                    extra=extra | (rwr.FLAG_LIGHT_PARTS if parts else 0) | (rwr.FLAG_LIGHT_MIS if mis else 0))


def reference(L, rwr, orc, s, seed, spp, name, mis=True, parts=None, light=None, bounces=None, entry="mis", shadows=None) -> dict:
    """The CPU reference's frame of scene s, kept for the session (never modified by a test).  mis=False: the frame without
    RWR_FLAG_LIGHT_MIS, by the same loop; entry="parts": part_light_render_path's frame."""
    bounces = s["bounces"] if bounces is None else bounces
    shadows = s["shadows"] if shadows is None else shadows
    light = s["light"] if light is None else light
    parts = s["parts"] if parts is None else parts
    key = ("ref", name, seed, spp, bounces, mis, parts, light, entry, shadows)
    if key not in _cache:
        inst = None if s["instances"] is None else s["instances"].view(orc.INSTANCE_DTYPE)
        kw = dict(mis=mis) if entry == "mis" else {}
        _cache[key] = mis_ref.render_path(L, orc, camera(rwr, s).view(orc.CAMERA_INV_DTYPE), orc.make_screen(s["w"], s["h"]),
                                          orc.make_params(spp, bounces, seed=seed), s["spheres"].view(orc.SPHERE_DTYPE), s["model"],
                                          emissive_parts=s["emissive_parts"], emissive_spheres=s["emissive_spheres"], light=light, parts=parts, entry=entry,
                                          instances=inst, shadows=shadows, sky=ec.sky_of(s) if bounces else None,
                                          mirror_parts=s["mirror_parts"] if bounces else None, glass_spheres=s["glass_spheres"] if bounces else None,
                                          gloss_parts=s["gloss_parts"] if bounces else None, **kw)
    return _cache[key]
