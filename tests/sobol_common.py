"""The scenes the tests of the Sobol sample sequence (RWR_FLAG_SOBOL) share, taken from the other features' common modules and
completed to one shape, and the reference frames, computed once per session by tests/sobol_ref.py's switched library.

A scene: emission_common.scene's entries plus "light" / "parts" / "mis" (the three light flags its frames carry), "radii" (soft
shadows: the two lights' radii, or None) and "sky" ((zenith, horizon), or None)."""
import emission_common as ec
import emission_ref
import gloss_common
import mis_common
import sobol_ref

_cache = {}
DEFAULT_SKY = (emission_ref.glass_ref.DEFAULT_ZENITH, emission_ref.glass_ref.DEFAULT_HORIZON)
# name -> (module, its scene's name): the GPU parity test's scenes
PARITY = {"tiny": ("emission", "tiny"), "floor": ("gloss", "floor"), "room": ("emission", "room"), "shadowed": ("emission", "shadowed"),
          "with_models": ("emission", "with_models"), "instances": ("emission", "instances"), "panel_and_lamp": ("mis", "panel_and_lamp"),
          "soft_sky": (None, None)}
SPP_PLANS = ((1, 1), (2, None), (33, None))   # (spp, bounces; None: the scene's): spp 1 with a bounce, 2, and 33, which crosses a launch group unevenly


def scene(name, rwr, ref_loader, suzanne, cube, orc=None) -> dict:
    key = ("scene", name)
    if key in _cache:
        return _cache[key]
    base = dict(shadows=False, emissive_parts={}, emissive_spheres={}, light=False, parts=False, mis=False, radii=None)
    if name == "cube":          # the denoise host test's frame: the cube alone, 64 x 48, one bounce, no sky
        s = dict(base, instances=None, fovy=60.0, gloss_parts={}, gloss_spheres={}, glass_parts={}, glass_spheres={}, mirror_parts={}, mirror_spheres={},
                 spheres=rwr.make_spheres([]), model=cube, eye=(1.4, 1.0, 1.9), target=(0.0, 0.0, 0.0), w=64, h=48, bounces=1, sky=None)
    elif name == "lamp_room":   # the emission tests' lamp-lit room with sphere light sampling and MIS
        s = dict(base, **ec.scene("room", rwr, ref_loader, suzanne, cube))
        s.update(light=True, mis=True, sky=None)
    elif name == "soft_sky":    # the room's model without the lamp, under the default sky, soft shadow rays of radii 0.1
        r = ec.scene("room", rwr, ref_loader, suzanne, cube)
        s = dict(base, **r)
        s.update(spheres=rwr.make_spheres([]), emissive_spheres={}, shadows=True, radii=(0.1, 0.1), sky=DEFAULT_SKY)
    else:
        module, theirs = PARITY[name]
        if module == "emission":
            s = dict(base, **ec.scene(theirs, rwr, ref_loader, suzanne, cube))
            s["sky"] = ec.sky_of(s)
        elif module == "gloss":
            s = dict(base, **gloss_common.scene(theirs, rwr, ref_loader, suzanne, cube))
            s["sky"] = DEFAULT_SKY
        else:
            s = dict(base, **mis_common.scene(theirs, rwr, ref_loader, suzanne, cube, orc))
            s.update(mis=True, sky=ec.sky_of(s))
    _cache[key] = s
    return s


camera = gloss_common.camera


def emits(s) -> bool:
    return bool(s["emissive_parts"] or s["emissive_spheres"])


def bar_factor(s) -> float:
    """The colour bar scales with the largest Le where something emits (the emission and light tests' rule)."""
    return max(1.0, ec.max_le(s))


def flags(rwr, s, bounces=None, sobol=True, extra=0) -> int:
    b = s["bounces"] if bounces is None else bounces
    f = rwr.FLAG_AUX_OUTPUTS | extra | (rwr.FLAG_SOBOL if sobol else 0) | (rwr.FLAG_MULTI_BOUNCE if b > 1 else 0)
    f |= (rwr.FLAG_SHADOWS if s["shadows"] else 0) | (rwr.FLAG_SOFT_SHADOWS if s["shadows"] and s["radii"] else 0) | (rwr.FLAG_SKY if s["sky"] else 0)
    f |= (rwr.FLAG_MIRRORS if s["mirror_parts"] else 0) | (rwr.FLAG_GLASS if s["glass_spheres"] else 0) | (rwr.FLAG_GLOSSY if s["gloss_parts"] else 0)
    f |= (rwr.FLAG_EMISSIVE if emits(s) else 0) | (rwr.FLAG_LIGHT_SAMPLING if s["light"] else 0) | (rwr.FLAG_LIGHT_PARTS if s["parts"] else 0)
    return f | (rwr.FLAG_LIGHT_MIS if s["mis"] else 0)


def render(L, rwr, orc, s, seed, spp, bounces=None, sobol=True, by=None) -> dict:
    """One frame of scene s by the CPU reference, not kept.  L: sobol_ref.lib's library; by=mis_ref.render_path with mis_ref's own
    library renders the hashed frame by the reference as it is committed."""
    b = s["bounces"] if bounces is None else bounces
    inst = None if s["instances"] is None else s["instances"].view(orc.INSTANCE_DTYPE)
    kw = dict(emissive_parts=s["emissive_parts"], emissive_spheres=s["emissive_spheres"]) if emits(s) else {}
    if by is None:
        by, kw["sobol"] = sobol_ref.render_path, sobol
    return by(L, orc, camera(rwr, s).view(orc.CAMERA_INV_DTYPE), orc.make_screen(s["w"], s["h"]), orc.make_params(spp, b, seed=seed),
              s["spheres"].view(orc.SPHERE_DTYPE), s["model"], light=s["light"], parts=s["parts"], mis=s["mis"], instances=inst, shadows=s["shadows"],
              radii=s["radii"] if s["shadows"] else None, sky=s["sky"] if b else None, mirror_parts=s["mirror_parts"] if b else None,
              glass_spheres=s["glass_spheres"] if b else None, gloss_parts=s["gloss_parts"] if b else None, **kw)


def reference(L, rwr, orc, s, seed, spp, name, bounces=None, sobol=True) -> dict:
    """The CPU reference's frame of scene s, kept for the session (never modified by a test).  L: sobol_ref.lib's library."""
    b = s["bounces"] if bounces is None else bounces
    key = ("ref", name, seed, spp, b, sobol)
    if key not in _cache:
        _cache[key] = render(L, rwr, orc, s, seed, spp, bounces=b, sobol=sobol)
    return _cache[key]
