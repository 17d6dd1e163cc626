"""The scenes the tests of the light rays aimed at the sky's image share (RWR_FLAG_LIGHT_SKY), their flags, and the reference frames,
computed once per session and never modified.  A scene is an emission_common scene dict (model, spheres, surfaces, emitters, camera,
size, bounces) plus "spp" and the two light flags its frames carry beside the new one ("light", "parts")."""
import numpy as np

import emission_common as ec
import gloss_common
import part_light_common as pc
import sky_light_ref

_cache = {}
SUN = sky_light_ref.sun_map()            # n = 16: 0.05 everywhere, a 2 x 2 sun of 40 in the upper hemisphere
SCENES = ("cube_b1", "cube_b8", "soup", "cube_grid", "lamp_panel_sun")


def _soup(ref_loader, cube):
    import shadow_common
    rng = np.random.default_rng(11)
    centre = rng.uniform(-1.2, 1.2, size=(60, 1, 3))
    tris = centre + rng.normal(scale=0.45, size=(60, 3, 3))
    return shadow_common.triangle_model(ref_loader, [tuple(map(tuple, t)) for t in tris.astype(np.float32)], cube["texture"])


def scene(name, rwr, ref_loader, suzanne, cube, orc=None) -> dict:
    key = ("scene", name)
    if key in _cache:
        return _cache[key]
    s = dict(instances=None, fovy=45.0, gloss_parts={}, gloss_spheres={}, glass_parts={}, glass_spheres={}, mirror_parts={}, mirror_spheres={},
             spheres=rwr.make_spheres([]), bounces=1, shadows=False, emissive_parts={}, emissive_spheres={}, light=False, parts=False)
    if name == "cube_b1":       # L = 1: no choice is drawn
        s.update(model=cube, eye=(1.0, 0.8, 1.4), target=(0, 0, 0), w=64, h=48, spp=4, bounces=1)
    elif name == "cube_b8":
        s.update(model=cube, eye=(1.0, 0.8, 1.4), target=(0, 0, 0), w=64, h=48, spp=4, bounces=8)
    elif name == "soup":        # an odd size: partial tiles; sphere 0 a mirror, whose reflected rays are unmarked and keep S
        s.update(model=_soup(ref_loader, cube), spheres=rwr.make_spheres([((0.9, 0.4, 0.6), 0.5), ((-0.8, -0.5, 0.2), 0.35)]), eye=(0.3, 0.5, 2.2),
                 target=(0, 0, 0), w=37, h=29, spp=5, bounces=3, mirror_spheres={0: (1.0, 1.0, 1.0)})
    elif name == "cube_grid":   # 64 samples: pools dense enough for the packet kernel and its miss sites
        s.update(model=cube, instances=rwr.make_instance_grid(2, 3.0), eye=(-1.5, 1.5, 2.5), target=(-1.5, 0.0, -1.5), w=64, h=48, spp=64, bounces=2)
    elif name == "sunlit":      # the tests' floor and cube, no emitter, lit by the sun map alone
        s.update(model=gloss_common._merged(cube, gloss_common._floor(ref_loader, cube)), eye=(2.1, 1.2, 3.3), target=(0.0, -0.6, 0.0), fovy=60.0,
                 w=64, h=48, spp=4, bounces=2)
    elif name == "lamp_panel_sun":   # an emitting sphere and an emitting part beside the sun: all three light flags, L = 3
        s.update({k: v for k, v in pc.scene("panel_and_lamp", rwr, ref_loader, suzanne, cube, orc).items()})
        s.update(spp=4, light=True, parts=True)
    elif name == "bare_lamp_sun":    # part_light_common's floor under an emitting sphere: a BVH small enough for LDS beside 32-bit stacks; SKY without PARTS
        s.update({k: v for k, v in pc.scene("bare_lamp", rwr, ref_loader, suzanne, cube, orc).items()})
        s.update(spp=4, light=True, parts=False)
    elif name == "bare_panel_sun":   # the same under the emitting panel: SKY with PARTS
        s.update({k: v for k, v in pc.scene("bare_panel", rwr, ref_loader, suzanne, cube, orc).items()})
        s.update(spp=4, light=False, parts=True)
    else:
        raise KeyError(name)
    _cache[key] = s
    return s


camera = ec.camera


def flags(rwr, s, sky_light=True, mis=True, image=True, sky=True, bounces=None, extra=0) -> int:
    bounces = s["bounces"] if bounces is None else bounces
    emits = bool(s["emissive_parts"] or s["emissive_spheres"])
    f = rwr.FLAG_AUX_OUTPUTS | extra | (rwr.FLAG_MULTI_BOUNCE if bounces > 1 else 0) | (rwr.FLAG_SHADOWS if s["shadows"] else 0)
    f |= (rwr.FLAG_SKY if sky else 0) | (rwr.FLAG_SKY_IMAGE if image else 0) | (rwr.FLAG_LIGHT_SKY if sky_light else 0)
    f |= (rwr.FLAG_MIRRORS if s["mirror_parts"] or s["mirror_spheres"] else 0) | (rwr.FLAG_EMISSIVE if emits else 0)
    f |= (rwr.FLAG_LIGHT_SAMPLING if s["light"] else 0) | (rwr.FLAG_LIGHT_PARTS if s["parts"] else 0) | (rwr.FLAG_LIGHT_MIS if mis else 0)
    return f


def bar_factor(s, image, mis) -> float:
    """With RWR_FLAG_LIGHT_MIS every light term is at most T * max(S, Le) <= the largest component; without it a term may reach the cap."""
    return max(1.0, float(np.max(image)), ec.max_le(s)) if mis else 64.0


def reference(L, rwr, orc, s, seed, name, image=SUN, sky_light=True, mis=True, spp=None, bounces=None) -> dict:
    """The CPU reference's frame of scene s under `image`, kept for the session.  sky_light=False: the frame under the image without
    the new flag, by the same loop (mis then weights the scene's other lights alone)."""
    spp = s["spp"] if spp is None else spp
    bounces = s["bounces"] if bounces is None else bounces
    key = ("ref", id(L), name, seed, spp, bounces, sky_light, mis, None if image is None else image.tobytes())
    if key not in _cache:
        inst = None if s["instances"] is None else s["instances"].view(orc.INSTANCE_DTYPE)
        _cache[key] = sky_light_ref.render_path(L, orc, camera(rwr, s).view(orc.CAMERA_INV_DTYPE), orc.make_screen(s["w"], s["h"]),
                                                orc.make_params(spp, bounces, seed=seed), s["spheres"].view(orc.SPHERE_DTYPE), s["model"],
                                                image=image, sky_light=sky_light, mis=mis,
                                                emissive_parts=s["emissive_parts"] or None, emissive_spheres=s["emissive_spheres"] or None,
                                                light=s["light"], parts=s["parts"], instances=inst, shadows=s["shadows"],
                                                mirror_spheres=s["mirror_spheres"] or None, mirror_parts=s["mirror_parts"] or None)
    return _cache[key]
