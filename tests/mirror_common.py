"""The scenes the mirror tests share (tests/test_mirror_host.py asserts with the CPU reference alone that each of them exercises
what the GPU file, tests/test_gpu_mirror.py, relies on), and the reference frames, computed once per session."""
import numpy as np

import mirror_ref
import shadow_common

QUAD_R = (0.5, 0.75, 1.0)
_cache = {}


def _quad(ref_loader, cube, y=-1.3, half=3.5):
    """One upward-facing quad (two triangles wound so that their normal is +y) in the plane y = const."""
    a, b, c, d = (-half, y, -half), (-half, y, half), (half, y, half), (half, y, -half)
    return shadow_common.triangle_model(ref_loader, [(a, b, c), (a, c, d)], cube["texture"])


def _soup(ref_loader, cube):
    """tests/test_gpu_sky.py's soup: about 60 triangles of all sizes and orientations in a box around the origin."""
    rng = np.random.default_rng(11)
    centre = rng.uniform(-1.2, 1.2, size=(60, 1, 3))
    tris = centre + rng.normal(scale=0.45, size=(60, 3, 3))
    return shadow_common.triangle_model(ref_loader, [tuple(map(tuple, t)) for t in tris.astype(np.float32)], cube["texture"])


def _two_parts(cube):
    """The cube and a copy of it beside it, their faces dealt to two parts with materials of their own: the first half of each
    cube's faces is part 0, the second half part 1.  (A lone convex mesh would never see itself in its mirror faces.)"""
    v = cube["vertices"]
    v2 = v.copy()
    v2["position"] = v["position"] + np.array([2.7, 0.35, -0.5], np.float32)
    verts = np.concatenate([v, v2])
    f = cube["faces"]
    f2 = f.copy()
    f2["indices"] = f["indices"] + len(v)
    n = len(f) // 2
    parts = []
    for k, faces in enumerate((np.concatenate([f[:n], f2[:n]]), np.concatenate([f[n:], f2[n:]]))):
        mat = cube["material"].copy()
        mat["ambient"] = (0.12, 0.03, 0.02) if k == 0 else (0.02, 0.04, 0.15)
        parts.append({"vertices": verts, "faces": faces, "material": mat, "texture": cube["texture"]})
    return parts


def _split_cube(cube):
    """The cube's faces dealt to two parts with materials of their own (both carry every vertex)."""
    f = cube["faces"]
    n = len(f) // 2
    parts = []
    for k, faces in enumerate((f[:n], f[n:])):
        mat = cube["material"].copy()
        mat["ambient"] = (0.12, 0.03, 0.02) if k == 0 else (0.02, 0.04, 0.15)
        parts.append({"vertices": cube["vertices"], "faces": faces.copy(), "material": mat, "texture": cube["texture"]})
    return parts


def scene(name, rwr, ref_loader, suzanne, cube) -> dict:
    """model (one model or a list of parts), spheres, instances, eye, target, w, h, spp, bounces, mirror_parts, mirror_spheres"""
    key = ("scene", name)
    if key in _cache:
        return _cache[key]
    none = rwr.make_spheres([])
    if name == "quad_alone":   # the closed form: every primary hit reflects into the sky
        s = dict(model=_quad(ref_loader, cube), spheres=none, instances=None, eye=(0.4, 1.1, 3.0), target=(0, -1.3, 0), w=16, h=12, spp=1,
                 bounces=1, mirror_parts={0: QUAD_R}, mirror_spheres={})
    elif name == "quad_floor":
        s = dict(model=[_quad(ref_loader, cube), cube], spheres=none, instances=None, eye=(2.4, 1.6, 3.4), target=(0, -0.6, 0), w=64, h=48,
                 spp=4, bounces=2, mirror_parts={0: QUAD_R}, mirror_spheres={})
    elif name == "soup":       # an odd size: partial tiles; sphere normals
        s = dict(model=_soup(ref_loader, cube), spheres=rwr.make_spheres([((0.9, 0.4, 0.6), 0.5), ((-0.8, -0.5, 0.2), 0.35)]), instances=None,
                 eye=(0.3, 0.5, 2.2), target=(0, 0, 0), w=37, h=29, spp=5, bounces=3, mirror_parts={0: (0.9, 0.6, 0.3)},
                 mirror_spheres={0: (0.25, 1.0, 0.8)})
    elif name == "two_parts":  # lanes of one wave on mirror and on diffuse faces; the part from ShadeRec::material
        s = dict(model=_two_parts(cube), spheres=none, instances=None, eye=(3.2, 1.9, 3.6), target=(1.2, 0, 0), w=64, h=48, spp=4, bounces=8,
                 mirror_parts={1: (1.0, 0.5, 0.75)}, mirror_spheres={})
    elif name == "cube_grid":  # 64 samples: pools dense enough for the packet kernel
        s = dict(model=cube, spheres=none, instances=rwr.make_instance_grid(2, 3.0), eye=(-1.5, 1.5, 2.5), target=(-1.5, 0.0, -1.5), w=64, h=48,
                 spp=64, bounces=2, mirror_parts={0: (0.8, 0.9, 1.0)}, mirror_spheres={})
    elif name == "parts_grid":  # instances of a mesh of two parts, one of them a mirror: a world face's part is its base face's
        s = dict(model=_split_cube(cube), spheres=none, instances=rwr.make_instance_grid(2, 3.0), eye=(-1.5, 1.5, 2.5), target=(-1.5, 0.0, -1.5),
                 w=64, h=48, spp=4, bounces=2, mirror_parts={1: (0.6, 1.0, 0.8)}, mirror_spheres={})
    elif name == "suzanne":    # the reference's scene: its two spheres beside the mesh, seen from where both spheres show
        s = dict(model=suzanne, spheres=rwr.make_spheres(), instances=None, eye=(3.2, 1.4, -1.2), target=(0.2, 0.2, -2.2), w=200, h=72, spp=7,
                 bounces=2, mirror_parts={}, mirror_spheres={1: (1.0, 1.0, 1.0)})
    else:
        raise KeyError(name)
    _cache[key] = s
    return s


GPU_SCENES = ("quad_floor", "soup", "two_parts", "cube_grid", "suzanne", "parts_grid")


def n_parts(s) -> int:
    return len(s["model"]) if isinstance(s["model"], (list, tuple)) else 1


def camera(rwr, s, w=None, h=None):
    w, h = w or s["w"], h or s["h"]
    return rwr.camera_build_inv_uniform(rwr.make_camera(eye=s["eye"], target=s["target"], aspect=w / h))


def reference(L, rwr, orc, s, seed, mirrors=True, sky=None, shadows=False, spp=None, bounces=None, first=False, name=None) -> dict:
    """The CPU reference's frame of scene s, kept for the session (never modified by a test)."""
    spp, bounces = spp or s["spp"], s["bounces"] if bounces is None else bounces
    key = ("ref", name or id(s), seed, mirrors, sky, shadows, spp, bounces, first)
    if key not in _cache:
        inst = None if s["instances"] is None else s["instances"].view(orc.INSTANCE_DTYPE)
        _cache[key] = mirror_ref.render_path(L, orc, camera(rwr, s).view(orc.CAMERA_INV_DTYPE), orc.make_screen(s["w"], s["h"]),
                                             orc.make_params(spp, bounces, seed=seed), s["spheres"].view(orc.SPHERE_DTYPE), s["model"],
                                             instances=inst, shadows=shadows, sky=sky, first=first,
                                             mirror_parts=s["mirror_parts"] if mirrors else None,
                                             mirror_spheres=s["mirror_spheres"] if mirrors else None)
    return _cache[key]
