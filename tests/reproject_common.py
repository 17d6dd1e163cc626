"""The sequences the reprojection tests share (tests/test_reproject_host.py asserts with the CPU reference alone that each of them
exercises what the GPU file, tests/test_gpu_reproject.py, relies on): a scene, a start camera and a list of
rwr_circle_controller_update key steps - or direct camera literals where the controller cannot make the move.

Small frames: 64x48, 80x56, 37x29 and 5x3 (the last two are no multiple of the stage's 64x4 workgroup nor of the integrator's 64x8
tile), 1-4 spp, at most two bounces."""
import numpy as np

import glass_ref
import path_cases
import world_offset_common

SEED = 21
NAMES = ("still", "orbit", "dolly", "occluder", "turn_away", "instances", "spheres_only", "far", "all_flags", "tiny")
CUBE_SPHERE = ((1.6, 1.2, 1.4), 0.5)     # shadow_common's "cube" scene
CUBE_EYE = (2.2, 1.7, 3.1)
NEAR_EYE = (1.5, 1.1, 2.0)               # the cube overflows a 4:3 frame from here
_cache = {}


def _steps(rwr, w, h, eye, target, steps, fovy=60.0):
    """The start camera, then one camera per key step: steps = [(keys, count, speed), ...]."""
    cam = rwr.make_camera(eye=eye, target=target, aspect=w / h, fovy=fovy)
    cams = [cam]
    for keys, count, speed in steps:
        for _ in range(count):
            cam = rwr.circle_controller_update(cam, keys, speed)
            cams.append(cam)
    return cams


def _literals(rwr, w, h, poses, fovy=60.0):
    return [rwr.make_camera(eye=e, target=t, aspect=w / h, fovy=fovy) for e, t in poses]


def sequence(name, rwr, orc, suzanne, cube) -> dict:
    """model (one model or a list of parts), spheres, instances, w, h, spp, bounces, cams (camera records, one per frame), shadows,
    sky ((zenith, horizon) or None), mirror_spheres / glass_spheres."""
    if name in _cache:
        return _cache[name]
    R, L, F, B = rwr.KEY_RIGHT, rwr.KEY_LEFT, rwr.KEY_FORWARD, rwr.KEY_BACKWARD
    s = dict(name=name, model=cube, spheres=rwr.make_spheres([CUBE_SPHERE]), instances=None, spp=2, bounces=1, shadows=False, sky=None,
             mirror_spheres={}, glass_spheres={})
    if name == "still":          # nothing moves for nine frames: frame 8 is the one the error is measured on
        s.update(w=64, h=48, cams=_steps(rwr, 64, 48, NEAR_EYE, (0, 0, 0), [(0, 8, 0.2)]))
    elif name == "orbit":        # sideways steps about the cube, which overflows the frame: taps fall outside it
        s.update(w=64, h=48, cams=_steps(rwr, 64, 48, NEAR_EYE, (0, 0, 0), [(R, 8, 0.05)]))
    elif name == "dolly":        # towards and away: te differs from t
        s.update(w=80, h=56, spp=1, cams=_steps(rwr, 80, 56, CUBE_EYE, (0, 0, 0), [(F, 3, 0.2), (B, 3, 0.2)]))
    elif name == "occluder":     # a sphere near the eye sweeps across the cube while the camera orbits: disocclusion behind it
        s.update(w=80, h=56, spheres=rwr.make_spheres([((1.25, 1.0, 1.8), 0.22)]),
                 cams=_steps(rwr, 80, 56, CUBE_EYE, (0, 0, 0), [(R, 4, 0.1)]))
    elif name == "turn_away":    # inside the cube: a small turn, then one of more than 90 degrees - the points lie behind the previous camera
        eye = (0.1, 0.2, 0.3)
        s.update(w=37, h=29, spheres=rwr.make_spheres([]), spp=1, bounces=0,
                 cams=_literals(rwr, 37, 29, [(eye, (0.1, 0.2, -0.7)), (eye, (0.25, 0.2, -0.7)), (eye, (1.0, 0.3, 1.2))]))
    elif name == "instances":    # rotated instances: nhat of world faces; a cube face's two triangles pass the normal rule
        inst = path_cases.instances(rwr, [path_cases._rotation(a, t) for a, t in (((1, 1, 0), 0.7), ((0, 1, 1), 2.1), ((1, 0, 1), 4.0))],
                                    [(-3.1, 0.0, 0.0), (0.0, 0.2, 0.0), (3.1, -0.1, 0.3)])
        s.update(w=80, h=56, instances=inst, spheres=rwr.make_spheres([((0.0, 2.3, 0.4), 0.6)]),
                 cams=_steps(rwr, 80, 56, (0.4, 1.7, 5.2), (0, 0, 0), [(R, 3, 0.05)]))
    elif name == "spheres_only":  # the mesh is behind the camera: only the two spheres are seen
        s.update(w=37, h=29, spheres=rwr.make_spheres(), spp=4, cams=_steps(rwr, 37, 29, (0.5, 0.45, -1.6), (0.5, 0.45, -4.0), [(L, 2, 0.1), (F, 1, 0.2)]))
    elif name == "far":          # the orbit 1e4 from the origin on every axis
        off = np.asarray(world_offset_common.OFFSETS["1e4"], np.float64)
        at = lambda p: tuple(np.asarray(p, np.float64) + off)   # noqa: E731
        s.update(w=64, h=48, model=world_offset_common.translated(cube, off), spheres=rwr.make_spheres([(at(CUBE_SPHERE[0]), CUBE_SPHERE[1])]),
                 cams=_steps(rwr, 64, 48, at(CUBE_EYE), at((0, 0, 0)), [(R, 4, 0.05)]))
    elif name == "all_flags":    # shadows, sky, a mirror sphere, a glass sphere, two bounces
        s.update(w=37, h=29, model=suzanne, spheres=rwr.make_spheres(), bounces=2, shadows=True, sky=((0.5, 0.7, 1.0), (1.0, 1.0, 1.0)),
                 mirror_spheres={0: (0.9, 0.9, 0.9)}, glass_spheres={1: (1.5, (1.0, 1.0, 1.0))},
                 cams=_steps(rwr, 37, 29, (2.5, 0.5, 1.0), (0, 0, 0), [(R, 2, 0.1), (F, 1, 0.2)]))
    elif name == "tiny":         # smaller than a wave: 5 x 3
        s.update(w=5, h=3, cams=_steps(rwr, 5, 3, NEAR_EYE, (0, 0, 0), [(0, 1, 0.2), (R, 2, 0.05)]))
    else:
        raise KeyError(name)
    s["cam_invs"] = [rwr.camera_build_inv_uniform(c) for c in s["cams"]]
    _cache[name] = s
    return s


def cpu_frame(gref, rwr, orc, s, cam_inv, seed, spp=None, bounces=None) -> dict:
    """The CPU path reference's frame of sequence s under one camera: the planes of c_now."""
    inst = None if s["instances"] is None else s["instances"].view(orc.INSTANCE_DTYPE)
    return glass_ref.render_path(gref, orc, cam_inv.view(orc.CAMERA_INV_DTYPE), orc.make_screen(s["w"], s["h"]),
                                 orc.make_params(s["spp"] if spp is None else spp, s["bounces"] if bounces is None else bounces, seed=seed),
                                 s["spheres"].view(orc.SPHERE_DTYPE), s["model"], instances=inst, shadows=s["shadows"], sky=s["sky"],
                                 mirror_spheres=s["mirror_spheres"] or None, glass_spheres=s["glass_spheres"] or None)


def cpu_frames(gref, rwr, orc, s, seed=SEED, spp=None, bounces=None) -> list:
    """Frame k of the sequence as it is traced: seed + k.  Kept for the session (never modified by a test)."""
    key = ("cpu", s["name"], seed, spp, bounces)
    if key not in _cache:
        _cache[key] = [cpu_frame(gref, rwr, orc, s, cam, (seed + k) & 0xffffffff, spp, bounces) for k, cam in enumerate(s["cam_invs"])]
    return _cache[key]


def gpu_flags(rwr, s) -> int:
    return ((rwr.FLAG_MULTI_BOUNCE if s["bounces"] > 1 else 0) | (rwr.FLAG_SHADOWS if s["shadows"] else 0) | (rwr.FLAG_SKY if s["sky"] else 0) |
            (rwr.FLAG_MIRRORS if s["mirror_spheres"] else 0) | (rwr.FLAG_GLASS if s["glass_spheres"] else 0))


def upload(ctx, s):
    """The sequence's scene and screen into a context."""
    if isinstance(s["model"], (list, tuple)):
        ctx.upload_parts(s["model"])
    else:
        ctx.upload_model(s["model"])
    ctx.set_instances(s["instances"])
    ctx.set_spheres(s["spheres"])
    for i, r in s["mirror_spheres"].items():
        ctx.set_sphere_mirror(i, r)
    for i, (ior, tint) in s["glass_spheres"].items():
        ctx.set_sphere_glass(i, ior, tint)
    if s["sky"]:
        ctx.sky_set_params(*s["sky"])
    ctx.resize(s["w"], s["h"])
