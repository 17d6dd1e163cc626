"""The frames of tests/golden/surface_frames.json: what tests/golden/make_surface_frames.py records from a build of the commit before
the surface table got its module (csrc/rwr_surface.h) and tests/test_gpu_surface_frames.py renders again.  The integrator's frames
are bit-reproducible (integer sums, no contraction), so a frame is held to a SHA-256 per plane and to its four event counters.

Every frame: 200 x 72 pixels (3 1/8 tiles wide, 9 tall: partial tiles on the right edge), 4 spp, 4 bounces, seed 11, one frame in
flight.  The scene: suzanne_lowpoly.obj with the two reference spheres, part 0 glossy (roughness 0.25), sphere 0 glass (ior 1.5),
sphere 1 a mirror.  Two cameras: the reference camera, inside the mesh, and eye (0, 0, 3).  Flags {MIRRORS}, {MIRRORS, GLASS},
{MIRRORS, GLASS, GLOSSY}, each x shadows off / on x sky off / on; then one frame with the normal map on (cube.obj) and one with
RWR_FLAG_AUX_OUTPUTS, both with all three surface flags.

What those 26 frames turned out not to reach when they were recorded, and the frames added for it:
  * at this size the sort classes every pool of either camera for the per-lane kernel, so the reference camera's twelve frames are
    rendered once more under the schedule tests/test_gpu_fuzz.py forces (path_cases.FORCED_SCHEDULE: every pool traced as packets);
  * neither camera sees a sphere (the frames with and without RWR_FLAG_GLASS are the same frames), so the three sets of flags are
    rendered from tools/gloss_probe.py's side camera too, with both spheres in view, shadows and sky on;
  * a ray that entered a glass sphere never meets its surface beyond the critical angle, so one frame has cube.obj's part 0 as
    glass: the only total internal reflections of the set."""
import hashlib
import os

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "surface_frames.json")
W, H, SPP, BOUNCES, SEED = 200, 72, 4, 4, 11
CAMERAS = {"inside": dict(eye=(0, 0, 0), target=(0, 0, -1)), "front": dict(eye=(0, 0, 3), target=(0, 0, -1)),
           "side": dict(eye=(3.2, 1.4, -1.2), target=(0.2, 0.2, -2.2)), "cube": dict(eye=(2.2, 1.7, 3.1), target=(0, 0, 0))}
# every pool traced as packets, launch groups of five samples (path_cases.FORCED_SCHEDULE); read when a context is created
PACKETS = {"RWR_WF_GROUP": "5", "RWR_WF_PACKET_FILL": "0", "RWR_WF_PACKET_EXTENT": "1e30", "RWR_WF_MIN_PACKET_POOLS": "0"}
SURFACE_SETS = (("mirrors",), ("mirrors", "glass"), ("mirrors", "glass", "glossy"))
COUNTERS = ("reflected", "transmitted", "totally_reflected", "glossy")


def frames():
    """[{name, scene, camera, packets, part0, surfaces, shadows, sky, normal_map, aux}] in the order they are rendered."""
    out = []

    def add(name, camera, surfaces, shadows=False, sky=False, scene="suzanne_lowpoly.obj", packets=False, part0="gloss", normal_map=False, aux=False):
        out.append(dict(name=name, scene=scene, camera=camera, packets=packets, part0=part0, surfaces=surfaces, shadows=shadows, sky=sky,
                        normal_map=normal_map, aux=aux))

    for camera, packets in (("inside", False), ("front", False), ("inside", True)):
        for surfaces in SURFACE_SETS:
            for shadows in (False, True):
                for sky in (False, True):
                    add(f"{camera}{'-packets' if packets else ''}-{'+'.join(surfaces)}{'-shadows' if shadows else ''}{'-sky' if sky else ''}",
                        camera, surfaces, shadows, sky, packets=packets)
    for surfaces in SURFACE_SETS:
        add(f"side-{'+'.join(surfaces)}-shadows-sky", "side", surfaces, True, True)
    every = SURFACE_SETS[-1]
    add("cube-normal-map", "cube", every, scene="cube.obj", normal_map=True)
    add("cube-glass-part", "cube", every, scene="cube.obj", part0="glass")
    add("inside-aux", "inside", every, aux=True)
    return out


def context_key(f):
    """Frames with the same key share a context."""
    return (f["scene"], f["packets"], f["part0"])


def flags_of(rwr, f):
    return (rwr.FLAG_MULTI_BOUNCE | (rwr.FLAG_MIRRORS if "mirrors" in f["surfaces"] else 0) | (rwr.FLAG_GLASS if "glass" in f["surfaces"] else 0) |
            (rwr.FLAG_GLOSSY if "glossy" in f["surfaces"] else 0) | (rwr.FLAG_SHADOWS if f["shadows"] else 0) | (rwr.FLAG_SKY if f["sky"] else 0) |
            (rwr.FLAG_NORMAL_MAP if f["normal_map"] else 0) | (rwr.FLAG_AUX_OUTPUTS if f["aux"] else 0))


def make_ctx(rwr, key, stats=False):
    """A context of its own for the frames of context_key `key`: the scene, the schedule, the three surfaces set.  stats:
    RWR_WF_STATS=1, the context prints its account of pools and launches when it is destroyed."""
    scene, packets, part0 = key
    env = dict(PACKETS if packets else {}, **({"RWR_WF_STATS": "1"} if stats else {}))
    saved = {k: os.environ.get(k) for k in list(PACKETS) + ["RWR_WF_STATS"]}
    try:
        for k in saved:
            os.environ.pop(k, None)
        os.environ.update(env)
        ctx = rwr.Context(0)   # the tunables are read here
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    ctx.upload_model(rwr.load_model_compute(scene))
    ctx.set_spheres(rwr.make_spheres())
    ctx.resize(W, H)
    ctx.set_frames_in_flight(1)
    if part0 == "glass":
        ctx.set_part_glass(0, 1.5, (0.9, 0.8, 0.7))
    else:
        ctx.set_part_gloss(0, 0.25, (0.9, 0.8, 0.7))
    ctx.set_sphere_glass(0, 1.5, (0.9, 1.0, 0.9))
    ctx.set_sphere_mirror(1, (0.8, 0.8, 0.9))
    return ctx


def render(rwr, ctx, f):
    """{"planes": {plane: SHA-256 of its bytes}, "counters": [reflected, transmitted, totally reflected, glossy]} of frame f."""
    cam = rwr.camera_build_inv_uniform(rwr.make_camera(aspect=W / H, **CAMERAS[f["camera"]]))
    ctx.render(cam, rwr.make_params(spp=SPP, max_bounces=BOUNCES, seed=SEED, flags=flags_of(rwr, f)))
    out = ctx.readback(aux=f["aux"])
    planes = ("color", "depth", "obj_id", "hit_t") if f["aux"] else ("color", "depth")
    return dict(planes={p: hashlib.sha256(out[p].tobytes()).hexdigest() for p in planes},
                counters=[int(c) for c in ctx.last_glass_stats()] + [int(ctx.last_gloss_stats())])
