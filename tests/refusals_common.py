"""The sweep of render calls and of surface entry point calls whose (return code, error message) pairs are recorded in
tests/golden/render_refusals.json: shared by the generator (tests/golden/make_render_refusals.py, run against a build of the
commit BEFORE the host units were split) and by tests/test_gpu_render_refusals.py, so both walk the same calls in the same order.

Also a model of validate's rules for the swept calls, written from include/rwr_hip.h and the order DESIGN.md records, not from
the library: which rules refuse a call, in the order they are checked."""
import itertools
import os


FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_refusals.json")
W, H = 64, 16
SWEPT_FLAGS = ("ACCUMULATE", "SHADOWS", "DENOISE", "REPROJECT", "SKY", "MIRRORS", "GLASS", "GLOSSY")   # validate's order
EXTRAS = ("none", "ORTHO_RAYS", "USE_BVH", "triangles")
ROWS = (None, (0, 8))
BOUNCES = (0, 1)
SYNC_EVERY = 256
OFF_REFERENCE = "RWR_FLAG_%s: RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes apply to the reference frame only"
PART_FRAME = {"DENOISE": "RWR_FLAG_DENOISE: the filter needs the whole frame (its taps reach 62 pixels); rows [0,8) every 1-th strip is a part of it",
              "REPROJECT": "RWR_FLAG_REPROJECT: the stage needs the whole frame (its taps land anywhere in the previous one); rows [0,8) "
                           "every 1-th strip is a part of it"}
BVH_TEXT = "RWR_FLAG_USE_BVH applies to the reference frame (spp 1, no bounce); bounce rays always use the BVH"
TWO_HISTORIES = "RWR_FLAG_REPROJECT with RWR_FLAG_ACCUMULATE: a context blends one history, not two"
DORMANT_TEXT = "single-triangle passes and RWR_FLAG_ORTHO_RAYS apply to the reference frame (spp 1, no bounce, no RWR_FLAG_USE_BVH)"
# every refusal of validate that depends on the call's flags, rows and bounces (the others test the arguments alone: ARGUMENT_CASES)
FLAG_REFUSALS = ([BVH_TEXT, TWO_HISTORIES, DORMANT_TEXT] + [OFF_REFERENCE % f for f in SWEPT_FLAGS] + [PART_FRAME["DENOISE"], PART_FRAME["REPROJECT"]])


def sweep_cases():
    """4 096 cases (extra, subset of SWEPT_FLAGS as a bit mask, rows, max_bounces), the single-triangle set outermost so that the
    scene changes twice in the sweep."""
    return list(itertools.product(EXTRAS, range(256), ROWS, BOUNCES))


def rules_refusing(case):
    """The texts of the rules that refuse `case`, in validate's order (spp is 1 and RWR_FLAG_MULTI_BOUNCE is not set)."""
    extra, subset, rows, bounces = case
    on = [f for i, f in enumerate(SWEPT_FLAGS) if subset >> i & 1]
    out = []
    if extra == "USE_BVH" and bounces:
        out.append(BVH_TEXT)
    for f in on:
        if f == "REPROJECT" and "ACCUMULATE" in on:
            out.append(TWO_HISTORIES)
        if extra != "none":
            out.append(OFF_REFERENCE % f)
        if f in PART_FRAME and rows is not None:
            out.append(PART_FRAME[f])
    wavefront = bounces != 0 or any(f in on for f in ("ACCUMULATE", "SHADOWS", "DENOISE", "REPROJECT"))
    if extra in ("ORTHO_RAYS", "triangles") and wavefront:
        out.append(DORMANT_TEXT)
    return out


def make_scene(rwr):
    """One context: the cube at 64 x 16, the reference's two spheres; sphere 0 a mirror, sphere 1 glass, part 0 glossy."""
    ctx = rwr.Context(0)
    ctx.upload_model(rwr.load_model_compute("cube.obj"))
    ctx.set_spheres(rwr.make_spheres())
    ctx.resize(W, H)
    ctx.set_sphere_mirror(0, (0.9, 0.8, 0.7))
    ctx.set_sphere_glass(1, 1.5, (1.0, 0.9, 0.8))
    ctx.set_part_gloss(0, 0.25, (0.8, 0.8, 0.9))
    return ctx


def _pair(fn):
    """(return code, message) of one call through the package: (0, "") when it was accepted."""
    try:
        fn()
    except Exception as e:   # rwr.RwrError (the package is loaded under another name by the generator)
        return [int(e.code), str(e.message)]
    return [0, ""]


def run_sweep(rwr, ctx):
    """The pairs of all cases, in sweep order."""
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0, 0, 3), aspect=W / H))
    triangle = rwr.make_triangles([((-1.0, -1.0, -2.0), (1.0, -1.0, -2.0), (0.0, 1.0, -2.0))])
    pairs = []
    for i, (extra, subset, rows, bounces) in enumerate(sweep_cases()):
        if i % 1024 == 0:   # the first case of an `extra` block
            ctx.set_triangles(triangle if extra == "triangles" else rwr.make_triangles())
        flags = sum(getattr(rwr, "FLAG_" + f) for k, f in enumerate(SWEPT_FLAGS) if subset >> k & 1)
        if extra in ("ORTHO_RAYS", "USE_BVH"):
            flags |= getattr(rwr, "FLAG_" + extra)
        params = rwr.make_params(spp=1, max_bounces=bounces, seed=0, flags=flags)
        pairs.append(_pair(lambda: ctx.render(cam_inv, params, rows=rows)))
        if (i + 1) % SYNC_EVERY == 0:
            ctx.synchronize()
    ctx.set_triangles(rwr.make_triangles())
    ctx.synchronize()
    return pairs


# Calls validate refuses for their arguments alone: (name, make_params keywords, rows)
ARGUMENT_CASES = [
    ("spp 0", dict(spp=0), None),
    ("spp 4097", dict(spp=4097), None),
    ("max_bounces 9 with MULTI_BOUNCE", dict(max_bounces=9, flags=1 << 6), None),
    ("max_bounces 2 without MULTI_BOUNCE", dict(max_bounces=2), None),
    ("USE_BVH at spp 2", dict(spp=2, flags=4), None),
    ("rows [8,4)", dict(), (8, 4)),
    ("rows [0,17)", dict(), (0, 17)),
]


def run_argument_cases(rwr, ctx):
    cam_inv = rwr.camera_build_inv_uniform(rwr.make_camera(eye=(0, 0, 3), aspect=W / H))
    return {name: _pair(lambda: ctx.render(cam_inv, rwr.make_params(**kw), rows=rows)) for name, kw, rows in ARGUMENT_CASES}


NAN = float("nan")
SURFACE_ENTRY_POINTS = [f"{verb}_{owner}_{model}" for model in ("mirror", "glass", "gloss") for verb in ("set", "get") for owner in ("part", "sphere")]


def surface_error_calls(entry):
    """The refused calls of one surface entry point (a Context method's name): [(label, args)].  Index out of range for both
    owners (the scene has one part; 8 sphere indices), and for the setters every range check of the model's values, at both
    ends and with NaN."""
    verb, owner, model = entry.split("_")
    bad = 1 if owner == "part" else 8
    if verb == "get":
        return [(f"index {bad}", (bad,)), ("index 2^32 - 1", (0xffffffff,))]
    rgb_bad = [(0.5, 1.5, 0.5), (-0.25, 0.5, 0.5), (0.5, 0.5, NAN)]
    calls = [(f"index {bad}", (bad,))]
    if model == "mirror":
        calls += [(f"reflectance {v}", (0, v)) for v in rgb_bad]
    elif model == "glass":
        calls += [(f"ior {v}", (0, v, (1.0, 1.0, 1.0))) for v in (0.5, 4.5, NAN)]
        calls += [(f"tint {v}", (0, 1.5, v)) for v in rgb_bad]
        calls += [("ior 0.5 and tint[0] 2", (0, 0.5, (2.0, 0.0, 0.0)))]   # two faults: the ior's refusal comes first
    else:
        calls += [(f"roughness {v}", (0, v, (1.0, 1.0, 1.0))) for v in (0.0, 2.0 ** -11, 1.5, NAN)]
        calls += [(f"reflectance {v}", (0, 0.25, v)) for v in rgb_bad]
        calls += [("roughness 2 and reflectance[0] 2", (0, 2.0, (2.0, 0.0, 0.0)))]
    return calls


def run_surface_errors(ctx, entry):
    return [[label] + _pair(lambda: getattr(ctx, entry)(*args)) for label, args in surface_error_calls(entry)]
