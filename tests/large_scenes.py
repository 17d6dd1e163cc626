"""Scenes beyond the per-lane BVH kernels' 16-bit traversal stacks (csrc/rwr_bvh.h lane_lds_plan: 16-bit entries up to 4 095 world
faces and 32 767 nodes, 32-bit entries beyond), shared by tests/test_large_scenes_host.py - which asserts with the CPU reference
alone that every frame below can fail - and tests/test_gpu_large_scenes.py.  Test infrastructure; everything is deterministic
from the seeds written here.

scene(name, ...) is shadow_common.scene's tuple (model or parts, spheres, instances, eye, target, extra flags); MARKS[name] the
surface marks a frame may take with it, by variant, in the keyword shape of soft_shadow_ref.render_path.  FRAMES lists every frame
the GPU file renders against the reference (parts a and b of its docstring); reference() keeps each for the session."""
import numpy as np

import fuzz_common
import soft_shadow_ref as ssr

STACK16_MAX_FACES = 4095          # lane_lds_plan's limit
RADII = ((0.2, 0.2), (0.3, 0.0))  # tests/test_gpu_soft_shadows.py's pairs
SKY = ((0.5, 0.7, 1.0), (1.0, 1.0, 1.0))   # no component above 1: path_cases.color_bar's factor is 1
SOUP_FACES = 4096
SOUP_SEED, PARTS_SEED = 4096, 3000
SOUP_LAST_FROM = 888   # the face the soups' camera sees on most pixels is made the last one: the frames of 4 095 and 4 096 faces differ
ROUGH_LOW, ROUGH_HIGH = 2.0 ** -10, 0.9375   # the setters' lower end, and near 1

_cache = {}


def slab(ref_loader, seed, n_faces, tex, half=(2.2, 2.2, 0.35), tri_size=0.16, last_from=None):
    """fuzz_common.soup, its cube of centres pressed into a thin slab across z (the mesh light stands at (-1, 1, 5) / sqrt(27): a
    shadow ray leaves a slab sooner than a ball, and a camera off the slab sees faces of every index)."""
    model = fuzz_common.soup(ref_loader, np.random.default_rng(seed), n_faces, extent=1.0, tri_size=tri_size, tex=tex)
    rng = np.random.default_rng(seed + 1)
    centres = rng.uniform(-1.0, 1.0, (n_faces, 1, 3)) * np.asarray(half)
    shape = rng.normal(0.0, tri_size, (n_faces, 3, 3))
    pos = centres + shape
    if last_from is not None:   # the face drawn as number last_from changes places with the last one
        pos[[last_from, n_faces - 1]] = pos[[n_faces - 1, last_from]]
    model["vertices"]["position"] = pos.reshape(-1, 3).astype(np.float32)
    return model


def first_faces(model, n):
    """The model's first n faces (a soup: three vertices of its own per face)."""
    m = dict(model)
    m["vertices"], m["faces"] = model["vertices"][:3 * n].copy(), model["faces"][:n].copy()
    return m


def scene(name, rwr, orc, ref_loader, suzanne, cube):
    key = ("scene", name)
    if key in _cache:
        return _cache[key]
    ref_spheres = orc.make_spheres()
    tex = suzanne["texture"]
    if name in ("soup_4095", "soup_4096"):
        soup = _cache.setdefault("soup", slab(ref_loader, SOUP_SEED, SOUP_FACES, tex, last_from=SOUP_LAST_FROM))
        model = soup if name == "soup_4096" else first_faces(soup, SOUP_FACES - 1)
        s = (model, orc.make_spheres([((0.5, 0.3, 0.9), 0.45), ((-0.9, -0.6, 0.8), 0.35)]), None, (0.9, -1.4, 2.1), (0.0, 0.0, 0.0), 0)
    elif name in ("cube_grid4", "cube_grid4_nmap"):
        grid = rwr.make_instance_grid(4, 3.0).view(orc.INSTANCE_DTYPE)
        s = (cube, ref_spheres, grid, (3.0, 4.0, 0.5), (-0.5, 0.0, -3.5), orc.FLAG_NORMAL_MAP if name.endswith("nmap") else 0)
    elif name == "parts_large":
        soup = slab(ref_loader, PARTS_SEED, 3000, tex, half=(1.3, 0.25, 1.3), tri_size=0.12)
        soup["vertices"]["position"] += np.array([0.0, 1.6, 0.0], np.float32)    # a canopy of small faces above the cube
        soup["material"]["ambient"] = (0.10, 0.06, 0.02)
        grid = rwr.make_instance_grid(2, 3.0).view(orc.INSTANCE_DTYPE)
        spheres = orc.make_spheres([((0.3, 0.3, 1.3), 0.45), ((-2.2, 0.2, 1.4), 0.4)])   # in front of the near cubes
        s = ([soup, cube], spheres, grid, (1.4, 1.2, 2.6), (-1.5, 0.3, -1.5), 0)
    else:
        raise KeyError(name)
    _cache[key] = s
    return s


SIZES = {"soup_4095": (96, 64), "soup_4096": (96, 64), "cube_grid4": (96, 64), "cube_grid4_nmap": (96, 64), "parts_large": (90, 60)}   # 90 x 60: partial 64 x 8 tiles
N_FACES = {"soup_4095": 4095, "soup_4096": 4096, "cube_grid4": 6848, "cube_grid4_nmap": 6848, "parts_large": 4 * (3000 + 428)}

# variant -> marks.  One model per surface within a variant.  parts_large: part 0 the soup, part 1 the cube; cube_grid4: the one part.
_R, _TINT = (0.9, 0.8, 0.7), (0.95, 0.9, 1.0)
MARKS = {
    "parts_large": {
        "mirror": dict(mirror_parts={1: _R}, mirror_spheres={0: (0.9, 0.9, 0.9)}),
        "glass": dict(glass_parts={1: (1.5, _TINT)}, glass_spheres={1: (1.33, (1.0, 1.0, 1.0))}),
        "gloss": dict(gloss_parts={1: (ROUGH_LOW, _R)}, gloss_spheres={0: (ROUGH_HIGH, (0.8, 0.9, 1.0))}),
        "all": dict(mirror_spheres={0: (0.9, 0.9, 0.9)}, glass_parts={1: (1.5, _TINT)}, gloss_parts={0: (ROUGH_HIGH, _R)},
                    gloss_spheres={1: (ROUGH_LOW, (0.8, 0.9, 1.0))}),
    },
    "cube_grid4": {
        "mirror": dict(mirror_parts={0: _R}, mirror_spheres={0: (0.9, 0.9, 0.9)}),
        "glass": dict(glass_parts={0: (1.5, _TINT)}, glass_spheres={1: (1.33, (1.0, 1.0, 1.0))}),
        "gloss": dict(gloss_parts={0: (ROUGH_LOW, _R)}, gloss_spheres={0: (ROUGH_HIGH, (0.8, 0.9, 1.0))}),
        # (sphere 1 lies inside a cube: only a ray that glass let through finds it)
        "all": dict(mirror_spheres={0: (0.9, 0.9, 0.9)}, glass_parts={0: (1.5, _TINT)}, gloss_spheres={1: (ROUGH_HIGH, (0.8, 0.9, 1.0))}),
    },
}


def _frame(scene_, spp, bounces, shadows=False, radii=None, sky=False, variant=None, seed=13):
    return dict(scene=scene_, spp=spp, bounces=bounces, shadows=shadows or radii is not None, radii=radii, sky=sky, variant=variant, seed=seed)


def _ladder(name):
    """Part b's ladder on one scene: the plain path at depth 0, 1 and 4, then hard shadows, both pairs of soft radii, sky, each
    surface model alone and all three together (with soft shadows and sky on)."""
    out = [_frame(name, 2, 0), _frame(name, 2, 1), _frame(name, 2, 4),
           _frame(name, 2, 0, shadows=True), _frame(name, 2, 4, shadows=True),
           _frame(name, 2, 4, radii=RADII[0]), _frame(name, 3, 1, radii=RADII[1]),
           _frame(name, 2, 4, radii=RADII[0], sky=True)]
    out += [_frame(name, 2, 4, radii=RADII[0], sky=True, variant=v) for v in ("mirror", "glass", "gloss", "all")]
    return out


LIMIT = [_frame(n, 3, 4, shadows=True, radii=r, sky=True) for n in ("soup_4095", "soup_4096") for r in (None,) + RADII]
LADDER = _ladder("cube_grid4") + _ladder("parts_large") + [_frame("cube_grid4_nmap", 2, 1, shadows=True)]
# parts c and e of the GPU file, at depth 3: the schedule sweep's frame (soft shadows, a glossy part; five samples: two launch groups of
# three or four) and the frame the splits and the accumulation are held to (four samples: 2 x 2)
SCHEDULES = _frame("cube_grid4", 5, 3, radii=RADII[0], variant="gloss", seed=3)
SPLITS = _frame("cube_grid4", 4, 3, radii=RADII[0], seed=11)
FRAMES = LIMIT + LADDER + [SCHEDULES, SPLITS]


def describe(f) -> str:
    return (f"{f['scene']} spp {f['spp']} B {f['bounces']} shadows {int(f['shadows'])} radii {f['radii']} sky {int(f['sky'])} "
            f"surfaces {f['variant']}")


def marks(f) -> dict:
    return MARKS[f["scene"]][f["variant"]] if f["variant"] else {}


def camera(rwr, orc, sc, w, h):
    return rwr.camera_build_inv_uniform(rwr.make_camera(eye=sc[3], target=sc[4], aspect=w / h, fovy=60.0)).view(orc.CAMERA_INV_DTYPE)


def reference(L, rwr, orc, ref_loader, suzanne, cube, f, **over) -> dict:
    """soft_shadow_ref.c's frame of f (kept for the session; never modified by a test), with the coverage counts of its radii.
    over: spp, bounces, seed, rows, variant marks as keywords."""
    key = ("ref", describe(f), f["seed"], tuple(sorted((k, str(v)) for k, v in over.items())))
    if key not in _cache:
        sc = scene(f["scene"], rwr, orc, ref_loader, suzanne, cube)
        w, h = SIZES[f["scene"]]
        kw = dict(marks(f))
        kw.update({k: v for k, v in over.items() if k not in ("spp", "bounces", "seed")})
        _cache[key] = ssr.reference(L, orc, sc, camera(rwr, orc, sc, w, h), w, h, over.get("spp", f["spp"]), over.get("bounces", f["bounces"]),
                                    seed=over.get("seed", f["seed"]), radii=f["radii"], shadows=f["shadows"], sky=SKY if f["sky"] else None,
                                    coverage=f["radii"] is not None, **kw)
    return _cache[key]


def world_corners(orc, sc) -> np.ndarray:
    """The scene's world faces as (n, 9) float32 corners in the oracle's order - face = instance * base faces + base face - by the
    oracle's own instancing rule (rt_oracle.c: world = model * vec4(p, 1), float32 products summed left to right)."""
    model, inst = sc[0], sc[2]
    flat = orc.concat_parts(list(model) if isinstance(model, (list, tuple)) else [model])
    pos = flat["vertices"]["position"].astype(np.float32)
    idx = flat["faces"]["indices"]
    if inst is None or len(inst) == 0:
        return np.ascontiguousarray(pos[idx].reshape(len(idx), 9))
    out = []
    for m in np.ascontiguousarray(inst, dtype=orc.INSTANCE_DTYPE)["model"]:   # m[column][row]
        m = m.astype(np.float32)
        x, y, z = pos[:, 0:1], pos[:, 1:2], pos[:, 2:3]
        q = ((m[0, :3] * x + m[1, :3] * y) + m[2, :3] * z) + m[3, :3] * np.float32(1.0)
        out.append(q.astype(np.float32)[idx].reshape(len(idx), 9))
    return np.ascontiguousarray(np.concatenate(out))


def skewed_corners() -> np.ndarray:
    """tests/test_gpu_random.py's 6 000-face scene (a dense cluster plus far outliers), drawn the way that test draws it: its
    binned-SAH tree is deeper than the traversal stacks, so build_bvh rebuilds it with object-median splits."""
    rng = np.random.default_rng(42)
    n = 6000
    scale = np.where(np.arange(n) % 50 == 0, 1000.0 * 2.0 ** (np.arange(n) % 13), 1.0)[:, None, None]
    centers = scale * rng.uniform(-1, 1, (n, 1, 3))
    rng.uniform(-1.0, 1.0, (n, 1, 3)); rng.normal(0, 0.05, (n, 3, 3)); rng.uniform(-0.2, 1.2, (3 * n, 2))   # (the soup that test draws first)
    return np.ascontiguousarray((centers + rng.normal(0, 0.05, (n, 3, 3))).reshape(n, 9).astype(np.float32))
