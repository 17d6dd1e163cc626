"""Scenes far from the world origin, and the float64 audit of how far the oracle's literal hits stray outside their faces
(test infrastructure: tests/test_world_offset_margin.py on the CPU, tests/test_gpu_world_offset.py on the GPU).

The exact hit test (oracle/rt_oracle.c triangle_ray_intersect, which the GPU reproduces bit for bit) rounds at WORLD
magnitude: -dot(N, p0), dot(N, O) + d and t*D + O.  Far from the origin a "hit" can therefore lie outside its face by
more than a pixel, and the conservative culling of csrc/rwr_cull.h may drop a face only where no such hit can happen.
`audit` restates the culling's margins (make_frame_tri, compute_cull_consts, the whole-mesh rectangle) in float64, with
the half-pixel guard between tile bounds and pixel centres, and measures every oracle hit against them."""
import numpy as np

KCULL_REL = 2.002e-5                  # kCullRel with compute_cull_consts' 1.001
KCULL_WORLD = 12.0 * 5.9604645e-8     # kCullWorld
KCULL_DEGENERATE = 1e-4

OFFSETS = {"0": (0.0, 0.0, 0.0), "1e3": (1e3, 1e3, 1e3), "1e4": (1e4, 1e4, 1e4), "3e4": (3e4, -2e4, 1e4), "1e5": (1e5, 1e5, 1e5)}


def translated(model, offset, scale=1.0, center=None):
    """A copy of `model` moved by `offset` (and scaled by `scale` about `center`), rounded to f32 once."""
    m = dict(model)
    v = model["vertices"].copy()
    p = v["position"].astype(np.float64)
    c = np.zeros(3) if center is None else np.asarray(center, np.float64)
    v["position"] = ((p - c) * scale + c + np.asarray(offset, np.float64)).astype(np.float32)
    m["vertices"] = v
    return m


def spheres_at(rwr, offset, spec=None):
    spec = rwr.REFERENCE_SPHERES if spec is None else spec
    return rwr.make_spheres([(tuple(np.asarray(c, np.float64) + np.asarray(offset, np.float64)), r) for c, r in spec])


def camera(rwr, eye, target, offset, w, h, fovy=60.0):
    o = np.asarray(offset, np.float64)
    cam = rwr.make_camera(eye=tuple(np.asarray(eye, np.float64) + o), target=tuple(np.asarray(target, np.float64) + o), aspect=w / h, fovy=fovy)
    return rwr.camera_build_inv_uniform(cam)


def _dirs(cam_inv, fx, fy, w, h):
    """compute_cull_consts' dir(fx, fy): the un-normalised ray direction through pixel-space point (fx, fy), in float64."""
    P = cam_inv["proj_inv"][0].astype(np.float64)      # [column][row]
    V = cam_inv["viewmodel_inv"][0].astype(np.float64)
    xn, yn = 2.0 * np.asarray(fx, np.float64) / w - 1.0, 2.0 * np.asarray(fy, np.float64) / h - 1.0
    v = xn[..., None] * P[0] + yn[..., None] * P[1] + P[2] + P[3]
    return v[..., 0:1] * V[0, :3] + v[..., 1:2] * V[1, :3] + v[..., 2:3] * V[2, :3]


def cull_consts(cam_inv, w, h):
    """compute_cull_consts in float64 (the GPU rounds these to f32; the margins' 1.001 factors cover that)."""
    A = _dirs(cam_inv, 0.0, 0.0, w, h)
    Bx = (_dirs(cam_inv, float(w), 0.0, w, h) - A) / w
    By = (_dirs(cam_inv, 0.0, float(h), w, h) - A) / h
    Ux, Vx, Uy, Vy = np.cross(A, By), np.cross(Bx, By), np.cross(A, Bx), np.cross(By, Bx)
    sx, sy = (-1.0 if Ux @ Bx < 0 else 1.0), (-1.0 if Uy @ By < 0 else 1.0)
    Ux, Vx, Uy, Vy = sx * Ux, sx * Vx, sy * Uy, sy * Vy
    corners = _dirs(cam_inv, np.array([0.0, w, w, 0.0]), np.array([0.0, 0.0, h, h]), w, h)
    dmax = float(np.abs(corners).sum(-1).max())
    vxa, vya = float(Vx @ A), float(Vy @ A)
    l1 = lambda a: float(np.abs(a).sum())   # noqa: E731
    O = cam_inv["origin"][0][:3].astype(np.float64)
    return dict(A=A, Bx=Bx, By=By, Ux=Ux, Vx=Vx, Uy=Uy, Vy=Vy, vxa=vxa, vya=vya, dmax=dmax, O=O, o_l1=l1(O),
                corner_margin=KCULL_REL * dmax,
                gx=(l1(Ux) + (w + 1.0) * l1(Vx)) * dmax / abs(vxa), gy=(l1(Uy) + (h + 1.0) * l1(Vy)) * dmax / abs(vya),
                kk=max(l1(Vx) / abs(vxa), l1(Vy) / abs(vya)) * dmax)


def face_rho(cc, p):
    """rwr_cull.h world_rho for faces p[..., 3 corners, 3] (float64); +inf where the bound does not hold."""
    q = p - cc["O"]
    e0 = np.cross(q[:, 0], q[:, 1])
    vol = np.einsum("ij,ij->i", e0, q[:, 2])
    delta = KCULL_WORLD * (cc["o_l1"] + np.abs(p).sum(-1).max(-1))
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    nl1 = np.abs(np.cross(a, b)).sum(-1) + 1e-6 * np.abs(a).sum(-1) * np.abs(b).sum(-1)
    dist = np.maximum(np.abs(vol) / nl1, np.maximum(q.min(1), -q.max(1)).max(-1)) * 0.999
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(dist > 2.0 * delta, delta / (dist - delta), np.inf), delta


def mesh_rho(cc, lo, hi):
    mag = np.maximum(np.abs(lo), np.abs(hi)).sum()
    dist = max(0.0, float(np.maximum(lo - cc["O"], cc["O"] - hi).max())) * 0.999
    delta = KCULL_WORLD * (cc["o_l1"] + mag)
    return delta / (dist - delta) if dist > 2.0 * delta else np.inf


def audit(cam_inv, w, h, fovy, model, frame, world_term=True):
    """Every pixel the oracle's `frame` shows a face of `model` at: how far its centre ray passes outside that face, in
    pixels (float64, the issue's measure: min over the edges of s (q_i x q_j).D / |q_i x q_j| over the angle of a
    pixel), and the worst ratio of stray to margin granted, for the edge functions, the face rectangle and the whole-mesh
    rectangle.  world_term=False restates the margins without rwr_cull.h's world-magnitude term (rho = 0).
    A ratio <= 1 everywhere means no culling test can drop a face at a pixel where the oracle hits it."""
    ids = frame["obj_id"]
    ys, xs = np.nonzero(ids >= 0)
    out = {"pixels": int(len(ys)), "stray_px": np.zeros(0), "edge": 0.0, "rect": 0.0, "mesh": 0.0, "unbounded": 0.0}
    if not len(ys):
        return out
    cc = cull_consts(cam_inv, w, h)
    pos = model["vertices"]["position"].astype(np.float64)
    tri = pos[model["faces"]["indices"].astype(np.int64)]          # [faces, 3, 3]
    rho_all, _ = face_rho(cc, tri)
    if not world_term:
        rho_all = np.zeros_like(rho_all)
    f = ids[ys, xs].astype(np.int64)
    p, rho = tri[f], rho_all[f]
    fx, fy = xs + 0.5, ys + 0.5
    D = _dirs(cam_inv, fx, fy, w, h)
    q = p - cc["O"]
    e = np.stack([np.cross(q[:, 0], q[:, 1]), np.cross(q[:, 1], q[:, 2]), np.cross(q[:, 2], q[:, 0])], 1)
    vol = np.einsum("ij,ij->i", e[:, 0], q[:, 2])
    s = np.where(vol > 0, 1.0, -1.0)[:, None]
    d = s * np.einsum("ikj,ij->ik", e, D)                          # d_i at the pixel centre
    en = np.linalg.norm(e, axis=-1)
    pix_angle = np.deg2rad(fovy) / h
    with np.errstate(divide="ignore", invalid="ignore"):
        out["stray_px"] = -np.nanmin(d / en, axis=1) / np.linalg.norm(D, axis=-1) / pix_angle
    world_ok = rho * cc["kk"] <= 0.5
    out["unbounded"] = float(1.0 - world_ok.mean())   # share of the hit pixels whose face the world bound leaves unculled
    reliable = world_ok & (np.abs(vol) > KCULL_DEGENERATE * np.abs(e[:, 0]).sum(-1) * np.abs(q[:, 2]).sum(-1))
    me = cc["corner_margin"] * (1.0 + rho[:, None] / KCULL_REL) * np.abs(e).sum(-1)
    granted = 0.5 * (np.abs(s * (e @ cc["Bx"])) + np.abs(s * (e @ cc["By"]))) + me
    with np.errstate(invalid="ignore"):
        ratio = np.where(reliable[:, None] & (d < 0), -d / granted, 0.0)
    out["edge"] = float(np.nan_to_num(ratio, nan=np.inf).max())
    # the face's rectangle: pixel-space projections of its corners (all in front), padded, against the pixel's square
    vx, vy = q @ cc["Vx"], q @ cc["Vy"]
    front = (vx / cc["vxa"] > 1e-5 * np.abs(q).sum(-1) * np.abs(cc["Vx"]).sum() / abs(cc["vxa"])).all(1) & world_ok
    px_, py_ = -(q @ cc["Ux"]) / vx, -(q @ cc["Uy"]) / vy
    rect = 0.0
    for c, lo, hi, g in ((fx, px_.min(1), px_.max(1), cc["gx"]), (fy, py_.min(1), py_.max(1), cc["gy"])):
        pad = 0.02 + 1e-5 * np.maximum(np.abs(lo), np.abs(hi)) + 2.0 * rho * g
        out_by = np.maximum(lo - c, c - hi)
        with np.errstate(invalid="ignore"):
            rect = max(rect, float(np.where(front & (out_by > 0), out_by / (0.5 + pad), 0.0).max()))
    out["rect"] = rect
    # the whole mesh's rectangle (frame_consts.cpp mesh_screen_rect + its margins), from the box of every face
    lo3, hi3 = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    corners = np.array([[(hi3 if (c >> k) & 1 else lo3)[k] for k in range(3)] for c in range(8)]) - cc["O"]
    cvx, cvy = corners @ cc["Vx"], corners @ cc["Vy"]
    mr = mesh_rho(cc, lo3, hi3) if world_term else 0.0
    if (cvx / cc["vxa"] > 1e-6).all() and (cvy / cc["vya"] > 1e-6).all() and mr * cc["kk"] <= 0.5:
        cx, cy = -(corners @ cc["Ux"]) / cvx, -(corners @ cc["Uy"]) / cvy
        mesh = 0.0
        for c, lo, hi, g in ((fx, cx.min(), cx.max(), cc["gx"]), (fy, cy.min(), cy.max(), cc["gy"])):
            out_by = np.maximum(lo - c, c - hi)
            pad = 1.0 + 2.0 * mr * g + 1e-4 * max(abs(lo), abs(hi))
            mesh = max(mesh, float(np.where(out_by > 0, out_by / (0.5 + pad), 0.0).max()))
        out["mesh"] = mesh
    return out


def heightfield(ref_loader, n, tex):
    """tests/test_gpu_frame_vmem.py's heightfield: 2 n^2 faces, a gently waved plane at z ~ -4."""
    g = np.linspace(-1.0, 1.0, n + 1, dtype=np.float64)
    x, y = np.meshgrid(g, g)
    z = -4.0 + 0.25 * np.sin(5.0 * x) * np.cos(4.0 * y) + 0.6 * x
    verts = np.zeros((n + 1) * (n + 1), ref_loader.VERTEX_DTYPE)
    verts["position"] = np.stack([2.2 * x, 1.3 * y, z], -1).reshape(-1, 3).astype(np.float32)
    verts["tex_coords"] = np.stack([(x + 1) / 2, (y + 1) / 2], -1).reshape(-1, 2).astype(np.float32)
    i = np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]
    a, b, c, d = i, i + 1, i + n + 1, i + n + 2
    faces = np.zeros(2 * n * n, ref_loader.FACE_DTYPE)
    faces["indices"] = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([b, d, c], -1).reshape(-1, 3)]).astype(np.uint32)
    mat = np.zeros(1, ref_loader.MATERIAL_DTYPE)
    mat["ambient"], mat["diffuse"], mat["specular"] = 0.05, 0.8, 0.3
    return {"vertices": verts, "faces": faces, "material": mat, "texture": tex}


def meshes(ref_loader, res_dir):
    """{name: (model, centre, radius)}: each reaches a different frame path (tile lists; 256 / 257 faces on either side of
    the tile-list limit and the binning threshold; binned or the auto-BVH kernel; a few thousand faces)."""
    import fuzz_common

    suz = ref_loader.load_model_compute(res_dir, "suzanne_lowpoly.obj")
    cube = ref_loader.load_model_compute(res_dir, "cube.obj")
    rng = np.random.default_rng(4242)
    out = {"suzanne": suz, "cube": cube,
           "soup256": fuzz_common.soup(ref_loader, rng, 256, extent=1.0, tri_size=0.15, tex=suz["texture"]),
           "soup257": fuzz_common.soup(ref_loader, rng, 257, extent=1.0, tri_size=0.15, tex=suz["texture"]),
           "heightfield": heightfield(ref_loader, 40, suz["texture"])}
    res = {}
    for k, m in out.items():
        p = m["vertices"]["position"].astype(np.float64)
        lo, hi = p.min(0), p.max(0)
        res[k] = (m, (lo + hi) / 2.0, float(np.linalg.norm(hi - lo)) / 2.0)
    return res


def views(center, radius):
    """{view: (eye, target)} relative to the untranslated model: filling the frame, small in the frame, grazing."""
    c = np.asarray(center, np.float64)
    return {"fill": (tuple(c + radius * np.array([0.25, 0.15, 1.9])), tuple(c)),
            "small": (tuple(c + radius * np.array([1.5, 1.0, 14.0])), tuple(c)),
            "grazing": (tuple(c + radius * np.array([2.2, 0.12, 0.35])), tuple(c))}
