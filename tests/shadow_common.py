"""Scenes and helpers shared by the shadow-ray tests (tests/test_shadows_host.py, tests/test_gpu_shadows.py).

A parity scene must not let "always lit" or "always dark" pass, so every scene carries the class the CPU reference must put it
in at the tests' size (spp 1, primary hits): "mixed" - at least a tenth of its shadow rays occluded and at least a tenth not -
or one of the named extremes, "lit" (occluded share < 0.05) and "dark" (every ray occluded)."""
import numpy as np

W, H = 96, 64

# name -> class
SCENES = {
    "cube": "mixed", "cube_back": "mixed", "suzanne_side": "mixed", "grid": "mixed", "two_parts": "mixed", "cube_nmap": "mixed",
    "suzanne_front": "lit", "two_parts_front": "lit", "closed_room": "dark", "inside_suzanne": "dark",
}
MIXED = [k for k, v in SCENES.items() if v == "mixed"]


def scene(name, rwr, orc, suzanne, cube):
    """(model or parts, spheres, instances, eye, target, extra flags).  Spheres and instances as the oracle's dtypes."""
    ref_spheres = orc.make_spheres()
    one_sphere = orc.make_spheres([((1.6, 1.2, 1.4), 0.5)])
    none = np.zeros(0, orc.SPHERE_DTYPE)
    grid2 = rwr.make_instance_grid(2, 3.0).view(orc.INSTANCE_DTYPE)
    table = {
        "cube": (cube, one_sphere, None, (2.2, 1.7, 3.1), (0, 0, 0), 0),
        "cube_back": (cube, none, None, (-3.0, 1.5, -2.0), (0, 0, 0), 0),
        "suzanne_side": (suzanne, ref_spheres, None, (2.5, 0.5, 1.0), (0, 0, 0), 0),
        "grid": (suzanne, ref_spheres, grid2, (6.5, -1.0, 2.0), (1.5, -1.5, 0), 0),
        "two_parts": ([suzanne, cube], ref_spheres, None, (3.0, 0.5, 1.2), (0, 0, 0), 0),
        "cube_nmap": (cube, one_sphere, None, (-3.0, 1.5, -2.0), (0, 0, 0), orc.FLAG_NORMAL_MAP),
        "suzanne_front": (suzanne, ref_spheres, None, (0.3, 0.2, 2.5), (0.2, 0.2, -2.0), 0),
        "two_parts_front": ([suzanne, cube], ref_spheres, None, (0.5, 0.5, 4.0), (0, 0, 0), 0),
        "closed_room": (cube, none, None, (0.1, 0.2, 0.3), (0.0, 0.0, -1.0), 0),
        "inside_suzanne": (suzanne, ref_spheres, None, (0, 0, 0), (0, 0, -1), 0),
    }
    return table[name]


def camera(rwr, orc, sc, w=W, h=H):
    return rwr.camera_build_inv_uniform(rwr.make_camera(eye=sc[3], target=sc[4], aspect=w / h, fovy=60.0)).view(orc.CAMERA_INV_DTYPE)


def reference(shadow_ref, L, orc, sc, cam_inv, w, h, spp, bounces, seed=7, shadows=True, rows=None):
    model, spheres, inst, _, _, flags = sc
    return shadow_ref.render_path(L, orc, cam_inv, orc.make_screen(w, h), orc.make_params(spp, bounces, seed=seed, flags=flags), spheres, model,
                                  instances=inst, rows=rows, shadows=shadows)


def check_class(name, ref):
    """The coverage condition, asserted on a reference frame of the scene."""
    rays, occ = ref["shadow_rays"], ref["occluded"]
    assert rays > 0, name
    share = occ / rays
    kind = SCENES[name]
    if kind == "mixed":
        assert 0.1 <= share <= 0.9, (name, occ, rays)
    elif kind == "lit":
        assert share < 0.05, (name, occ, rays)
    else:
        assert occ == rays, (name, occ, rays)


def triangle_model(ref_loader, tris, tex, ambient=(0.05, 0.04, 0.03)):
    """A mesh of the given triangles ((p0, p1, p2), ...) with one material."""
    n = len(tris)
    verts = np.zeros(3 * n, ref_loader.VERTEX_DTYPE)
    verts["position"] = np.asarray(tris, np.float32).reshape(-1, 3)
    verts["tex_coords"] = np.tile(np.array([[0.1, 0.1], [0.9, 0.1], [0.5, 0.9]], np.float32), (n, 1))
    faces = np.zeros(n, ref_loader.FACE_DTYPE)
    faces["indices"] = np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)
    mat = np.zeros(1, ref_loader.MATERIAL_DTYPE)
    mat["ambient"], mat["diffuse"], mat["specular"] = ambient, 0.8, 0.3
    return {"vertices": verts, "faces": faces, "material": mat, "texture": tex}


FLOOR = ((-6.0, -6.0, 0.0), (6.0, -6.0, 0.0), (0.0, 8.0, 0.0))        # faces +z: towards the mesh light (-1, 1, 5) / sqrt(27)
BLOCKER = ((-1.0, -1.0, 1.0), (1.5, -1.0, 1.0), (0.0, 1.5, 1.0))      # one unit above it
