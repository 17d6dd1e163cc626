"""Python driver for librwr_hip.so (tests, bench.py, smoke) — thin ctypes over the C ABI.

The product is the shared library declared in include/rwr_hip.h (HIP kernels for
gfx950 + host code in C++); this module only marshals numpy arrays across that
boundary.  There is NO CPU fallback: if the library is missing or no GPU is
visible, construction of a `Context` raises.

The directory name contains '-', so it is imported through
`__graft_entry__.load_package()` under the module name `rwr_amd`.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RWR_HIP_LIB") or os.path.join(_HERE, "lib", "librwr_hip.so")  # override: A/B runs of two builds
RES_DIR = os.path.join(_HERE, "res")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "rwr_hip.h")

# ---- PODs (layout-identical to include/rwr_hip.h and the reference's #[repr(C)] structs)
CAMERA_INV_DTYPE = np.dtype(
    [("viewmodel_inv", "<f4", (4, 4)), ("proj_inv", "<f4", (4, 4)), ("origin", "<f4", (3,)), ("_padding", "<u4")])
SCREEN_DTYPE = np.dtype([("width", "<u4"), ("height", "<u4")])
VERTEX_DTYPE = np.dtype([("position", "<f4", (3,)), ("pad0", "<f4"), ("tex_coords", "<f4", (2,)), ("pad1", "<f4", (2,))])
FACE_DTYPE = np.dtype([("indices", "<u4", (3,)), ("pad0", "<u4")])
MATERIAL_DTYPE = np.dtype([("ambient", "<f4", (3,)), ("pad0", "<f4"), ("diffuse", "<f4", (3,)), ("pad1", "<f4"),
                           ("specular", "<f4", (3,)), ("pad2", "<f4")])
SPHERE_DTYPE = np.dtype([("center", "<f4", (3,)), ("radius", "<f4")])
INSTANCE_DTYPE = np.dtype([("model", "<f4", (4, 4))])
TRIANGLE_DTYPE = np.dtype([("p0", "<f4", (3,)), ("pad0", "<f4"), ("p1", "<f4", (3,)), ("pad1", "<f4"),
                           ("p2", "<f4", (3,)), ("pad2", "<f4")])  # rwr_triangle_buffer_data, 48 B
CAMERA_DTYPE = np.dtype([("eye", "<f4", (3,)), ("target", "<f4", (3,)), ("up", "<f4", (3,)),
                         ("aspect", "<f4"), ("fovy", "<f4"), ("znear", "<f4"), ("zfar", "<f4")])
PARAMS_DTYPE = np.dtype([("spp", "<u4"), ("max_bounces", "<u4"), ("seed", "<u4"), ("flags", "<u4")])
assert (CAMERA_INV_DTYPE.itemsize, VERTEX_DTYPE.itemsize, FACE_DTYPE.itemsize, MATERIAL_DTYPE.itemsize,
        SPHERE_DTYPE.itemsize, INSTANCE_DTYPE.itemsize, CAMERA_DTYPE.itemsize) == (144, 32, 16, 48, 16, 64, 52)

FLAG_AUX_OUTPUTS, FLAG_NO_CULL, FLAG_USE_BVH = 1, 2, 4
# internal debug flags (csrc/rwr_internal.h, not part of include/rwr_hip.h)
FLAG_ORTHO_RAYS = 1 << 3
FLAG_NORMAL_MAP = 1 << 4
FLAG_ACCUMULATE = 1 << 5
FLAG_MULTI_BOUNCE = 1 << 6   # max_bounces up to MAX_BOUNCES (include/rwr_hip.h)
FLAG_SHADOWS = 1 << 7        # shadow rays towards the reference's two lights (include/rwr_hip.h)
FLAG_DENOISE = 1 << 8        # the a-trous filter behind the integrator's resolve; implies FLAG_AUX_OUTPUTS (include/rwr_hip.h)
DENOISE_PARAMS_DTYPE = np.dtype([("iterations", "<u4"), ("sigma_color", "<f4"), ("normal_cos_min", "<f4"), ("depth_rel", "<f4")])
FLAG_SKY = 1 << 9            # bounce rays that leave the scene return the sky's radiance (include/rwr_hip.h)
SKY_PARAMS_DTYPE = np.dtype([("zenith", "<f4", 3), ("horizon", "<f4", 3)])
FLAG_MIRRORS = 1 << 10       # parts and spheres marked as mirrors reflect the ray that found them (include/rwr_hip.h)
FLAG_GLASS = 1 << 11         # parts and spheres marked as glass reflect by Fresnel's law and refract by Snell's (include/rwr_hip.h)
FLAG_REPROJECT = 1 << 12     # temporal reprojection of the context's history while the camera moves; implies FLAG_AUX_OUTPUTS (include/rwr_hip.h)
FLAG_GLOSSY = 1 << 13        # parts and spheres marked as glossy send on a ray between the mirror reflection and the diffuse ray (include/rwr_hip.h)
FLAG_SOFT_SHADOWS = 1 << 14  # FLAG_SHADOWS' two lights get an angular size: penumbrae (include/rwr_hip.h)
FLAG_EMISSIVE = 1 << 15      # parts and spheres with an emission (set_part_emission, set_sphere_emission) give off light (include/rwr_hip.h)
FLAG_LIGHT_SAMPLING = 1 << 16  # every diffuse hit also sends a ray towards an emitting sphere: next-event estimation (include/rwr_hip.h)
FLAG_LIGHT_PARTS = 1 << 21     # ... or towards a point on a face of an emitting part, the mesh light (include/rwr_hip.h; bits 17-20 are reserved)
FLAG_LIGHT_MIS = 1 << 22       # the light ray and the diffuse bounce ray are combined by the balance heuristic: multiple importance sampling (include/rwr_hip.h)
FLAG_SOBOL = 1 << 23           # every random number of the path tracer comes from an Owen-scrambled Sobol sequence instead of the hash (include/rwr_hip.h)
FLAG_LIGHT_SKY = 1 << 25       # the light ray of a diffuse hit may aim at FLAG_SKY_IMAGE's map, drawn in proportion to its radiance (include/rwr_hip.h)
FLAG_SKY_IMAGE = 1 << 24       # FLAG_SKY's radiance comes from the context's octahedral environment map (sky_set_image) instead of the gradient (include/rwr_hip.h)
FLAG_TONEMAP = 1 << 26         # exposure and a tone curve over the frame's rgba8 plane, the last stage behind the resolve; implies FLAG_AUX_OUTPUTS (include/rwr_hip.h)
TONEMAP_CLAMP, TONEMAP_REINHARD, TONEMAP_ACES = 0, 1, 2   # RWR_TONEMAP_*
TONEMAP_PARAMS_DTYPE = np.dtype([("curve", "<u4"), ("auto_exposure", "<u4"), ("exposure", "<f4"), ("key", "<f4"), ("white", "<f4")])
SKY_IMAGE_SIZE_MAX, SKY_IMAGE_COMPONENT_MAX = 2048, 64.0  # RWR_SKY_IMAGE_SIZE_MAX, RWR_SKY_IMAGE_COMPONENT_MAX
MAX_EMISSION = 64.0         # RWR_MAX_EMISSION: the largest component of a radiance
SHADOW_PARAMS_DTYPE = np.dtype([("mesh_light_radius", "<f4"), ("sphere_light_radius", "<f4")])
REPROJECT_PARAMS_DTYPE = np.dtype([("max_history", "<u4"), ("normal_cos_min", "<f4"), ("depth_rel", "<f4")])
MAX_BOUNCES = 8
FLAG_DEBUG_COUNTS, FLAG_ONE_PIXEL_PER_LANE = 1 << 20, 1 << 17
KEY_FORWARD, KEY_BACKWARD, KEY_LEFT, KEY_RIGHT, KEY_UP, KEY_DOWN = 1, 2, 4, 8, 16, 32
OK, ERR_INVALID_ARGUMENT, ERR_HIP, ERR_NOT_READY, ERR_IO, ERR_PARSE, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6

# reference scene literals: src/lib.rs:352-361, 532-534
REFERENCE_SPHERES = [((0.6, 0.5, -4.0), 0.4), ((0.4, 0.4, -3.0), 0.4)]
CONTROLLER_SPEED = 0.2


class RwrError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"rwr error {code}: {message}")
        self.code = code
        self.message = message


def build(force: bool = False) -> str:
    """Compile librwr_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", _HERE, "-j4"] + (["-B"] if force else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building librwr_hip.so failed:\n" + r.stdout + r.stderr)
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    """Loads librwr_hip.so.  torch is imported first so that the process binds ONE
    libamdhip64 (torch ships its own copy with the same SONAME)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the render path)")
    try:
        import torch  # noqa: F401  (HIP runtime provider)
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u32, i32, f32 = C.c_void_p, C.c_uint32, C.c_int, C.c_float
    L.rwr_last_error_string.restype = C.c_char_p
    L.rwr_ctx_get_stream.restype = vp
    for name in ("rwr_model_vertices", "rwr_model_faces", "rwr_model_material", "rwr_model_texture_rgba8"):
        getattr(L, name).restype = vp
        getattr(L, name).argtypes = [vp]
    sigs = {
        "rwr_ctx_create": [i32, vp], "rwr_ctx_destroy": [vp], "rwr_device_count": [vp],
        "rwr_ctx_device_info": [vp, vp, C.c_size_t, vp, vp], "rwr_ctx_set_stream": [vp, vp], "rwr_ctx_get_stream": [vp],
        "rwr_scene_upload_mesh": [vp, vp, u32, vp, u32, vp, vp, u32, u32],
        "rwr_scene_clear": [vp], "rwr_scene_add_mesh": [vp, vp, u32, vp, u32, vp, vp, u32, u32], "rwr_scene_commit": [vp],
        "rwr_model_part_count": [vp, vp], "rwr_model_part": [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp],
        "rwr_scene_upload_model_all": [vp, vp], "rwr_model_part_normal_map": [vp, u32, vp, vp, vp],
        "rwr_scene_set_normal_map": [vp, u32, vp, u32, u32], "rwr_scene_part_count": [vp, vp],
        "rwr_scene_set_spheres": [vp, vp, u32], "rwr_scene_set_triangles": [vp, vp, u32], "rwr_scene_set_instances": [vp, vp, u32],
        "rwr_resize": [vp, vp], "rwr_render": [vp, vp, vp], "rwr_render_rows": [vp, vp, vp, u32, u32], "rwr_render_strips": [vp, vp, vp, u32, u32],
        "rwr_synchronize": [vp], "rwr_readback": [vp, vp, vp, vp, vp, vp], "rwr_get_device_targets": [vp, vp, vp],
        "rwr_timer_begin": [vp], "rwr_timer_end": [vp, vp], "rwr_timer_stop": [vp], "rwr_timer_elapsed": [vp, vp], "rwr_last_render_stats": [vp, vp, vp],
        "rwr_last_shadow_stats": [vp, vp, vp], "rwr_frame_setup_launches": [vp, vp], "rwr_ray_plane_stats": [vp, vp, vp],
        "rwr_debug_tile_classes": [vp, vp, C.c_size_t, vp, vp],
        "rwr_debug_tile_cover": [vp, vp, C.c_size_t, vp, vp], "rwr_tile_cover_stats": [vp, vp, vp], "rwr_lean_rest_stats": [vp, vp],
        "rwr_last_traversal_plan": [vp, vp, vp],
        "rwr_accum_reset": [vp], "rwr_accum_samples": [vp, vp],
        "rwr_denoise_set_params": [vp, vp], "rwr_denoise_get_params": [vp, vp],
        "rwr_tonemap_set_params": [vp, vp], "rwr_tonemap_get_params": [vp, vp], "rwr_last_tonemap_stats": [vp, vp, vp, vp],
        "rwr_sky_set_params": [vp, vp], "rwr_sky_get_params": [vp, vp],
        "rwr_sky_set_image": [vp, vp, u32], "rwr_sky_get_image_info": [vp, vp, vp],
        "rwr_sky_image_from_equirect": [vp, u32, u32, f32, u32, vp], "rwr_selftest_sky_image": [vp, vp, C.c_size_t, vp],
        "rwr_sky_get_light_info": [vp, vp, vp], "rwr_last_sky_light_stats": [vp, vp, vp, vp], "rwr_selftest_sky_light": [vp, vp, C.c_size_t, vp, u32, vp],
        "rwr_shadow_set_params": [vp, vp], "rwr_shadow_get_params": [vp, vp],
        "rwr_reproject_set_params": [vp, vp], "rwr_reproject_get_params": [vp, vp], "rwr_reproject_reset": [vp],
        "rwr_reproject_frames": [vp, vp], "rwr_last_reproject_stats": [vp, vp, vp, vp], "rwr_reproject_readback": [vp, vp],
        "rwr_scene_set_part_mirror": [vp, u32, vp], "rwr_scene_set_sphere_mirror": [vp, u32, vp],
        "rwr_scene_get_part_mirror": [vp, u32, vp, vp], "rwr_scene_get_sphere_mirror": [vp, u32, vp, vp],
        "rwr_scene_set_part_glass": [vp, u32, f32, vp], "rwr_scene_set_sphere_glass": [vp, u32, f32, vp],
        "rwr_scene_get_part_glass": [vp, u32, vp, vp, vp], "rwr_scene_get_sphere_glass": [vp, u32, vp, vp, vp],
        "rwr_last_glass_stats": [vp, vp, vp, vp],
        "rwr_scene_set_part_gloss": [vp, u32, vp, f32], "rwr_scene_set_sphere_gloss": [vp, u32, vp, f32],
        "rwr_scene_get_part_gloss": [vp, u32, vp, vp, vp], "rwr_scene_get_sphere_gloss": [vp, u32, vp, vp, vp],
        "rwr_last_gloss_stats": [vp, vp],
        "rwr_scene_set_part_emission": [vp, u32, vp], "rwr_scene_set_sphere_emission": [vp, u32, vp],
        "rwr_scene_get_part_emission": [vp, u32, vp, vp], "rwr_scene_get_sphere_emission": [vp, u32, vp, vp],
        "rwr_last_emission_stats": [vp, vp], "rwr_last_light_stats": [vp, vp, vp, vp], "rwr_last_part_light_stats": [vp, vp, vp, vp],
        "rwr_camera_build_inv_uniform": [vp, vp], "rwr_circle_controller_update": [f32, u32, vp],
        "rwr_load_model_compute": [C.c_char_p, C.c_char_p, vp], "rwr_model_free": [vp],
        "rwr_model_info": [vp, vp, vp, vp, vp, vp, vp], "rwr_scene_upload_model": [vp, vp],
        "rwr_decode_image_rgba8": [vp, C.c_size_t, vp, vp, vp], "rwr_free": [vp],
        "rwr_make_instance_grid": [u32, f32, vp],
        "rwr_write_png_rgba8": [C.c_char_p, vp, u32, u32, i32, i32],
        "rwr_ctx_set_kernel_timing": [vp, u32], "rwr_kernel_timing_stats": [vp, vp, vp],
        "rwr_selftest_exact_math": [vp, u32, u32, vp], "rwr_selftest_exact_div": [vp, u32, u32, vp], "rwr_ctx_set_frames_in_flight": [vp, u32],
        "rwr_selftest_sobol": [vp, vp, vp, vp, vp, C.c_size_t, vp],
        "rwr_dist_get_unique_id": [vp], "rwr_dist_init": [vp, i32, i32, vp], "rwr_dist_band": [u32, u32, u32, vp, vp],
        "rwr_dist_gather_rgba8": [vp, i32], "rwr_dist_gather_strips_rgba8": [vp, i32], "rwr_dist_frame": [vp, vp], "rwr_dist_readback": [vp, vp],
        "rwr_dist_barrier": [vp], "rwr_dist_destroy": [vp],
        "rwr_dist_strip_layout": [u32, u32, u32, vp], "rwr_dist_host_pack_strips": [u32, u32, u32, u32, vp, vp],
        "rwr_dist_host_deal_strips": [u32, u32, u32, vp, vp], "rwr_host_texture_quads": [vp, u32, u32, vp],
        "rwr_dist_loopback_deposit": [vp, u32, u32, i32], "rwr_dist_loopback_finish": [vp, u32, i32],
        "rwr_measure_valu_clock": [vp, u32, vp], "rwr_clock_probe_start": [vp, u32], "rwr_clock_probe_read": [vp, vp],
    }
    _NEWER_ENTRY_POINTS = ("rwr_last_shadow_stats", "rwr_denoise_set_params", "rwr_denoise_get_params", "rwr_frame_setup_launches", "rwr_ray_plane_stats", "rwr_debug_tile_classes", "rwr_debug_tile_cover", "rwr_tile_cover_stats", "rwr_lean_rest_stats", "rwr_last_traversal_plan",
                           "rwr_sky_set_params", "rwr_sky_get_params", "rwr_scene_set_part_mirror", "rwr_scene_set_sphere_mirror",
                           "rwr_scene_get_part_mirror", "rwr_scene_get_sphere_mirror", "rwr_scene_set_part_glass", "rwr_scene_set_sphere_glass",
                           "rwr_scene_get_part_glass", "rwr_scene_get_sphere_glass", "rwr_last_glass_stats",
                           "rwr_reproject_set_params", "rwr_reproject_get_params", "rwr_reproject_reset", "rwr_reproject_frames",
                           "rwr_last_reproject_stats", "rwr_reproject_readback", "rwr_scene_set_part_gloss", "rwr_scene_set_sphere_gloss",
                           "rwr_scene_get_part_gloss", "rwr_scene_get_sphere_gloss", "rwr_last_gloss_stats",
                           "rwr_shadow_set_params", "rwr_shadow_get_params", "rwr_scene_set_part_emission", "rwr_scene_set_sphere_emission",
                           "rwr_scene_get_part_emission", "rwr_scene_get_sphere_emission", "rwr_last_emission_stats", "rwr_last_light_stats", "rwr_last_part_light_stats",
                           "rwr_selftest_sobol", "rwr_sky_set_image", "rwr_sky_get_image_info", "rwr_sky_image_from_equirect", "rwr_selftest_sky_image",
                           "rwr_sky_get_light_info", "rwr_last_sky_light_stats", "rwr_selftest_sky_light",
                           "rwr_tonemap_set_params", "rwr_tonemap_get_params", "rwr_last_tonemap_stats")   # what a library named by RWR_HIP_LIB may lack; any other gap is an error
    for name, argtypes in sigs.items():
        fn = getattr(L, name, None)
        if fn is None and name in _NEWER_ENTRY_POINTS and os.environ.get("RWR_HIP_LIB"):
            continue   # an A/B build of an earlier commit (tools/ab.sh, tools/shadow_probe.py) lacks it; calling it raises
        if fn is None:
            raise AttributeError(f"{LIB_PATH} does not export {name}")
        fn.argtypes = argtypes
        if name not in ("rwr_ctx_destroy", "rwr_model_free", "rwr_free", "rwr_ctx_get_stream"):
            fn.restype = C.c_int
        elif name != "rwr_ctx_get_stream":
            fn.restype = None
    _lib = L
    return L


def _check(rc: int):
    if rc != OK:
        raise RwrError(rc, lib().rwr_last_error_string().decode("utf-8", "replace"))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------ host surface --
def make_camera(eye=(0, 0, 0), target=(0, 0, -1), up=(0, 1, 0), aspect=1.0, fovy=60.0, znear=0.1, zfar=100.0):
    """Camera literal of src/lib.rs:352-360 by default."""
    cam = np.zeros(1, dtype=CAMERA_DTYPE)
    cam["eye"], cam["target"], cam["up"] = eye, target, up
    cam["aspect"], cam["fovy"], cam["znear"], cam["zfar"] = aspect, fovy, znear, zfar
    return cam


def camera_build_inv_uniform(cam: np.ndarray) -> np.ndarray:
    out = np.zeros(1, dtype=CAMERA_INV_DTYPE)
    _check(lib().rwr_camera_build_inv_uniform(_p(cam), _p(out)))
    return out


def circle_controller_update(cam: np.ndarray, keys: int, speed: float = CONTROLLER_SPEED) -> np.ndarray:
    cam = cam.copy()
    _check(lib().rwr_circle_controller_update(speed, keys, _p(cam)))
    return cam


def make_screen(w: int, h: int) -> np.ndarray:
    s = np.zeros(1, dtype=SCREEN_DTYPE)
    s["width"], s["height"] = w, h
    return s


def make_spheres(spec=REFERENCE_SPHERES) -> np.ndarray:
    s = np.zeros(len(spec), dtype=SPHERE_DTYPE)
    for i, (c, r) in enumerate(spec):
        s[i]["center"], s[i]["radius"] = c, r
    return s


def make_triangles(spec=()) -> np.ndarray:
    t = np.zeros(len(spec), dtype=TRIANGLE_DTYPE)
    for i, (p0, p1, p2) in enumerate(spec):
        t[i]["p0"], t[i]["p1"], t[i]["p2"] = p0, p1, p2
    return t


def make_params(spp=1, max_bounces=0, seed=0, flags=0) -> np.ndarray:
    p = np.zeros(1, dtype=PARAMS_DTYPE)
    p["spp"], p["max_bounces"], p["seed"], p["flags"] = spp, max_bounces, seed, flags
    return p


def make_instance_grid(per_row: int, space_between: float = 3.0) -> np.ndarray:
    out = np.zeros(per_row * per_row, dtype=INSTANCE_DTYPE)
    _check(lib().rwr_make_instance_grid(per_row, space_between, _p(out)))
    return out


def decode_image_rgba8(data: bytes) -> np.ndarray:
    buf = np.frombuffer(data, dtype=np.uint8)
    out = C.c_void_p()
    w, h = C.c_uint32(), C.c_uint32()
    _check(lib().rwr_decode_image_rgba8(_p(buf), len(data), C.byref(out), C.byref(w), C.byref(h)))
    try:
        arr = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), shape=(h.value, w.value, 4)).copy()
    finally:
        lib().rwr_free(out)
    return arr


def write_png(path: str, rgba8: np.ndarray, flip_vertical: bool = True, encode_srgb: bool = False):
    rgba8 = np.ascontiguousarray(rgba8, dtype=np.uint8)
    h, w = rgba8.shape[:2]
    _check(lib().rwr_write_png_rgba8(path.encode(), _p(rgba8), w, h, int(flip_vertical), int(encode_srgb)))


def load_model_compute(file_name: str, res_dir: str = RES_DIR) -> dict:
    """resources::load_model_compute through the C ABI; returns numpy copies of
    meshes[0] / materials[0] (what TriangleList consumes)."""
    L = lib()
    h = C.c_void_p()
    _check(L.rwr_load_model_compute(res_dir.encode(), file_name.encode(), C.byref(h)))
    try:
        n = [C.c_uint32() for _ in range(6)]
        _check(L.rwr_model_info(h, *[C.byref(x) for x in n]))
        n_meshes, n_materials, n_verts, n_faces, tw, th = [x.value for x in n]
        verts = np.frombuffer(C.string_at(L.rwr_model_vertices(h), n_verts * 32), dtype=VERTEX_DTYPE).copy()
        faces = np.frombuffer(C.string_at(L.rwr_model_faces(h), n_faces * 16), dtype=FACE_DTYPE).copy()
        material = np.frombuffer(C.string_at(L.rwr_model_material(h), 48), dtype=MATERIAL_DTYPE).copy()
        tex = np.frombuffer(C.string_at(L.rwr_model_texture_rgba8(h), tw * th * 4), dtype=np.uint8).reshape(th, tw, 4).copy()
        nmap = _part_normal_map(L, h, 0)
    finally:
        L.rwr_model_free(h)
    return {"vertices": verts, "faces": faces, "material": material, "texture": tex, "normal_map": nmap,
            "n_meshes": n_meshes, "n_materials": n_materials}


def _part_normal_map(L, h, part):
    """The decoded map_Bump image of a part's material (extension), or None."""
    pn, nw, nh = C.c_void_p(), C.c_uint32(), C.c_uint32()
    _check(L.rwr_model_part_normal_map(h, part, C.byref(pn), C.byref(nw), C.byref(nh)))
    if not pn.value:
        return None
    return np.frombuffer(C.string_at(pn, nw.value * nh.value * 4), dtype=np.uint8).reshape(nh.value, nw.value, 4).copy()



def load_model_parts(file_name: str, res_dir: str = RES_DIR) -> list:
    """Extension: every mesh of the file with its own material, as a list of model dicts."""
    L = lib()
    h = C.c_void_p()
    _check(L.rwr_load_model_compute(res_dir.encode(), file_name.encode(), C.byref(h)))
    parts = []
    try:
        n = C.c_uint32()
        _check(L.rwr_model_part_count(h, C.byref(n)))
        for i in range(n.value):
            pv, pf, pt = C.c_void_p(), C.c_void_p(), C.c_void_p()
            nv, nf, tw, th = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
            mat = np.zeros(1, dtype=MATERIAL_DTYPE)
            _check(L.rwr_model_part(h, i, C.byref(pv), C.byref(nv), C.byref(pf), C.byref(nf), _p(mat), C.byref(pt), C.byref(tw), C.byref(th)))
            parts.append({
                "vertices": np.frombuffer(C.string_at(pv, nv.value * 32), dtype=VERTEX_DTYPE).copy(),
                "faces": np.frombuffer(C.string_at(pf, nf.value * 16), dtype=FACE_DTYPE).copy(),
                "material": mat,
                "texture": np.frombuffer(C.string_at(pt, tw.value * th.value * 4), dtype=np.uint8).reshape(th.value, tw.value, 4).copy(),
                "normal_map": _part_normal_map(L, h, i),
            })
    finally:
        L.rwr_model_free(h)
    return parts


# ----------------------------------------------------------------- multi-GPU frames --
DIST_ID_BYTES = 128
STRIP_ROWS = 8   # RWR_STRIP_ROWS


def dist_get_unique_id() -> bytes:
    """RCCL unique id (rank 0 creates it, the launcher hands it to every rank)."""
    buf = (C.c_uint8 * DIST_ID_BYTES)()
    _check(lib().rwr_dist_get_unique_id(buf))
    return bytes(buf)


def dist_band(rank: int, world: int, height: int) -> tuple[int, int]:
    a, b = C.c_uint32(), C.c_uint32()
    _check(lib().rwr_dist_band(rank, world, height, C.byref(a), C.byref(b)))
    return a.value, b.value


class _StripLayout(C.Structure):   # rwr_strip_layout
    _fields_ = [(n, C.c_uint32) for n in ("n_strips", "strips", "rows", "recv_row", "recv_rows_total", "owns_tail")]


def dist_strip_layout(rank: int, world: int, height: int) -> dict:
    """The interleaved partition's gather layout as the library uses it (rwr_dist_strip_layout; host arithmetic, no GPU)."""
    out = _StripLayout()
    _check(lib().rwr_dist_strip_layout(rank, world, height, C.byref(out)))
    return {n: int(getattr(out, n)) for n, _ in _StripLayout._fields_}


def dist_host_pack_strips(rank: int, world: int, frame: np.ndarray) -> np.ndarray:
    """rank's message (its strips back to back) cut from a whole (H, W, 4) uint8 frame in HOST memory, by the library's layout."""
    frame = np.ascontiguousarray(frame, np.uint8)
    h, w = frame.shape[:2]
    lay = dist_strip_layout(rank, world, h)
    msg = np.zeros((max(1, lay["strips"] * STRIP_ROWS), w, 4), np.uint8)
    _check(lib().rwr_dist_host_pack_strips(rank, world, w, h, _p(frame), _p(msg)))
    return msg[:lay["rows"]]


def host_texture_quads(rgba8: np.ndarray) -> np.ndarray:
    """The frame kernel's quad records of an (H, W, 4) uint8 sRGB texture, built on the host: (H + 1, W + 1, 4) uint32."""
    rgba8 = np.ascontiguousarray(rgba8, np.uint8)
    h, w = rgba8.shape[:2]
    out = np.zeros((h + 1, w + 1, 4), np.uint32)
    _check(lib().rwr_host_texture_quads(_p(rgba8), w, h, _p(out)))
    return out


def dist_host_deal_strips(world: int, recv: np.ndarray, height: int) -> np.ndarray:
    """The frame assembled from the root's receive buffer ((recv_rows_total, W, 4) uint8, HOST memory), by the library's layout."""
    recv = np.ascontiguousarray(recv, np.uint8)
    w = recv.shape[1]
    assert recv.shape[0] == dist_strip_layout(0, world, height)["recv_rows_total"]
    frame = np.zeros((height, w, 4), np.uint8)
    _check(lib().rwr_dist_host_deal_strips(world, w, height, _p(recv), _p(frame)))
    return frame


# ------------------------------------------------------------------------ context --
def device_count() -> int:
    n = C.c_int()
    lib().rwr_device_count(C.byref(n))
    return n.value


class Context:
    """One GPU, one HIP stream (rwr_context)."""

    def __init__(self, device_id: int = 0):
        self._h = C.c_void_p()
        _check(lib().rwr_ctx_create(device_id, C.byref(self._h)))
        self.width = self.height = 0

    def close(self):
        if getattr(self, "_h", None):
            lib().rwr_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def device_info(self) -> dict:
        name = C.create_string_buffer(256)
        cu, ws = C.c_int(), C.c_int()
        _check(lib().rwr_ctx_device_info(self._h, name, 256, C.byref(cu), C.byref(ws)))
        return {"name": name.value.decode(), "cu_count": cu.value, "wave_size": ws.value}

    def set_stream(self, hip_stream: int | None):
        _check(lib().rwr_ctx_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def upload_mesh(self, vertices, faces, material, texture):
        vertices = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE)
        faces = np.ascontiguousarray(faces, dtype=FACE_DTYPE)
        material = np.ascontiguousarray(material, dtype=MATERIAL_DTYPE)
        texture = np.ascontiguousarray(texture, dtype=np.uint8)
        th, tw = texture.shape[:2] if texture.ndim == 3 else (0, 0)
        _check(lib().rwr_scene_upload_mesh(self._h, _p(vertices), len(vertices), _p(faces), len(faces),
                                           _p(material), _p(texture), tw, th))

    def upload_model(self, model: dict):
        self.upload_mesh(model["vertices"], model["faces"], model["material"], model["texture"])
        if model.get("normal_map") is not None and len(model["faces"]):
            self.set_normal_map(0, model["normal_map"])

    def set_normal_map(self, part: int, rgba8_linear):
        """Extension: the normal map (RGBA8, linear) of scene part `part`; None removes it.  Used by FLAG_NORMAL_MAP renders."""
        if rgba8_linear is None:
            _check(lib().rwr_scene_set_normal_map(self._h, part, None, 0, 0))
            return
        t = np.ascontiguousarray(rgba8_linear, dtype=np.uint8)
        _check(lib().rwr_scene_set_normal_map(self._h, part, _p(t), t.shape[1], t.shape[0]))

    def upload_parts(self, parts: list):
        """Extension: a scene of several meshes, each with its own material and texture."""
        _check(lib().rwr_scene_clear(self._h))
        for m in parts:
            vertices = np.ascontiguousarray(m["vertices"], dtype=VERTEX_DTYPE)
            faces = np.ascontiguousarray(m["faces"], dtype=FACE_DTYPE)
            material = np.ascontiguousarray(m["material"], dtype=MATERIAL_DTYPE)
            texture = np.ascontiguousarray(m["texture"], dtype=np.uint8)
            th, tw = texture.shape[:2]
            _check(lib().rwr_scene_add_mesh(self._h, _p(vertices), len(vertices), _p(faces), len(faces), _p(material),
                                            _p(texture), tw, th))
            if m.get("normal_map") is not None and len(faces):
                n = C.c_uint32()
                _check(lib().rwr_scene_part_count(self._h, C.byref(n)))
                self.set_normal_map(n.value - 1, m["normal_map"])
        _check(lib().rwr_scene_commit(self._h))

    def set_spheres(self, spheres):
        spheres = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
        _check(lib().rwr_scene_set_spheres(self._h, _p(spheres) if len(spheres) else None, len(spheres)))

    @staticmethod
    def _reflectance(reflectance):
        if reflectance is None:
            return None
        r = np.ascontiguousarray(reflectance, dtype=np.float32)
        if r.shape != (3,):
            raise ValueError("reflectance: three floats, or None")
        return r

    def set_part_mirror(self, part: int, reflectance=(1.0, 1.0, 1.0)):
        """FLAG_MIRRORS: scene part `part` is a mirror of this reflectance (three floats in [0, 1]); None: not a mirror.  Out of
        range or NaN: RwrError(ERR_INVALID_ARGUMENT), and the old state stays (rwr_scene_set_part_mirror)."""
        r = self._reflectance(reflectance)
        _check(lib().rwr_scene_set_part_mirror(self._h, part, _p(r)))

    def set_sphere_mirror(self, sphere: int, reflectance=(1.0, 1.0, 1.0)):
        """FLAG_MIRRORS: the sphere of index `sphere` (< 8, kept whatever set_spheres holds) is a mirror; None: not a mirror."""
        r = self._reflectance(reflectance)
        _check(lib().rwr_scene_set_sphere_mirror(self._h, sphere, _p(r)))

    def _get_mirror(self, fn, index: int):
        on = C.c_int(0)
        r = np.zeros(3, np.float32)
        _check(fn(self._h, index, C.byref(on), _p(r)))
        return r if on.value else None

    def get_part_mirror(self, part: int):
        """The part's reflectance (float32[3]) when it is a mirror, else None (rwr_scene_get_part_mirror)."""
        return self._get_mirror(lib().rwr_scene_get_part_mirror, part)

    def get_sphere_mirror(self, sphere: int):
        """The sphere index's reflectance (float32[3]) when it is a mirror, else None (rwr_scene_get_sphere_mirror)."""
        return self._get_mirror(lib().rwr_scene_get_sphere_mirror, sphere)

    def set_part_glass(self, part: int, ior: float = 1.5, tint=(1.0, 1.0, 1.0)):
        """FLAG_GLASS: scene part `part` is glass of index of refraction `ior` (in [1, 4]) and this tint (three floats in [0, 1]);
        tint None: not glass.  Out of range or NaN: RwrError(ERR_INVALID_ARGUMENT), and the old state stays.  An accepted call
        clears the part's mirror attribute (rwr_scene_set_part_glass)."""
        t = self._reflectance(tint)
        _check(lib().rwr_scene_set_part_glass(self._h, part, ior, _p(t)))

    def set_sphere_glass(self, sphere: int, ior: float = 1.5, tint=(1.0, 1.0, 1.0)):
        """FLAG_GLASS: the sphere of index `sphere` (< 8, kept whatever set_spheres holds) is glass; tint None: not glass."""
        t = self._reflectance(tint)
        _check(lib().rwr_scene_set_sphere_glass(self._h, sphere, ior, _p(t)))

    def _get_glass(self, fn, index: int):
        on = C.c_int(0)
        ior = C.c_float(0.0)
        t = np.zeros(3, np.float32)
        _check(fn(self._h, index, C.byref(on), C.byref(ior), _p(t)))
        return (float(ior.value), t) if on.value else None

    def get_part_glass(self, part: int):
        """(ior, tint float32[3]) when the part is glass, else None (rwr_scene_get_part_glass)."""
        return self._get_glass(lib().rwr_scene_get_part_glass, part)

    def get_sphere_glass(self, sphere: int):
        """(ior, tint float32[3]) when the sphere index is glass, else None (rwr_scene_get_sphere_glass)."""
        return self._get_glass(lib().rwr_scene_get_sphere_glass, sphere)

    def last_glass_stats(self):
        """(reflected, transmitted, totally reflected): what the glass hits of the last render call did (rwr_last_glass_stats)."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().rwr_last_glass_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def set_part_gloss(self, part: int, roughness: float = 0.25, reflectance=(1.0, 1.0, 1.0)):
        """FLAG_GLOSSY: scene part `part` is glossy, of this roughness (in [2**-10, 1]) and reflectance (three floats in [0, 1]);
        reflectance None: not glossy.  Out of range or NaN: RwrError(ERR_INVALID_ARGUMENT), and the old state stays.  An accepted
        call clears the part's mirror and glass attribute (rwr_scene_set_part_gloss)."""
        r = self._reflectance(reflectance)
        _check(lib().rwr_scene_set_part_gloss(self._h, part, _p(r), roughness))

    def set_sphere_gloss(self, sphere: int, roughness: float = 0.25, reflectance=(1.0, 1.0, 1.0)):
        """FLAG_GLOSSY: the sphere of index `sphere` (< 8, kept whatever set_spheres holds) is glossy; reflectance None: not glossy."""
        r = self._reflectance(reflectance)
        _check(lib().rwr_scene_set_sphere_gloss(self._h, sphere, _p(r), roughness))

    def _get_gloss(self, fn, index: int):
        on = C.c_int(0)
        rough = C.c_float(0.0)
        r = np.zeros(3, np.float32)
        _check(fn(self._h, index, C.byref(on), _p(r), C.byref(rough)))
        return (float(rough.value), r) if on.value else None

    def get_part_gloss(self, part: int):
        """(roughness, reflectance float32[3]) when the part is glossy, else None (rwr_scene_get_part_gloss)."""
        return self._get_gloss(lib().rwr_scene_get_part_gloss, part)

    def get_sphere_gloss(self, sphere: int):
        """(roughness, reflectance float32[3]) when the sphere index is glossy, else None (rwr_scene_get_sphere_gloss)."""
        return self._get_gloss(lib().rwr_scene_get_sphere_gloss, sphere)

    def last_gloss_stats(self):
        """The rays the glossy hits of the last render call sent on (rwr_last_gloss_stats)."""
        a = C.c_uint64(0)
        _check(lib().rwr_last_gloss_stats(self._h, C.byref(a)))
        return int(a.value)

    @staticmethod
    def _radiance(radiance):
        if radiance is None:
            return None
        r = np.ascontiguousarray(radiance, dtype=np.float32)
        if r.shape != (3,):
            raise ValueError("radiance: three floats, or None")
        return r

    def set_part_emission(self, part: int, radiance=(1.0, 1.0, 1.0)):
        """FLAG_EMISSIVE: scene part `part` gives off light of this radiance (three floats in [0, MAX_EMISSION]); None or zeros: it
        does not emit.  Out of range, NaN or inf: RwrError(ERR_INVALID_ARGUMENT), and the old state stays.  The part's mirror,
        glass or gloss attribute is left alone (rwr_scene_set_part_emission)."""
        _check(lib().rwr_scene_set_part_emission(self._h, part, _p(self._radiance(radiance))))

    def set_sphere_emission(self, sphere: int, radiance=(1.0, 1.0, 1.0)):
        """FLAG_EMISSIVE: the sphere of index `sphere` (< 8, kept whatever set_spheres holds) gives off light; None or zeros: it does not."""
        _check(lib().rwr_scene_set_sphere_emission(self._h, sphere, _p(self._radiance(radiance))))

    def _get_emission(self, fn, index: int):
        on = C.c_int(0)
        r = np.zeros(3, np.float32)
        _check(fn(self._h, index, C.byref(on), _p(r)))
        return r if on.value else None

    def get_part_emission(self, part: int):
        """The part's radiance, float32[3], when it emits, else None (rwr_scene_get_part_emission)."""
        return self._get_emission(lib().rwr_scene_get_part_emission, part)

    def get_sphere_emission(self, sphere: int):
        """The sphere index's radiance, float32[3], when it emits, else None (rwr_scene_get_sphere_emission)."""
        return self._get_emission(lib().rwr_scene_get_sphere_emission, sphere)

    def last_emission_stats(self):
        """The shaded hits of the last render call that lay on an emitting surface (rwr_last_emission_stats)."""
        a = C.c_uint64(0)
        _check(lib().rwr_last_emission_stats(self._h, C.byref(a)))
        return int(a.value)

    def last_light_stats(self):
        """FLAG_LIGHT_SAMPLING: (light rays traced, those that reached their sphere, hits whose Le was suppressed or, under
        FLAG_LIGHT_MIS, weighted) of the last render call (rwr_last_light_stats)."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().rwr_last_light_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def last_part_light_stats(self):
        """FLAG_LIGHT_PARTS: the mesh light's share of last_light_stats' three counts (rwr_last_part_light_stats)."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().rwr_last_part_light_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def last_sky_light_stats(self):
        """FLAG_LIGHT_SKY: the sky's share of last_light_stats' three counts — light rays aimed at the image, those that reached it,
        misses of diffuse rays that were silenced or, under FLAG_LIGHT_MIS, weighted (rwr_last_sky_light_stats)."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().rwr_last_sky_light_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def set_triangles(self, triangles):
        """Single-triangle passes (the reference's dormant models/triangle), after the spheres."""
        triangles = np.ascontiguousarray(triangles, dtype=TRIANGLE_DTYPE)
        _check(lib().rwr_scene_set_triangles(self._h, _p(triangles) if len(triangles) else None, len(triangles)))

    def set_instances(self, instances):
        n = 0 if instances is None else len(instances)
        arr = None if n == 0 else np.ascontiguousarray(instances, dtype=INSTANCE_DTYPE)
        _check(lib().rwr_scene_set_instances(self._h, _p(arr), n))

    def resize(self, width: int, height: int):
        _check(lib().rwr_resize(self._h, _p(make_screen(width, height))))
        self.width, self.height = width, height

    def render(self, cam_inv, params=None, rows=None, strips=None):
        """rows = (row_begin, row_end): a band (rwr_render_rows); strips = (first_strip, strip_stride): every strip_stride-th
        8-row strip (rwr_render_strips); neither: the whole frame."""
        if strips is not None:
            _check(lib().rwr_render_strips(self._h, _p(cam_inv), _p(params), strips[0], strips[1]))
        elif rows is None:
            _check(lib().rwr_render(self._h, _p(cam_inv), _p(params)))
        else:
            _check(lib().rwr_render_rows(self._h, _p(cam_inv), _p(params), rows[0], rows[1]))

    def render_call(self, cam_inv, params, rows=None, strips=None):
        """A zero-argument callable that enqueues one frame; arguments are marshalled
        once so that the per-frame host cost is one foreign call."""
        fn, h = (lib().rwr_render_strips if strips is not None else lib().rwr_render_rows), self._h
        a, b = _p(cam_inv), _p(params)
        if strips is None and rows is None:
            rows = (0, self.height)
        r0, r1 = (C.c_uint32(strips[0]), C.c_uint32(strips[1])) if strips is not None else (C.c_uint32(rows[0]), C.c_uint32(rows[1]))

        def call(_keep=(cam_inv, params)):
            rc = fn(h, a, b, r0, r1)
            if rc:
                _check(rc)

        return call

    def loop_call(self, cam: np.ndarray, keys: list[int], params, speed: float = CONTROLLER_SPEED, render: bool = True):
        """One iteration of the reference's redraw loop (State::update + State::render, src/lib.rs:994-1010,1335-1337) per call:
        CircleCameraController::update_camera with the next key mask of `keys` (cycled), CameraInvUniform::update_view_proj,
        rwr_render.  Arguments are marshalled once; `cam` is advanced in place.  render=False: the host side alone."""
        L, h = lib(), self._h
        upd, inv, ren = L.rwr_circle_controller_update, L.rwr_camera_build_inv_uniform, L.rwr_render
        uni = np.zeros(1, dtype=CAMERA_INV_DTYPE)
        pc, pu, pp = _p(cam), _p(uni), _p(params)
        sp = C.c_float(speed)
        masks = [C.c_uint32(k) for k in keys]
        state = [0]

        def call(_keep=(cam, uni, params)):
            i = state[0]
            state[0] = i + 1 if i + 1 < len(masks) else 0
            rc = upd(sp, masks[i], pc) or inv(pc, pu) or (ren(h, pu, pp) if render else 0)
            if rc:
                _check(rc)

        return call

    def synchronize(self):
        _check(lib().rwr_synchronize(self._h))

    def readback(self, aux: bool = False) -> dict:
        h, w = self.height, self.width
        out = {"color": np.zeros((h, w, 4), np.uint8), "depth": np.zeros((h, w), np.float32)}
        if aux:
            out["color_f32"] = np.zeros((h, w, 4), np.float32)
            out["obj_id"] = np.zeros((h, w), np.int32)
            out["hit_t"] = np.zeros((h, w), np.float32)
        _check(lib().rwr_readback(self._h, _p(out["color"]), _p(out["depth"]), _p(out.get("color_f32")),
                                  _p(out.get("obj_id")), _p(out.get("hit_t"))))
        return out

    def device_targets(self) -> tuple[int, int]:
        a, b = C.c_void_p(), C.c_void_p()
        _check(lib().rwr_get_device_targets(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def timer_begin(self):
        _check(lib().rwr_timer_begin(self._h))

    def timer_end(self) -> float:
        ms = C.c_float()
        _check(lib().rwr_timer_end(self._h, C.byref(ms)))
        return ms.value

    def timer_stop(self):
        """Enqueue the end event of the interval without waiting for it (rwr_timer_stop)."""
        _check(lib().rwr_timer_stop(self._h))

    def timer_elapsed(self) -> float:
        ms = C.c_float()
        _check(lib().rwr_timer_elapsed(self._h, C.byref(ms)))
        return ms.value

    def set_frames_in_flight(self, n: int):
        _check(lib().rwr_ctx_set_frames_in_flight(self._h, n))

    def set_kernel_timing(self, every_n: int):
        _check(lib().rwr_ctx_set_kernel_timing(self._h, every_n))

    def kernel_timing_stats(self) -> tuple[float, int]:
        mean, n = C.c_double(), C.c_uint32()
        _check(lib().rwr_kernel_timing_stats(self._h, C.byref(mean), C.byref(n)))
        return mean.value, n.value

    def selftest_exact_math(self, normalize_count: int = 1 << 30, seed: int = 1) -> tuple[int, int, int, int]:
        out = (C.c_uint64 * 4)()
        _check(lib().rwr_selftest_exact_math(self._h, normalize_count, seed, out))
        return tuple(int(v) for v in out)

    def selftest_exact_div(self, count: int = 1 << 30, seed: int = 1) -> tuple[int, int, int, int]:
        out = (C.c_uint64 * 4)()
        _check(lib().rwr_selftest_exact_div(self._h, count, seed, out))
        return tuple(int(v) for v in out)

    def selftest_sobol(self, pixel, sample, dim, seed) -> np.ndarray:
        """FLAG_SOBOL's 32-bit word for every tuple (pixel[i], sample[i], dim[i], seed[i]), evaluated by the kernels' device
        function (rwr_selftest_sobol)."""
        cols = [np.ascontiguousarray(a, dtype=np.uint32).ravel() for a in (pixel, sample, dim, seed)]
        n = len(cols[0])
        if any(len(c) != n for c in cols):
            raise ValueError("the four columns must have one length")
        out = np.zeros(n, np.uint32)
        _check(lib().rwr_selftest_sobol(self._h, *[c.ctypes.data_as(C.c_void_p) for c in cols], n, out.ctypes.data_as(C.c_void_p)))
        return out

    def selftest_sky_image(self, dirs) -> np.ndarray:
        """FLAG_SKY_IMAGE's S_img(D) of the context's image for every row of `dirs` (float32 (N, 3)), evaluated by the kernels' device
        function (rwr_selftest_sky_image): float32 (N, 3).  RwrError(ERR_NOT_READY) while no image is held."""
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        out = np.zeros_like(d)
        _check(lib().rwr_selftest_sky_image(self._h, _p(d), len(d), _p(out)))
        return out

    def selftest_sky_light(self, u4, normal=(0.0, 1.0, 0.0), n_lights: int = 1) -> dict:
        """FLAG_LIGHT_SKY's draw and factor on the context's image for every row of `u4` (float32 (N, 4), uniforms in [0, 1)), evaluated
        by the kernels' device functions (rwr_selftest_sky_light): {"omega": float32 (N, 3), "texel": uint32 (N, 2) column and row,
        "P": float32 (N,), "g": float32 (N,)}.  RwrError(ERR_NOT_READY) while no image is held or the image is all black."""
        u = np.ascontiguousarray(u4, dtype=np.float32).reshape(-1, 4)
        nrm = np.ascontiguousarray(normal, dtype=np.float32).reshape(3)
        out = np.zeros((len(u), 8), np.float32)
        _check(lib().rwr_selftest_sky_light(self._h, _p(u), len(u), _p(nrm), int(n_lights), _p(out)))
        return {"omega": out[:, 0:3].copy(), "texel": out[:, 3:5].copy().view(np.uint32), "P": out[:, 5].copy(), "g": out[:, 6].copy()}

    def measure_valu_clock(self, waves_per_simd: int = 8) -> dict:
        """Shader clock (MHz) and cycles a SIMD spends per wave64 v_fma_f32 / v_pk_fma_f32, measured under load."""
        out = (C.c_double * 4)()
        _check(lib().rwr_measure_valu_clock(self._h, waves_per_simd, out))
        return {"shader_mhz": out[0], "cycles_per_v_fma_f32": out[1], "cycles_per_v_pk_fma_f32": out[2], "shader_mhz_pk": out[3]}

    def dist_init(self, rank: int, world: int, unique_id: bytes):
        assert len(unique_id) == DIST_ID_BYTES
        buf = (C.c_uint8 * DIST_ID_BYTES).from_buffer_copy(unique_id)
        _check(lib().rwr_dist_init(self._h, rank, world, buf))

    def dist_gather(self, root: int = 0):
        """The frame's single collective: every rank's finished RGBA8 band to `root` (RCCL, stream-ordered)."""
        _check(lib().rwr_dist_gather_rgba8(self._h, root))

    def dist_gather_call(self, root: int = 0, strips: bool = False):
        """strips: the ranks rendered the interleaved partition (render(..., strips=(rank, world)))"""
        fn, h, r = (lib().rwr_dist_gather_strips_rgba8 if strips else lib().rwr_dist_gather_rgba8), self._h, C.c_int(root)

        def call():
            rc = fn(h, r)
            if rc:
                _check(rc)

        return call

    def dist_loopback_deposit(self, rank: int, world: int, strips: bool = True):
        """One-GPU self-test of the gather: `rank`'s side on the frame just rendered, a device copy in place of Send/Recv."""
        _check(lib().rwr_dist_loopback_deposit(self._h, rank, world, 1 if strips else 0))

    def dist_loopback_finish(self, world: int, strips: bool = True):
        _check(lib().rwr_dist_loopback_finish(self._h, world, 1 if strips else 0))

    def dist_readback(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), np.uint8)
        _check(lib().rwr_dist_readback(self._h, _p(out)))
        return out

    def dist_barrier(self):
        _check(lib().rwr_dist_barrier(self._h))

    def dist_destroy(self):
        _check(lib().rwr_dist_destroy(self._h))

    def clock_probe_start(self, micros: int):
        _check(lib().rwr_clock_probe_start(self._h, micros))

    def clock_probe_read(self) -> float:
        mhz = C.c_double()
        _check(lib().rwr_clock_probe_read(self._h, C.byref(mhz)))
        return mhz.value

    def last_render_stats(self) -> tuple[int, int]:
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib().rwr_last_render_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def frame_setup_launches(self) -> int:
        """k_frame_setup launches of this context so far (rwr_frame_setup_launches): a frame whose slot still holds the records of
        its camera, screen, rows and scene adds none (RWR_SETUP_CACHE=0: every frame adds one)."""
        n = C.c_uint64()
        _check(lib().rwr_frame_setup_launches(self._h, C.byref(n)))
        return n.value

    def ray_plane_stats(self) -> tuple[int, int]:
        """(k_ray_plane launches, frames that loaded their ray directions from a slot's kept plane) of this context so far
        (rwr_ray_plane_stats); (0, 0) for ever with RWR_RAY_PLANE=0."""
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib().rwr_ray_plane_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def tile_classes(self) -> np.ndarray:
        """The class words of the frame rendered last (rwr_debug_tile_classes), one per 32x4-pixel tile of the frame kernel's grid, as
        a (2 * grid_y, 2 * grid_x) uint32 array: entry [ty, tx] is the tile whose pixels start at x = 32 tx, at row 4 (ty & 1) of
        the launch's strip ty // 2.  Bits 0-1: faces (0 none, 1 one, 2 more), bits 8-15: the one face, bits 16-23: the spheres whose
        rectangles touch the tile.  Waits for that frame alone; RwrError (NOT_READY) when the frame has none."""
        gx, gy = C.c_uint32(), C.c_uint32()
        _check(lib().rwr_debug_tile_classes(self._h, None, 0, C.byref(gx), C.byref(gy)))
        words = np.empty(4 * gx.value * gy.value, np.uint32)
        _check(lib().rwr_debug_tile_classes(self._h, _p(words), words.size, C.byref(gx), C.byref(gy)))
        return np.ascontiguousarray(words.reshape(gy.value, gx.value, 2, 2).transpose(0, 2, 1, 3).reshape(2 * gy.value, 2 * gx.value))

    def tile_cover(self) -> np.ndarray:
        """The cover words of the frame rendered last (rwr_debug_tile_cover), laid out like tile_classes(): 1 where a frame served
        from the slot's kept records found every pixel pair of a one-face tile hitting, 0 elsewhere and after every setup launch."""
        gx, gy = C.c_uint32(), C.c_uint32()
        _check(lib().rwr_debug_tile_cover(self._h, None, 0, C.byref(gx), C.byref(gy)))
        words = np.empty(4 * gx.value * gy.value, np.uint32)
        _check(lib().rwr_debug_tile_cover(self._h, _p(words), words.size, C.byref(gx), C.byref(gy)))
        return np.ascontiguousarray(words.reshape(gy.value, gx.value, 2, 2).transpose(0, 2, 1, 3).reshape(2 * gy.value, 2 * gx.value))

    def tile_cover_stats(self) -> tuple[int, int]:
        """(frames of this context so far that looked at cover words, tiles the frame rendered last took as covered)
        (rwr_tile_cover_stats); (0, 0) for ever with RWR_TILE_COVER=0."""
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib().rwr_tile_cover_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def lean_rest_stats(self) -> int:
        """Frames of this context so far that the frame kernel's lean resting form rendered (rwr_lean_rest_stats); 0 for ever with
        RWR_LEAN_REST=0."""
        a = C.c_uint64()
        _check(lib().rwr_lean_rest_stats(self._h, C.byref(a)))
        return a.value

    def last_traversal_plan(self) -> dict:
        """How the last wavefront frame walked the BVH per lane (rwr_last_traversal_plan): {"trace": plan, "shadow": plan}, a plan
        being {"launches", "nodes_in_lds", "stack16", "wide"} - all 0 for a stage the frame did not have.  RWR_WF_STACK16=0 (read
        when the context is created): 32-bit stack entries whatever the scene's size."""
        t, s = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
        _check(lib().rwr_last_traversal_plan(self._h, _p(t), _p(s)))
        names = ("launches", "nodes_in_lds", "stack16", "wide")
        return {"trace": dict(zip(names, map(int, t))), "shadow": dict(zip(names, map(int, s)))}

    def last_shadow_stats(self) -> tuple[int, int]:
        """(shadow rays traced by the last render call, how many of them were occluded); (0, 0) without FLAG_SHADOWS."""
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib().rwr_last_shadow_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def accum_reset(self):
        """The next FLAG_ACCUMULATE frame starts a new accumulation."""
        _check(lib().rwr_accum_reset(self._h))

    def accum_samples(self) -> int:
        """Samples per pixel held by the image of the frame rendered last (0: it did not accumulate)."""
        n = C.c_uint64()
        _check(lib().rwr_accum_samples(self._h, C.byref(n)))
        return n.value

    def set_denoise_params(self, iterations=None, sigma_color=None, normal_cos_min=None, depth_rel=None):
        """The FLAG_DENOISE filter's parameters (rwr_denoise_set_params); an argument left out keeps its value, no argument at all
        restores the defaults.  Out of range: RwrError(ERR_INVALID_ARGUMENT), and the parameters stay."""
        given = {"iterations": iterations, "sigma_color": sigma_color, "normal_cos_min": normal_cos_min, "depth_rel": depth_rel}
        if all(v is None for v in given.values()):
            _check(lib().rwr_denoise_set_params(self._h, None))
            return
        p = np.zeros(1, dtype=DENOISE_PARAMS_DTYPE)
        for k, v in self.denoise_params().items():
            p[k] = v if given[k] is None else given[k]
        _check(lib().rwr_denoise_set_params(self._h, _p(p)))

    def denoise_params(self) -> dict:
        p = np.zeros(1, dtype=DENOISE_PARAMS_DTYPE)
        _check(lib().rwr_denoise_get_params(self._h, _p(p)))
        return {"iterations": int(p["iterations"][0]), "sigma_color": float(p["sigma_color"][0]),
                "normal_cos_min": float(p["normal_cos_min"][0]), "depth_rel": float(p["depth_rel"][0])}

    def set_tonemap_params(self, curve=None, auto_exposure=None, exposure=None, key=None, white=None):
        """The FLAG_TONEMAP stage's parameters (rwr_tonemap_set_params); an argument left out keeps its value, no argument at all
        restores the defaults.  Out of range or NaN: RwrError(ERR_INVALID_ARGUMENT), and the parameters stay.  No history restarts."""
        given = {"curve": curve, "auto_exposure": auto_exposure, "exposure": exposure, "key": key, "white": white}
        if all(v is None for v in given.values()):
            _check(lib().rwr_tonemap_set_params(self._h, None))
            return
        p = np.zeros(1, dtype=TONEMAP_PARAMS_DTYPE)
        for k, v in self.tonemap_params().items():
            p[k] = v if given[k] is None else given[k]
        _check(lib().rwr_tonemap_set_params(self._h, _p(p)))

    def tonemap_params(self) -> dict:
        p = np.zeros(1, dtype=TONEMAP_PARAMS_DTYPE)
        _check(lib().rwr_tonemap_get_params(self._h, _p(p)))
        return {"curve": int(p["curve"][0]), "auto_exposure": int(p["auto_exposure"][0]), "exposure": float(p["exposure"][0]),
                "key": float(p["key"][0]), "white": float(p["white"][0])}

    def last_tonemap_stats(self) -> tuple[int, int, float]:
        """(log_sum, count, exposure) of the last render call (rwr_last_tonemap_stats): the measure's two sums and the frame's E as a
        float32 value; (0, 0, exposure) for a manual frame, (0, 0, 0.0) for a frame without the flag.  Waits for the frame."""
        a, b, e = C.c_int64(0), C.c_uint32(0), C.c_float(0.0)
        _check(lib().rwr_last_tonemap_stats(self._h, C.byref(a), C.byref(b), C.byref(e)))
        return int(a.value), int(b.value), float(e.value)

    def set_reproject_params(self, max_history=None, normal_cos_min=None, depth_rel=None):
        """The FLAG_REPROJECT stage's parameters (rwr_reproject_set_params); an argument left out keeps its value, no argument at all
        restores the defaults.  Out of range or NaN: RwrError(ERR_INVALID_ARGUMENT), and the parameters stay.  Every accepted call
        starts a new history."""
        given = {"max_history": max_history, "normal_cos_min": normal_cos_min, "depth_rel": depth_rel}
        if all(v is None for v in given.values()):
            _check(lib().rwr_reproject_set_params(self._h, None))
            return
        p = np.zeros(1, dtype=REPROJECT_PARAMS_DTYPE)
        for k, v in self.reproject_params().items():
            p[k] = v if given[k] is None else given[k]
        _check(lib().rwr_reproject_set_params(self._h, _p(p)))

    def reproject_params(self) -> dict:
        p = np.zeros(1, dtype=REPROJECT_PARAMS_DTYPE)
        _check(lib().rwr_reproject_get_params(self._h, _p(p)))
        return {"max_history": int(p["max_history"][0]), "normal_cos_min": float(p["normal_cos_min"][0]), "depth_rel": float(p["depth_rel"][0])}

    def reproject_reset(self):
        """The next FLAG_REPROJECT frame starts a new history."""
        _check(lib().rwr_reproject_reset(self._h))

    def reproject_frames(self) -> int:
        """Frames the history of the frame rendered last holds, k + 1 (0: it did not reproject)."""
        n = C.c_uint64()
        _check(lib().rwr_reproject_frames(self._h, C.byref(n)))
        return n.value

    def last_reproject_stats(self) -> tuple[int, int, int]:
        """(reused, fresh, background) pixels of the last render call; they add up to width * height (rwr_last_reproject_stats)."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().rwr_last_reproject_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def reproject_history(self) -> np.ndarray:
        """The (H, W) float32 plane n' of the frame rendered last (rwr_reproject_readback); it synchronises."""
        out = np.zeros((self.height, self.width), np.float32)
        _check(lib().rwr_reproject_readback(self._h, _p(out)))
        return out

    def sky_set_params(self, zenith=None, horizon=None):
        """The FLAG_SKY sky's two colours (rwr_sky_set_params), each three floats in [0, 16]; an argument left out keeps its value,
        no argument at all restores the defaults.  Out of range or NaN: RwrError(ERR_INVALID_ARGUMENT), and the parameters stay."""
        if zenith is None and horizon is None:
            _check(lib().rwr_sky_set_params(self._h, None))
            return
        p = np.zeros(1, dtype=SKY_PARAMS_DTYPE)
        now = self.sky_get_params()
        p["zenith"] = now["zenith"] if zenith is None else np.asarray(zenith, np.float32)
        p["horizon"] = now["horizon"] if horizon is None else np.asarray(horizon, np.float32)
        _check(lib().rwr_sky_set_params(self._h, _p(p)))

    def sky_get_params(self) -> dict:
        """{"zenith": float32[3], "horizon": float32[3]} (rwr_sky_get_params)."""
        p = np.zeros(1, dtype=SKY_PARAMS_DTYPE)
        _check(lib().rwr_sky_get_params(self._h, _p(p)))
        return {"zenith": p["zenith"][0].copy(), "horizon": p["horizon"][0].copy()}

    def sky_set_image(self, img):
        """The FLAG_SKY_IMAGE sky's octahedral map (rwr_sky_set_image): float32 (n, n, 3), row j <-> v, column i <-> u, 2 <= n <= 2048,
        every component finite and in [0, 64]; None removes the image.  Anything else: RwrError(ERR_INVALID_ARGUMENT), and the image
        stays.  Every accepted call advances the image's generation (sky_get_image_info)."""
        if img is None:
            _check(lib().rwr_sky_set_image(self._h, None, 0))
            return
        a = np.ascontiguousarray(img, dtype=np.float32)
        if a.ndim != 3 or a.shape[0] != a.shape[1] or a.shape[2] != 3:
            raise ValueError(f"a sky image is (n, n, 3), not {a.shape}")
        _check(lib().rwr_sky_set_image(self._h, _p(a), a.shape[0]))

    def sky_get_image_info(self) -> dict:
        """{"n": side of the image held (0: none), "generation": how many accepted sky_set_image calls} (rwr_sky_get_image_info)."""
        n, gen = C.c_uint32(0), C.c_uint64(0)
        _check(lib().rwr_sky_get_image_info(self._h, C.byref(n), C.byref(gen)))
        return {"n": int(n.value), "generation": int(gen.value)}

    def sky_get_light_info(self) -> dict:
        """{"n": side of the FLAG_LIGHT_SKY sampling table a frame would use (0: no image, or an all-black one), "generation": the
        image generation it was built for} (rwr_sky_get_light_info); builds the table if the image changed since."""
        n, gen = C.c_uint32(0), C.c_uint64(0)
        _check(lib().rwr_sky_get_light_info(self._h, C.byref(n), C.byref(gen)))
        return {"n": int(n.value), "generation": int(gen.value)}

    def shadow_set_params(self, mesh=None, sphere=None):
        """The FLAG_SOFT_SHADOWS radii of the two lights (rwr_shadow_set_params): `mesh` the mesh shader's light, `sphere` the sphere
        shader's, each the tangent of the half-angle a hit sees the light under, in [0, 1]; an argument left out keeps its value, no
        argument at all restores the defaults.  Out of range or NaN: RwrError(ERR_INVALID_ARGUMENT), and the parameters stay."""
        if mesh is None and sphere is None:
            _check(lib().rwr_shadow_set_params(self._h, None))
            return
        p = np.zeros(1, dtype=SHADOW_PARAMS_DTYPE)
        now = self.shadow_get_params()
        p["mesh_light_radius"] = now["mesh"] if mesh is None else np.float32(mesh)
        p["sphere_light_radius"] = now["sphere"] if sphere is None else np.float32(sphere)
        _check(lib().rwr_shadow_set_params(self._h, _p(p)))

    def shadow_get_params(self) -> dict:
        """{"mesh": float32, "sphere": float32} (rwr_shadow_get_params)."""
        p = np.zeros(1, dtype=SHADOW_PARAMS_DTYPE)
        _check(lib().rwr_shadow_get_params(self._h, _p(p)))
        return {"mesh": np.float32(p["mesh_light_radius"][0]), "sphere": np.float32(p["sphere_light_radius"][0])}


def csrc_tree() -> str:
    """Hash of the sources librwr_hip.so is built from (csrc/, host/, include/rwr_hip.h, Makefile): ties a set of profiler
    counters (profiles/r*_counters.json `_csrc_tree`) to the code they were measured on, with or without a .git directory."""
    import hashlib

    h = hashlib.sha256()
    files = []
    for sub in ("csrc", "host"):
        d = os.path.join(_HERE, sub)
        files += [os.path.join(d, f) for f in os.listdir(d) if f.endswith((".h", ".hpp", ".hip", ".cpp"))]
    files += [os.path.join(_HERE, "Makefile"), HEADER_PATH]
    for f in sorted(files):
        h.update(os.path.relpath(f, _HERE).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def sky_image_from_equirect(arr, n: int, scale: float = 1.0) -> np.ndarray:
    """A latitude-longitude picture, float32 (h, w, 3) — row 0 straight up, the centre column direction (0, 0, -1), columns
    increasing towards +x — as the (n, n, 3) octahedral map Context.sky_set_image takes, times `scale`, clamped to [0, 64]
    (rwr_sky_image_from_equirect; host only, needs no device)."""
    a = np.ascontiguousarray(arr, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"a picture is (h, w, 3), not {a.shape}")
    n = int(n)
    if not 2 <= n <= SKY_IMAGE_SIZE_MAX:   # (ahead of the output's allocation; the library's own refusal, in its words)
        raise RwrError(ERR_INVALID_ARGUMENT, f"sky image size {n}: 2 ... {SKY_IMAGE_SIZE_MAX}")
    out = np.zeros((n, n, 3), np.float32)
    _check(lib().rwr_sky_image_from_equirect(_p(a), a.shape[1], a.shape[0], float(scale), n, _p(out)))
    return out


def exported_symbols_declared_in_header() -> list[str]:
    """Names of every RWR_API function declared in include/rwr_hip.h."""
    import re

    with open(HEADER_PATH, "r") as fh:
        text = fh.read()
    return sorted(set(re.findall(r"RWR_API\s+[^;(]*?\b(rwr_[a-z0-9_]+)\s*\(", text)))
