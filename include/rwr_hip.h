/*
 * rwr_hip.h — C ABI of the MI355X-native ray/path tracer (librwr_hip.so).
 *
 * This is the drop-in boundary for the reference's hot path
 * (clejacquet/rust-wgpu-raytracing): everything `State::render` hands to its
 * three WGSL compute passes through wgpu bind groups crosses this ABI as plain
 * pointers and sizes instead.  The reference has no FFI of its own; each entry
 * point below cites the reference interface it replaces (paths relative to
 * /root/reference/).  The Rust binding a maintainer would add is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - every function returns RWR_OK (0) or a negative rwr_status; the message
 *     for the calling thread's last failure is rwr_last_error_string().
 *     Nothing aborts or panics (the reference unwrap()s: lib.rs:275,284,303,566).
 *   - one context = one GPU = one caller thread (the reference's State is !Send,
 *     lib.rs:256).  Rendering is asynchronous on the context's HIP stream(s);
 *     rwr_readback() waits for the frame rendered last, rwr_synchronize() for
 *     every frame in flight (rwr_ctx_set_frames_in_flight).
 *   - caller owns host arrays; uploads copy; the context owns device memory
 *     until rwr_ctx_destroy().
 *   - all PODs are layout-identical to the reference's #[repr(C)] structs.
 *   - framebuffer row 0 is the BOTTOM image row (y_nds grows with the row
 *     index, compute.wgsl:152; the reference's blit compensates, lib.rs:39-64).
 */
#ifndef RWR_HIP_H
#define RWR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define RWR_API __attribute__((visibility("default")))
#else
#define RWR_API
#endif

typedef enum rwr_status {
    RWR_OK = 0,
    RWR_ERR_INVALID_ARGUMENT = -1,
    RWR_ERR_HIP = -2,            /* a HIP runtime call failed (no device, OOM, launch failure) */
    RWR_ERR_NOT_READY = -3,      /* render before resize / scene upload */
    RWR_ERR_IO = -4,             /* loader: file missing / unreadable   (anyhow::Error in resources.rs) */
    RWR_ERR_PARSE = -5,          /* loader: malformed OBJ/MTL/PNG/JPEG */
    RWR_ERR_UNSUPPORTED = -6
} rwr_status;

/* ------------------------------------------------------------------ PODs -- */

/* CameraInvUniform, src/lib.rs:86-93 — binding g0 b3 (compute.wgsl:10-14,57-58).
 * Matrices are column-major: m[col][row] (cgmath `Into<[[f32;4];4]>`). */
typedef struct rwr_camera_inv_uniform {
    float viewmodel_inv[4][4];
    float proj_inv[4][4];       /* = OPENGL_TO_WGPU_MATRIX * perspective^-1, lib.rs:109 */
    float origin[3];
    uint32_t _padding;
} rwr_camera_inv_uniform;

/* Screen, src/lib.rs:216-221 — binding g0 b4 (compute.wgsl:16-19,60-61). */
typedef struct rwr_screen {
    uint32_t width, height;
} rwr_screen;

/* ModelVertexSmall, src/model.rs:45-63 — binding g0 b5 element (compute.wgsl:27-30,63-64). */
typedef struct rwr_model_vertex_small {
    float position[3];
    float pad0;
    float tex_coords[2];
    float pad1[2];
} rwr_model_vertex_small;

/* ModelFaceSmall, src/model.rs:65-79 — binding g0 b6 element (compute.wgsl:66-67). */
typedef struct rwr_model_face_small {
    uint32_t indices[3];
    uint32_t pad0;
} rwr_model_face_small;

/* MaterialData, src/models/triangle_list/triangle_list.rs:24-33 — binding g0 b7 (compute.wgsl:32-36,69-70). */
typedef struct rwr_material_data {
    float ambient[3];  float pad0;
    float diffuse[3];  float pad1;
    float specular[3]; float pad2;
} rwr_material_data;

/* SphereBufferData, src/models/sphere/sphere.rs:10-15 — sphere binding g0 b5 (sphere/compute.wgsl:21-24,49-50). */
typedef struct rwr_sphere_buffer_data {
    float center[3];
    float radius;
} rwr_sphere_buffer_data;

/* TriangleBufferData, src/models/triangle/triangle.rs:10-19 — the single-triangle model's uniform
 * (triangle/compute.wgsl:21-25,50-51).  The reference builds this model type but never dispatches it. */
typedef struct rwr_triangle_buffer_data {
    float p0[3]; float pad0;
    float p1[3]; float pad1;
    float p2[3]; float pad2;
} rwr_triangle_buffer_data;

/* InstanceRaw, src/lib.rs:129-134 (computed but never bound by the reference;
 * used here by the instanced configs).  Column-major model matrix; must be rigid
 * (rotation + translation). */
typedef struct rwr_instance_raw {
    float model[4][4];
} rwr_instance_raw;

/* Camera, src/camera.rs:3-11 (cgmath Point3/Vector3 flattened). */
typedef struct rwr_camera {
    float eye[3];
    float target[3];
    float up[3];
    float aspect;
    float fovy;   /* degrees */
    float znear;
    float zfar;
} rwr_camera;

/* Extension (no reference counterpart): how many samples / bounces to trace.
 * With spp > 1 or max_bounces > 0 a pixel is (sum over samples of E(h0) + albedo(h0) * E(h1)) / spp, E being the reference's
 * local shading.  Part of that definition: every term a sample adds is clamped per channel — E(h0) to
 * [0, 16], albedo * E(h1) to [0, 64], NaN counting as 0 — so that the sums have a fixed range (they are added as fixed
 * point, in any order, and the frame is bit-reproducible).  The reference's materials (components <= 1) come nowhere near;
 * a material with Ka = 20 is clamped, in the oracle's or_render_path as here.  spp 1 / max_bounces 0 is the reference frame:
 * nothing is clamped before the rgba8unorm store.
 * Deeper paths (RWR_FLAG_MULTI_BOUNCE, max_bounces = B <= RWR_MAX_BOUNCES): a sample adds, for k = 1 ... B, the term
 * T(k-1) * E(hk) clamped per channel to [0, 64] (NaN counting as 0), with T0 = albedo(h0) and Tk = T(k-1) * albedo(hk).  Ray k
 * starts at P(k-1) + 1e-4 n(k-1) (P = origin + t * direction; n = the face normal flipped towards the ray, or the sphere's
 * outward normal; normal maps never change it) and leaves in the cosine-distributed direction about n(k-1) drawn from RNG
 * dimensions 2 + 16 (k-1) ... 17 + 16 (k-1) of (global pixel, global sample, seed): for k = 1 the one-bounce ray.  hk is its
 * nearest hit, spheres in order then faces, ties to the earlier candidate; a miss ends the path.  Depth, id and t planes
 * report primary sample 0 whatever B is, and a path of B bounces is a prefix of the path of B + 1. */
typedef struct rwr_render_params {
    uint32_t spp;          /* >= 1.  1 = the reference's single centre sample        */
    uint32_t max_bounces;  /* 0 = reference (primary rays only); 1 = one diffuse bounce; up to
                              RWR_MAX_BOUNCES with RWR_FLAG_MULTI_BOUNCE (else > 1 is RWR_ERR_UNSUPPORTED) */
    uint32_t seed;         /* RNG stream key; results do not depend on GPU count     */
    uint32_t flags;        /* RWR_FLAG_*                                              */
} rwr_render_params;

enum {
    RWR_FLAG_AUX_OUTPUTS = 1u << 0, /* also produce float colour, object id and hit distance planes */
    RWR_FLAG_NO_CULL     = 1u << 1, /* debug: brute-force every face for every pixel (reference loop order) */
    RWR_FLAG_USE_BVH     = 1u << 2, /* reference frame only: the mesh pass traverses the BVH per ray instead of
                                       walking per-tile candidate lists (better when many small faces share a
                                       tile, e.g. a distant mesh); same result bit for bit.  The context picks
                                       this kernel by itself when a scene of more than 256 faces projects to
                                       faces far smaller than a tile */
    RWR_FLAG_ORTHO_RAYS  = 1u << 3, /* every pass generates its rays with pixelToRay_ortho (defined, never called,
                                       in all three shaders: triangle_list/compute.wgsl:166-174): origin =
                                       camera.origin + (5 x_nds, 5 y_nds, 0), direction (0, 0, -1).  Reference
                                       frame only (spp 1, no bounce, no RWR_FLAG_USE_BVH) */
    RWR_FLAG_NORMAL_MAP  = 1u << 4, /* extension: mesh hits are shaded with the normal of their part's normal map
                                       (rwr_scene_set_normal_map; res/cube.mtl:13 `map_Bump`, which the reference parses
                                       nowhere: resources.rs:187-213 loads the diffuse texture only and compute.wgsl:226-229
                                       shades with the flat face normal).  Without the flag — the default — the frame is
                                       the reference's.  Visibility never changes; bounce rays still leave along the
                                       geometric normal */
    RWR_FLAG_ACCUMULATE  = 1u << 5, /* extension: progressive accumulation across frames (rwr_accum_reset, rwr_accum_samples).
                                       The frame traces global samples [N, N + spp), N = the samples the context's accumulation
                                       holds, and shows the mean of all N + spp: after frames of s1, s2, ... sK samples with an
                                       unchanged key, every plane (color, depth, and with RWR_FLAG_AUX_OUTPUTS color_f32, obj_id,
                                       hit_t) is, byte for byte, ONE frame without the flag of spp = s1 + ... + sK and the same
                                       seed, whenever that sum is >= 2 (depth / id / t report global sample 0 on every frame; spp
                                       may change from frame to frame).  Always the integrator, samples always jittered: a first
                                       accumulated frame of spp 1 is a jittered one-sample estimate, not the reference frame.
                                       KEY — the accumulation goes on only while all of these stay as they were: the camera
                                       uniform's 144 bytes, the screen size, the rows (rwr_render_rows / rwr_render_strips
                                       arguments), max_bounces, seed, flags but this bit, frames in flight, and the scene (any
                                       rwr_scene_* call that changes it, uploads included).  Any change starts over at N = 0, as
                                       do rwr_accum_reset and any frame rendered without the flag.  CAP: at most 2^24 samples
                                       per pixel (environment RWR_ACCUM_MAX_SAMPLES, read by rwr_ctx_create, lowers it); a
                                       frame that would go past it traces nothing and shows the image held; a first frame of
                                       more samples than the cap is RWR_ERR_INVALID_ARGUMENT.  With RWR_FLAG_ORTHO_RAYS,
                                       RWR_FLAG_USE_BVH or single-triangle passes: RWR_ERR_UNSUPPORTED.  Frames in flight and
                                       row bands / strips keep the contract (the sums are keyed by global pixel) */
    RWR_FLAG_MULTI_BOUNCE = 1u << 6,/* extension: max_bounces may be 0 ... RWR_MAX_BOUNCES (diffuse paths of that many bounces,
                                       rwr_render_params); more is RWR_ERR_INVALID_ARGUMENT.  With max_bounces <= 1 every plane
                                       is the frame without the flag, byte for byte.  RWR_FLAG_USE_BVH, RWR_FLAG_ORTHO_RAYS and
                                       single-triangle passes stay reference-frame only.  rwr_last_render_stats' bounce_rays
                                       counts the rays of every bounce */
    RWR_FLAG_SHADOWS = 1u << 7,     /* extension: shadow rays towards the reference's two directional lights.  Without the flag
                                       every frame is what it was, byte for byte.  With it:
                                       1. The frame always takes the path integrator, also at spp 1 / max_bounces 0.  Samples are
                                          placed as without the flag (pixel centre at spp 1, jittered from spp 2; an accumulating
                                          frame: jittered).  Every term is clamped as in the integrator (E(h0) to [0, 16], later
                                          terms to [0, 64], NaN as 0), also at spp 1 / no bounce.  The depth, object id and t
                                          planes (sample 0) are unchanged by the flag, bit for bit.
                                       2. Every hit h the integrator shades (h0 and every bounce hit) has one shadow ray:
                                          origin P + 1e-4 n, P = origin + t * direction of the ray that found h, n the hit
                                          record's normal (face normal flipped towards the ray, sphere's outward normal; normal
                                          maps never change it) - operation for operation the origin of the bounce ray that
                                          leaves h; direction -normalize(kLightDir) in f32, kLightDir = (1, -1, -5) for a mesh
                                          hit and (1, -5, 1) for a sphere hit (the reference's two shaders have two lights).
                                          occluded(h): any sphere or any face (all instances, all parts) is hit by that ray in
                                          the reference's own sphereRayIntersect / triangleRayIntersect arithmetic.  No distance
                                          limit, and the face h lies on is not excluded: a surface whose ray-facing side looks
                                          away from the light shadows itself.
                                       3. The local shading E(h) of an occluded hit is its ambient part alone: the part's
                                          MaterialData.ambient for a mesh hit, (0.1, 0, 0) for a sphere hit.  Albedo, throughput,
                                          random numbers and every primary and bounce ray are those of the frame without the
                                          flag, bit for bit; term k is clamp(T(k-1) * E_V(h_k)) with the caps above.
                                       4. RWR_FLAG_ACCUMULATE, RWR_FLAG_MULTI_BOUNCE, RWR_FLAG_NORMAL_MAP, RWR_FLAG_AUX_OUTPUTS,
                                          RWR_FLAG_NO_CULL, instances, parts, frames in flight, row bands, strips and the multi-GPU
                                          gather keep their contracts.  With RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH or
                                          single-triangle passes: RWR_ERR_UNSUPPORTED.
                                       5. rwr_last_shadow_stats counts the shadow rays and how many were occluded. */
    RWR_FLAG_DENOISE = 1u << 8,     /* extension: an edge-avoiding a-trous filter (Dammertz et al. 2010) over the frame the integrator
                                       resolved, for frames of few samples.  Without the flag every frame is what it was, byte for
                                       byte, with no further launch or allocation.  With it:
                                       1. The frame always takes the path integrator, also at spp 1 / max_bounces 0 (as with
                                          RWR_FLAG_SHADOWS), and is rendered as if RWR_FLAG_AUX_OUTPUTS were set too: rwr_readback's three
                                          aux planes are available.  Samples, rays, random numbers and sums are those of the frame
                                          without the flag; depth, obj_id and hit_t (sample 0) are unchanged, bit for bit.
                                       2. c0 = the resolved color_f32 plane.  For i = 0 ... N-1 (N = iterations), step s = 2^i, pixel p:
                                          taps (dx, dy) in {-2 ... 2}^2, row-major, dy outer, q = p + s (dx, dy); a tap outside the
                                          frame is skipped.  Kernel weight h = k[|dx|] k[|dy|], k = {3/8, 1/4, 1/16}.  Geometry weight
                                          g in {0, 1}: a background pixel (id(p) = -1) keeps its colour, and a background tap has
                                          g = 0; id(q) = id(p): g = 1; two mesh faces (both ids >= 0): g = 1 iff
                                          dot3(nhat[id p], nhat[id q]) >= normal_cos_min (nhat = normalize(N) of the face as wound)
                                          and fabsf(t(p) - t(q)) <= depth_rel * fminf(t(p), t(q)); anything else (two different
                                          spheres, sphere against mesh): g = 0.  Colour weight w = 1 / (1 + d2 inv_i),
                                          d2 = (dr dr + dg dg) + db db of c_i(p) - c_i(q), inv_0 = 1 / (sigma_color sigma_color),
                                          inv_(i+1) = 4 inv_i.  Over the taps with g = 1, in tap order: sum += (h w) c_i(q) per
                                          channel, norm += h w; c_(i+1)(p).rgb = sum / norm.  All in f32, + - * / only.
                                       3. c_N replaces color_f32 (alpha is c0's); the rgba8 plane is its conversion, as the resolve's.
                                       4. RWR_FLAG_ACCUMULATE: the filter is a post-process of the image shown; the history never
                                          sees it.  Neither this bit nor rwr_denoise_set_params is part of the accumulation key; the
                                          key holds the effective flags (RWR_FLAG_AUX_OUTPUTS implied).
                                       5. rwr_render_rows / rwr_render_strips with the flag: RWR_ERR_UNSUPPORTED unless the call
                                          covers the whole frame (the filter reaches 62 pixels; a rank does not hold its neighbours'
                                          rows).  With RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH or single-triangle passes:
                                          RWR_ERR_UNSUPPORTED. */
    RWR_FLAG_SKY = 1u << 9,         /* extension: sky light — a bounce ray that leaves the scene returns the radiance of a sky gradient
                                       (rwr_sky_set_params) instead of nothing.  Without the flag every frame is what it was, byte for
                                       byte, with no further launch or allocation.  With it:
                                       1. S(D), per channel c in f32 with no contraction: u = fminf(fmaxf(0.5f * D.y + 0.5f, 0.0f), 1.0f),
                                          S_c = horizon_c + (zenith_c - horizon_c) * u.  World +y is up (the reference's Camera.up).
                                       2. When bounce ray k (k = 1 ... max_bounces) with direction D_k finds no hit - no sphere and no
                                          face of any instance or part - the sample adds term k = clamp(T(k-1) * S(D_k), 0, 64) per
                                          channel, NaN counting as 0, and the path ends as it does without the flag.  A generation
                                          still adds at most one term <= 64 per sample.
                                       3. Primary rays that miss are unchanged: background pixels keep their colour, alpha and
                                          obj_id = -1 (the sky is a light, not a backdrop).  Depth, obj_id and hit_t (sample 0) do not
                                          depend on the flag, bit for bit.
                                       4. max_bounces = 0: the flag is ignored, the frame is the frame without it, byte for byte.
                                          zenith = horizon = 0: every plane equals the frame without the flag, byte for byte.
                                       5. No random numbers are used; every primary, bounce and shadow ray is the one of the frame
                                          without the flag, bit for bit.  A sky term casts no shadow ray: rwr_last_shadow_stats and
                                          rwr_last_render_stats do not depend on the flag.  RWR_FLAG_MULTI_BOUNCE, RWR_FLAG_SHADOWS,
                                          RWR_FLAG_NORMAL_MAP, RWR_FLAG_AUX_OUTPUTS, RWR_FLAG_NO_CULL, RWR_FLAG_DENOISE, instances, parts,
                                          frames in flight, row bands, strips and the multi-GPU gather keep their contracts.
                                       6. RWR_FLAG_ACCUMULATE: this bit is part of the key, and while it is set so are the 24 bytes of
                                          rwr_sky_params: changing a parameter starts over at N = 0.  Without the bit,
                                          rwr_sky_set_params does not disturb an accumulation.
                                       7. With RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH or single-triangle passes: RWR_ERR_UNSUPPORTED.  The
                                          refusal comes first: it holds at max_bounces = 0 too, where item 4 would otherwise ignore the
                                          flag — a combination that is refused does not start to work when the bounces go to 0. */
    RWR_FLAG_MIRRORS = 1u << 10,    /* extension: mirror surfaces — a scene part or a sphere marked as a mirror (rwr_scene_set_part_mirror,
                                       rwr_scene_set_sphere_mirror) sends the reflection of the ray that found it onwards instead of a
                                       cosine-distributed ray.  Without the flag every frame is what it was, byte for byte, with no further
                                       launch or allocation.  With it:
                                       1. Let h be a hit a path goes on from (h0, or bounce hit h_k with k < max_bounces) on a mirror
                                          surface of reflectance R, D the direction of the ray that found it, n the reference's HitRecord
                                          normal (the face normal flipped towards the ray, or the sphere's outward normal; normal maps
                                          never change it).  The next ray starts where it always does, P + 1e-4 n, operation for
                                          operation the diffuse ray's and the shadow ray's origin.  Its direction, in f32 with no
                                          contraction: d = n.x D.x + n.y D.y + n.z D.z, D' = D - (2 d) n per component — not
                                          re-normalised (the hit tests take a direction of any length).
                                       2. Throughput: T(k) = T(k-1) * R in place of T(k-1) * albedo(h); T(0) = R at a mirror h0.
                                       3. The local term of h is unchanged: E(h) (with RWR_FLAG_SHADOWS the shadowed E(h)) is added as
                                          ever, only what the surface sends onwards becomes specular — a coated surface.  For a pure
                                          mirror give the part Ka = Ks = 0 and a black texture.  Primary-stage sums, sample-0 planes
                                          (depth, obj_id, hit_t), h0's shadow records and their part of rwr_last_shadow_stats therefore
                                          do not depend on the flag.
                                       4. No random number is read at a mirror hit; that generation's 16 RNG dimensions are skipped, not
                                          reused: a later diffuse hit h_j of the path still reads dimensions 2 + 16 (j - 1) ... 17 + 16 (j - 1).
                                       5. The nearest-hit rule, the clamps (term k to [0, 64], NaN as 0) and RWR_FLAG_SKY's term at a
                                          miss, T * S(D') — a mirror shows the sky — are untouched.  The first generation has as many
                                          rays as the frame without the flag; later ones differ, because paths go elsewhere.  R <= 1:
                                          the integrator's range analysis stands.
                                       6. max_bounces = 0, or no part of the scene and none of its spheres (indices below the count
                                          rwr_scene_set_spheres gave) is a mirror: the flag is ignored — cleared before the frame's kernels
                                          are chosen — and the frame is the frame without it, byte for byte, in the same kernels.
                                       7. RWR_FLAG_ACCUMULATE: this bit (after item 6) is part of the key, and every call of the two
                                          setters that is accepted changes the scene (as rwr_scene_set_spheres does): setting or
                                          clearing a mirror or changing R by one ulp starts over at N = 0 — with or without the flag,
                                          whether or not the value is new.  A refused call changes nothing: the accumulation goes on.
                                       8. RWR_FLAG_MULTI_BOUNCE, RWR_FLAG_SHADOWS, RWR_FLAG_SKY, RWR_FLAG_NORMAL_MAP, RWR_FLAG_AUX_OUTPUTS,
                                          RWR_FLAG_NO_CULL, RWR_FLAG_DENOISE, instances, parts, frames in flight, row bands, strips and the
                                          multi-GPU gather keep their contracts.  With RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH or
                                          single-triangle passes: RWR_ERR_UNSUPPORTED, whatever max_bounces is and whether or not a
                                          mirror is set (the refusal comes first, as RWR_FLAG_SKY's). */
    RWR_FLAG_GLASS = 1u << 11,      /* extension: glass surfaces — a scene part or a sphere marked as glass (rwr_scene_set_part_glass,
                                       rwr_scene_set_sphere_glass) of index eta and tint C reflects by Fresnel's law (Schlick's form),
                                       refracts by Snell's, and reflects totally on the way out beyond the critical angle.  Independent
                                       of RWR_FLAG_MIRRORS: each flag switches its own surfaces on; a glass surface in a frame without
                                       this flag is the diffuse surface it was.  Without the flag every frame is what it was, byte for
                                       byte, with no further launch or allocation.  With it, at a hit h a path goes on from (h0, or h_k
                                       with k < max_bounces) on a glass surface, all in f32 with no contraction:
                                       1. Dh = normalize3(D), the oracle's routine (three divisions by the length); D is the direction
                                          of the ray that found h (un-normalised after a mirror or a refraction).
                                       2. n is the reference's HitRecord normal.  A face: entering = !(N.D > 0) with the winner's stored
                                          N.D — outside is the side the winding's normal points to — and n_f = n, already flipped
                                          towards the ray.  A sphere: s = dot3(n, Dh), entering = !(s > 0), n_f = entering ? n : -n.
                                       3. c = fminf(1, fmaxf(0, -dot3(n_f, Dh))), e = entering ? 1.0f / eta : eta,
                                          k = 1 - (e e) (1 - c c).
                                       4. k < 0, total internal reflection: (a, b) = (1, 2 c), no random number is read, m = n_f.
                                       5. Otherwise ct = sqrtf(k), r0 = ((1 - eta) / (1 + eta))^2, x = 1 - (entering ? c : ct),
                                          F = r0 + (1 - r0) ((x x) (x x) x), u = rng_uniform(pixel, sample, d0, seed) with d0 the first
                                          dimension of the generation's block (2 for the ray that leaves h0, 2 + 16 k for the one that
                                          leaves h_k); the block's other 15 dimensions are skipped, as at a mirror.  u < F: a Fresnel
                                          reflection, (a, b) = (1, 2 c), m = n_f.  Else a transmission: (a, b) = (e, e c - ct), m = -n_f.
                                       6. The next ray: direction a Dh + b n_f per component (a*Dh.x + b*n_f.x), not re-normalised;
                                          origin P + 1e-4 m (P.x + m.x*1e-4f, P = O + t D on the ray's own D); throughput T * C in all
                                          three events (the choice has probability F and weight 1).
                                       7. The local term of h is unchanged, E(h) or the shadowed E(h): a coated surface, as a mirror.
                                          For clear glass give the part Ka = Ks = 0 and a black texture.  h's shadow ray keeps the
                                          origin P + 1e-4 n whatever side the path goes on from; glass occludes shadow rays like any
                                          surface.  Primary-stage sums, sample-0 planes, h0's shadow records and generation 1's ray
                                          count do not depend on the flag; the nearest-hit rule, the clamps, the sky's term at a miss
                                          and (C <= 1) the integrator's range analysis are untouched.
                                       8. max_bounces = 0, or no part of the scene and none of its spheres (indices below the count
                                          rwr_scene_set_spheres gave) is glass: the flag is ignored — cleared before the frame's kernels
                                          are chosen — and the frame is the frame without it, byte for byte, in the same kernels.
                                       9. RWR_FLAG_ACCUMULATE: this bit (after item 8) is part of the key; every accepted call of the
                                          glass setters changes the scene's generation, a refused one changes nothing.
                                       10. rwr_last_glass_stats counts the three events.  Every other flag, instances, parts, frames in
                                          flight, row bands, strips and the multi-GPU gather keep their contracts.  With
                                          RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH or single-triangle passes: RWR_ERR_UNSUPPORTED, whatever
                                          max_bounces is and whether or not a surface is glass. */
    RWR_FLAG_REPROJECT = 1u << 12,  /* extension: temporal reprojection — a low-sample frame is blended with the context's history of
                                       the frames before it, fetched where the point a pixel sees was seen last frame, while the
                                       camera moves (RWR_FLAG_ACCUMULATE converges only while it rests).  Without the flag every
                                       frame is what it was, byte for byte, with no further launch or allocation.  With it the frame
                                       is frame k = 0, 1, ... of the context's history:
                                       1. The frame always takes the path integrator and is rendered as if RWR_FLAG_AUX_OUTPUTS were
                                          set (as with RWR_FLAG_DENOISE).  It is traced exactly as the frame without the flag whose
                                          seed is params.seed + k (mod 2^32): c_now is that frame's resolved color_f32 plane; depth,
                                          obj_id, hit_t and the render, shadow and glass stats are that frame's, bit for bit.  The
                                          caller keeps seed fixed; the frames decorrelate through k.
                                       2. The history goes on while the screen, spp, max_bounces, seed, the effective flags but the
                                          RWR_FLAG_DENOISE bit, frames in flight, the scene (every accepted setter of a scene
                                          attribute changes it), the sky's parameters while the sky lights the frame, and
                                          rwr_reproject_params equal the previous reprojecting frame's.  The camera is NOT part of
                                          this key.  Anything else starts over at k = 0: rwr_resize, rwr_reproject_reset, a frame
                                          without the flag in between, an accepted rwr_reproject_set_params (also one that sets the
                                          values it already has).
                                       3. Per frame, from the camera uniform alone, in f32 with no contraction: W(x_nds, y_nds) =
                                          pixelToRay's world_vec before the normalise; c0 = W(0,0), cx = W(1,0) - c0,
                                          cy = W(0,1) - c0, nrm = cross3(cx, cy).  These, the origin o and the screen are what the
                                          history keeps of a frame's camera (primed below).
                                       4. Pixel p = (x, y) of frame k >= 1, id = obj_id(p), t = hit_t(p); the previous frame's history
                                          planes: colour h, length n, id', t'.  id = -1: out = c_now, n' = 0 (background).
                                          Otherwise P = O + t Dc on the PIXEL-CENTRE ray (pixelToRay at +0.5, +0.5, not sample 0's
                                          jittered ray: under a resting camera P lands on p's own centre), d = P - o',
                                          den = dot3(nrm', d), mu = dot3(nrm', c0') / den; no history unless mu > 0 (false for NaN).
                                          r = mu d - c0', xn = dot3(cross3(r, cy'), nrm') / dot3(nrm', nrm'),
                                          yn = dot3(cross3(cx', r), nrm') / dot3(nrm', nrm'), fx = (xn + 1) 0.5 W - 0.5,
                                          fy = (yn + 1) 0.5 H - 0.5, te = sqrtf(dot3(d, d)).  Taps q = (x0, y0), (x0+1, y0),
                                          (x0, y0+1), (x0+1, y0+1) with x0 = floorf(fx), a = fx - x0 and the bilinear weights
                                          (1-a or a) * (1-b or b).  A tap counts if it lies inside the frame (a tap outside is
                                          skipped, never clamped), id'(q) == id or both ids >= 0 and
                                          dot3(nhat[id], nhat[id'(q)]) >= normal_cos_min, and fabsf(te - t'(q)) <= depth_rel * te.
                                          Over the counting taps in tap order: sw += w, sc += w h(q) per channel, sn += w n(q).
                                          Not sw > 0, or fx / fy not finite: out = c_now, n' = 1 (fresh).  Else hist = sc / sw,
                                          n' = fminf(sn / sw + 1, (float)max_history), out = hist + (c_now - hist) / n' per channel
                                          (reused) — and c_now itself when n' == 1: max_history = 1 is the plain frame byte for
                                          byte.  Frame 0: every hit pixel is fresh.  Alpha is c_now's.  tests/reproject_ref.c pins
                                          the operation order.
                                       5. color_f32 = out, the rgba8 plane its conversion as the resolve's; the history stores out, n',
                                          id, t and this frame's camera.  With RWR_FLAG_DENOISE the filter runs after this stage, on
                                          out; the history never sees the filter.
                                       6. The history is the context's, not a frame slot's: the stages run in frame order behind an
                                          event while tracing overlaps across frames in flight; every number of frames in flight
                                          gives the same bytes.
                                       7. RWR_ERR_UNSUPPORTED: together with RWR_FLAG_ACCUMULATE (two histories); rwr_render_rows /
                                          rwr_render_strips that do not cover the whole frame (taps reach into other ranks' rows);
                                          RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH, single-triangle passes.  Everything else keeps its
                                          contract: deeper paths, shadows, sky, mirrors, glass, normal maps, RWR_FLAG_NO_CULL,
                                          instances and parts — the stage only sees their resolved frame.  The scene is static
                                          between setters, so no motion vectors are needed. */
    RWR_FLAG_GLOSSY = 1u << 13,     /* extension: glossy surfaces — a scene part or a sphere marked as glossy (rwr_scene_set_part_gloss,
                                       rwr_scene_set_sphere_gloss) of reflectance R and roughness rho sends on a direction between the
                                       mirror reflection and the diffuse ray the hit would otherwise have sent: brushed metal, a
                                       polished floor, a satin ball.  Independent of RWR_FLAG_MIRRORS and RWR_FLAG_GLASS: each flag
                                       switches its own surfaces on; a glossy surface in a frame without this flag is the diffuse
                                       surface it was.  Without the flag every frame is what it was, byte for byte, with no further
                                       launch or allocation.  With it, at a hit h a path goes on from (h0, or h_k with
                                       k < max_bounces) on a glossy surface, all in f32 with no contraction:
                                       1. Dh = normalize3(D), the oracle's routine; D is the direction of the ray that found h, of any
                                          length (at h0 it is unit already and normalised all the same: one rule for every generation).
                                       2. n is the reference's HitRecord normal: a face's normal flipped towards the ray, a sphere's
                                          outward normal; normal maps never change it.  Rf = reflect_direction(n, Dh): d = dot3(n, Dh),
                                          Rf = Dh - (2 d) n per component.
                                       3. X = bounce_direction(n, pixel, sample, seed, d0), bit for bit the diffuse ray the same hit
                                          would have emitted, with d0 the first dimension of the generation's block (2 for the ray that
                                          leaves h0, 2 + 16 k for the one that leaves h_k); the block's dimensions are read exactly as a
                                          diffuse hit reads them.
                                       4. om = 1.0f - rho; S = om Rf + rho X per component (om*Rf.x + rho*X.x: two products, one sum).
                                          At rho = 1 every component of S equals X's.
                                       5. !(dot3(S, S) > 0.0f) — a vanishing sum, or NaN: S = Rf.
                                       6. The next ray: direction S, not re-normalised; origin P + 1e-4 n, operation for operation the
                                          diffuse, mirror and shadow rays' origin; throughput T * R (T0 = R at a glossy h0).  The local
                                          term of h is unchanged, E(h) or the shadowed E(h): a coated surface, as a mirror.  Primary-stage
                                          sums, sample-0 planes, h0's shadow records and generation 1's ray count do not depend on the
                                          flag; the nearest-hit rule, the clamps, the sky's term at a miss and (R <= 1) the integrator's
                                          range analysis are untouched.
                                       7. max_bounces = 0, or no part of the scene and none of its spheres (indices below the count
                                          rwr_scene_set_spheres gave) is glossy: the flag is ignored — cleared before the frame's kernels
                                          are chosen — and the frame is the frame without it, byte for byte, in the same kernels.
                                       8. RWR_FLAG_ACCUMULATE: this bit (after item 7) is part of the key, and of RWR_FLAG_REPROJECT's
                                          effective flags; every accepted call of the gloss setters changes the scene's generation, a
                                          refused one changes nothing.  rwr_last_gloss_stats counts the rays item 6 emitted.  Every
                                          other flag, instances, parts, frames in flight, row bands, strips and the multi-GPU gather keep
                                          their contracts.  With RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH or single-triangle passes:
                                          RWR_ERR_UNSUPPORTED, whatever max_bounces is and whether or not a surface is glossy. */
    RWR_FLAG_SOFT_SHADOWS = 1u << 14, /* extension: soft shadows — RWR_FLAG_SHADOWS' two lights get a finite angular size
                                       (rwr_shadow_set_params), so that shadow edges become penumbrae: sharp at the contact, wide far
                                       from the occluder.  The radius r of a light is the tangent of the half-angle under which a hit
                                       sees it (0: the point light at infinity; 0.0047: the sun).  Without the flag every frame is what
                                       it was, byte for byte.  With RWR_FLAG_SHADOWS and this flag, the shadow ray of hit h_k (k = 0 for
                                       h0, k for the hit of bounce ray k) keeps its origin P + 1e-4 n, operation for operation; its
                                       direction S is, in f32 with no contraction:
                                       1. L = -normalize3(kLightDir) of the shader that shaded the hit, as without the flag; r is that
                                          light's radius (mesh_light_radius for a face hit, sphere_light_radius for a sphere hit).
                                       2. (a, b): bounce_direction's rejection loop over the unit disk, operation for operation — 8 tries,
                                          ua = 2 u - 1, accepted on ua*ua + ub*ub <= 1.0f, a = b = 0 when all eight are refused — on the
                                          RNG dimensions d_s + 2 j, d_s + 1 + 2 j of (global pixel, global sample, seed), with
                                          d_s = 2 + 16 RWR_MAX_BOUNCES + 16 k = 130 + 16 k.  The block lies behind every block a path
                                          reads: no primary, bounce or glass random number changes.
                                       3. b1, b2: bounce_direction's basis about L — sign = copysignf(1, L.z), aa = -1 / (sign + L.z),
                                          bb = L.x L.y aa, b1 = (1 + sign L.x L.x aa, sign bb, -sign L.x), b2 = (bb, sign + L.y L.y aa,
                                          -L.y) — constant per light, the bits of this f32 evaluation.
                                       4. S.c = L.c + r * (a*b1.c + b*b2.c) per component: two products and a sum inside, one product, one
                                          sum.  S is not re-normalised (|S| >= 1; the hit tests take a direction of any length).  With
                                          r = 0 it is L exactly.
                                       5. occluded(h) is "any sphere or any face is hit by (origin, S)" in the reference's intersection
                                          arithmetic: no distance limit, no face excluded.  E(h) is still shaded with the fixed L — only
                                          visibility becomes stochastic; the ambient part, the clamps, the records and the counts of
                                          rwr_last_shadow_stats are RWR_FLAG_SHADOWS', and a soft frame traces as many shadow rays as the
                                          hard one.
                                       6. Without RWR_FLAG_SHADOWS, or with both radii 0, the flag is ignored — cleared before the frame's
                                          kernels are chosen — and the frame is the frame without it, byte for byte, in the same kernels
                                          (the flag alone at spp 1 without a bounce: the reference frame).
                                       7. While the flag is effective, its bit and the 8 bytes of rwr_shadow_params are part of
                                          RWR_FLAG_ACCUMULATE's key and of RWR_FLAG_REPROJECT's; without it rwr_shadow_set_params
                                          disturbs neither.  A reprojecting frame k is traced with seed + k, so its penumbra is drawn
                                          anew.  RNG keys are global pixel and global sample: frames in flight, row bands, strips, the
                                          multi-GPU gather and every schedule give the same bytes; every other flag keeps its contract.
                                          With RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH or single-triangle passes: RWR_ERR_UNSUPPORTED. */
    RWR_FLAG_EMISSIVE = 1u << 15,   /* extension: emissive surfaces — a scene part or a sphere that gives off light of radiance Le
                                       (rwr_scene_set_part_emission, rwr_scene_set_sphere_emission), so that a scene can hold its own
                                       lamps.  Emission is an attribute beside the surface model, not a model: a diffuse, mirror, glass
                                       or glossy surface may also emit, and the setters of one never touch the other.  Without the flag
                                       every frame is what it was, byte for byte.
                                       1. With the flag and at least one emitting surface in the scene, the local shading of every hit h
                                          the integrator shades — h0 and the hit of every bounce ray — becomes E'(h) = E(h) + Le(h): per
                                          channel one f32 add to the value the shader produced (after the normal map, where that is on).
                                          With RWR_FLAG_SHADOWS an occluded hit's shading is ambient(h) + Le(h): a surface's own light is
                                          never shadowed.  Term k is then, as without the flag, T(k-1) * E'(h_k) with T(-1) = 1,
                                          converted and capped as ever — [0, 16] at h0, [0, 64] later, NaN as 0: the sum first, then the
                                          product with T, then the conversion, no contraction.  Le goes inside the clamps, so the range of
                                          every fixed-point sum is what it was.
                                       2. Both sides of a face emit; a sphere emits inwards as well as outwards.
                                       3. Nothing else moves.  Primary, bounce and shadow rays, throughputs, RNG dimensions, the
                                          nearest-hit rule, rwr_last_render_stats, rwr_last_shadow_stats, rwr_last_glass_stats,
                                          rwr_last_gloss_stats, rwr_last_traversal_plan and the depth, id and t planes are those of the
                                          frame without the flag, bit for bit.  A shadow record carries fix(T (E + Le)) - fix(T (amb + Le)).
                                       4. A frame with the flag and an emitter always takes the integrator, also at spp 1 and
                                          max_bounces 0, as with RWR_FLAG_SHADOWS; samples are placed as without the flag.  Unlike the
                                          surface flags it is not cleared at max_bounces 0: an emitter shows at h0.
                                       5. No part of the scene and none of its spheres (indices below the count rwr_scene_set_spheres
                                          gave) emits: the flag is ignored — cleared before the frame's kernels are chosen — and the frame
                                          is the frame without it, byte for byte, in the same kernels (the flag alone at spp 1 without a
                                          bounce: the reference frame).
                                       6. The bit (after item 5) is part of RWR_FLAG_ACCUMULATE's key and of RWR_FLAG_REPROJECT's
                                          effective flags; every accepted call of the emission setters changes the scene's generation, a
                                          refused one changes nothing.  rwr_last_emission_stats counts the shaded hits with Le != 0.
                                       7. Accumulation, frames in flight, row bands, strips and the multi-GPU gather keep their
                                          contracts; RWR_FLAG_DENOISE and RWR_FLAG_REPROJECT are stages behind the resolve and do not know.
                                       8. With RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH or single-triangle passes: RWR_ERR_UNSUPPORTED,
                                          whatever the scene holds.
                                       A ray is aimed at an emitting sphere only under RWR_FLAG_LIGHT_SAMPLING and at an emitting part
                                       only under RWR_FLAG_LIGHT_PARTS; without them a lamp is found by chance, and its light is noisy
                                       at low sample counts. */
    RWR_FLAG_LIGHT_SAMPLING = 1u << 16, /* extension: light sampling (next-event estimation) towards emitting SPHERES — every diffuse hit
                                       that sends a ray on also sends one ray towards an emitting sphere, so that a small lamp lights a
                                       room at few samples.  Emitting mesh parts are RWR_FLAG_LIGHT_PARTS' (an area distribution over
                                       their faces): under this flag alone they are found by chance as before and their Le is never
                                       suppressed.  The light sample stands alone unless RWR_FLAG_LIGHT_MIS combines it with the bounce ray (multiple importance
                                       sampling), and mirror, glass and glossy hits send no light ray.  Without
                                       the flag every frame is what it was, byte for byte.  All arithmetic f32, no contraction.
                                       1. The flag is effective only while RWR_FLAG_EMISSIVE is effective, max_bounces >= 1 and at
                                          least one sphere in use (index below the count rwr_scene_set_spheres gave) emits; otherwise it
                                          is cleared before the frame's kernels are chosen and the frame is the frame without it, in the
                                          same kernels.  s_0 < ... < s_{M-1}: the indices of the emitting spheres in use.
                                       2. A hit h_k (k = 0 ... max_bounces - 1) is eligible when its surface's model, as the frame sees
                                          it, is diffuse, so that ray k + 1 is the cosine-distributed bounce ray (a "diffuse ray"; its
                                          queue record carries a mark).  Mirror, glass and glossy hits — roughness 1 included — are not.
                                       3. The light sample of an eligible hit.  O: the origin of ray k + 1 (P + 1e-4 n); T: its
                                          throughput as the queue holds it (after the unorm16 rounding); n: the hit record's normal.
                                          RNG block d = 274 + 17 k on (global pixel, global sample, seed), behind soft shadows' last
                                          dimension (273): no existing random number moves.
                                          u = rng(d); i = min((uint32)(u * (float)M), M - 1); s = s_i, centre C, radius R.
                                          w = C - O; d2 = dot3(w, w); !(d2 > R*R): no sample.  dl = sqrtf(d2); w = w / dl per component.
                                          s2 = R*R / d2; cmax = sqrtf(fmaxf(0, 1 - s2)); kc = s2 / (1 + cmax)   (1 - cmax, no cancellation).
                                          (a, b): the bounce direction's rejection loop over the unit disk, 8 tries on dimensions
                                          d + 1 + 2j, d + 2 + 2j; a = b = 0 when all are refused.
                                          q = a*a + b*b; c = 1 - q*kc; r = q > 0 ? sqrtf(fmaxf(0, 1 - c*c) / q) : 0; (b1, b2): the
                                          bounce direction's basis about w; omega = r*(a*b1 + b*b2) + c*w per component, not
                                          re-normalised: uniform over the solid angle the sphere subtends.
                                          ndw = dot3(n, omega); !(ndw > 0): no ray is traced.
                                          The ray (O, omega) REACHES s when the nearest hit along it under the integrator's own rule —
                                          spheres in order, strict '<', then the mesh if closer — is sphere s: the sample counts exactly
                                          when a bounce ray in that direction would have found the lamp; a ray that rounding lets graze
                                          past the rim does not reach it.
                                          g = 2 * (float)M * kc * ndw; per channel the term is T.c * (Le_s.c * g), converted and capped
                                          to [0, 64] like a bounce term (NaN as 0) and added to the same fixed-point sums.
                                       4. No double counting: a diffuse ray from origin O that hits an emitting sphere s in use with
                                          dot3(C - O, C - O) > R*R takes Le(hit) as 0 everywhere in RWR_FLAG_EMISSIVE's rule — shading,
                                          ambient part, rwr_last_emission_stats.  Every other hit keeps Le: h0, the hits of mirror, glass
                                          and glossy rays, hits from inside the sphere, emitting parts (those until RWR_FLAG_LIGHT_PARTS' item 8 silences them).
                                       5. Everything else is the frame's with RWR_FLAG_EMISSIVE alone, bit for bit: primary, bounce and
                                          shadow rays, throughputs, existing RNG dimensions, rwr_last_render_stats, the shadow, glass and
                                          gloss stats, rwr_last_traversal_plan, the depth, id and t planes.  The light ray needs no
                                          RWR_FLAG_SHADOWS and does not know it.  A path adds up to 1 + 2 max_bounces terms: 17 terms
                                          below 2^32 at 2^24 accumulated samples stay below 2^61 in the 64-bit sums.
                                       6. The bit (after item 1) is part of RWR_FLAG_ACCUMULATE's key and of RWR_FLAG_REPROJECT's
                                          effective flags; the emitting spheres are part of the scene's generation.
                                          rwr_last_light_stats counts the rays traced, those that reached, and the hits item 4 silenced.
                                          RNG keys are global pixel and global sample: frames in flight, row bands, strips, the multi-GPU
                                          gather, accumulation and every schedule give the same bytes.
                                       7. With RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH or single-triangle passes: RWR_ERR_UNSUPPORTED. */
    /* bits 17-20 are reserved: the library's internal flags (RWR_FLAGS_RESERVED below) */
    RWR_FLAG_LIGHT_PARTS = 1u << 21,   /* extension: light sampling towards emitting mesh PARTS — the light sample of an eligible hit may
                                       aim at a point of a face of an emitting part (the "mesh light"), so that a room lit by a ceiling
                                       panel converges at few samples.  Independent of RWR_FLAG_LIGHT_SAMPLING: either, both or neither.
                                       Without this flag every frame is what it was, byte for byte — frames with RWR_FLAG_LIGHT_SAMPLING
                                       and emitting parts included.  Multiple importance sampling is RWR_FLAG_LIGHT_MIS'; emitters emit from both
                                       sides; mirror, glass and glossy hits send no light ray.  All arithmetic f32, no contraction,
                                       except the host table of item 2.
                                       1. The mesh light is the list of the world faces (after instancing) whose part emits and whose
                                          area is greater than 0, in face-index order.  It changes with the scene and the part emission
                                          setter, so it is part of the scene's generation.
                                       2. The host table, one 16-byte record {float cdf; uint32 face; float inv_pdf; uint32 pad} per
                                          listed face; all sums in double, rounded to f32 once, on storing.  A_f = 0.5 |(p1 - p0) x
                                          (p2 - p0)| from the world-space vertices; w_f = A_f (Le_r + Le_g + Le_b) of the face's part;
                                          W the running sum of the w_f in list order; cdf_f that running sum over W, the last entry
                                          forced to 1.0f; inv_pdf_f = W / (Le_r + Le_g + Le_b): the reciprocal of the area density of a
                                          point of the face (choice w_f / W times 1 / A_f).
                                       3. The flag is effective only while RWR_FLAG_EMISSIVE is effective, max_bounces >= 1 and the list
                                          is not empty; otherwise it is cleared before the frame's kernels are chosen and the frame is
                                          the frame without it.  RWR_FLAG_LIGHT_SAMPLING keeps its own item 1.  M: the emitting spheres
                                          in use when that flag is effective, else 0; Q: 1 when this flag is effective, else 0; L = M + Q.
                                       4. Eligible hits, O, T, n and the RNG block d = 274 + 17 k are RWR_FLAG_LIGHT_SAMPLING's items 2
                                          and 3, unchanged: one light ray per eligible hit, no random number moves and none is added.
                                       5. Choosing the light: u = rng(d); i = min((uint32)(u * (float)L), L - 1) (with L = 1, i = 0 and
                                          no random number picks).  i < M: sphere s_i by RWR_FLAG_LIGHT_SAMPLING's item 3, with M
                                          replaced by L in g.  i == M: the mesh light, item 6.
                                       6. The face sample.  uf = rng(d + 1); the face f is that of the first list entry j with
                                          uf < cdf_j (binary search).  u1 = rng(d + 2), u2 = rng(d + 3); if u1 + u2 > 1 then u1 = 1 - u1,
                                          u2 = 1 - u2.  P = (p0 + u1*(p1 - p0)) + u2*(p2 - p0) per component, from the face's world-space
                                          vertices as the kernels hold them.  v = P - O; d2 = dot3(v, v); !(d2 > 0): no sample.
                                          dl = sqrtf(d2); omega = v / dl per component.  ndw = dot3(n, omega); !(ndw > 0): no ray is traced.
                                          N_f = normalize(cross(p1 - p0, p2 - p0)), the face's unit normal as the kernels hold it (v / sqrtf(
                                          dot3(v, v)) per component); cf = fabsf(dot3(N_f, omega)): both sides emit.
                                          g = (((((float)L * inv_pdf_f) * ndw) * cf) * 0.318309886f) / d2, in that order; per channel the
                                          term is T.c * (Le.c * g), Le the radiance of f's part, converted and capped to [0, 64] like a
                                          bounce term (NaN as 0) and added to the same fixed-point sums.  A path adds no more terms than
                                          under RWR_FLAG_LIGHT_SAMPLING.
                                       7. The ray (O, omega) REACHES f when the nearest hit along it under the integrator's own rule —
                                          spheres in order, strict '<', then the mesh if closer, the lowest face index winning ties — is
                                          face f: the ray hits f at t_f, no sphere at t <= t_f, no face g at t_g < t_f or at t_g == t_f
                                          with g < f.  A sample whose ray rounding lets miss f does not reach.
                                       8. No double counting: a diffuse ray (marked, item 4) whose hit is a face of an emitting part
                                          takes Le(hit) as 0 everywhere in RWR_FLAG_EMISSIVE's rule — shading, ambient part,
                                          rwr_last_emission_stats — while this flag is effective, and is counted as suppressed.  h0 and
                                          the hits of mirror, glass and glossy rays keep Le; so does an emitting sphere unless
                                          RWR_FLAG_LIGHT_SAMPLING's item 4 silences it.
                                       9. Everything else as RWR_FLAG_LIGHT_SAMPLING's items 5 and 6: the bit (after item 3) is part of
                                          RWR_FLAG_ACCUMULATE's key and of RWR_FLAG_REPROJECT's effective flags; rwr_last_light_stats
                                          counts the light stage's totals, rwr_last_part_light_stats the mesh light's share of each.
                                       10. With RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH or single-triangle passes: RWR_ERR_UNSUPPORTED. */
    RWR_FLAG_LIGHT_MIS = 1u << 22,     /* extension: multiple importance sampling (balance heuristic, Veach 1995) of the light ray and
                                       the diffuse bounce ray.  Under the two flags above the light sample stands alone and the bounce
                                       ray that finds the same emitter is silenced; under this flag both count, each weighted by its
                                       share of the two densities, so that every light term is bounded by T * Le, the cap no longer
                                       darkens receivers that touch an emitter, and both flags may stay on in any scene.  Without this
                                       flag every frame is what it was, byte for byte.  All arithmetic f32, no contraction.
                                       1. The flag is effective only while RWR_FLAG_LIGHT_SAMPLING, RWR_FLAG_LIGHT_PARTS or (its items 5
                                          and 6 say what is weighted there) RWR_FLAG_LIGHT_SKY is effective,
                                          each by its own rule; otherwise it is cleared before the frame's kernels are chosen and the
                                          frame is the frame without it, in the same kernels.  L: the lights the stage chooses among
                                          (RWR_FLAG_LIGHT_PARTS' item 3; M under RWR_FLAG_LIGHT_SAMPLING alone).
                                       2. No ray changes.  Eligible hits, the choice of the light, the sample's direction, the reach
                                          tests, RNG dimensions, bounce rays and throughputs, rwr_last_render_stats, the shadow, glass
                                          and gloss stats, rwr_last_traversal_plan, the depth, id and t planes and all six counts of
                                          rwr_last_light_stats and rwr_last_part_light_stats are those of the frame without the flag,
                                          bit for bit.  Only the values of items 4 and 5 change.
                                       3. The weight.  The diffuse bounce ray has density p_b = (n . omega) / pi; the g of
                                          RWR_FLAG_LIGHT_SAMPLING's item 3 and of RWR_FLAG_LIGHT_PARTS' item 6 is exactly p_b / p_l, p_l
                                          the light sampler's density of omega with the 1 / L choice.  One function serves both sides:
                                          m(g) = p_b / (p_b + p_l) = g / (1 + g), evaluated as
                                            m(g) = g > 0 ? 1.0f / (1.0f + 1.0f / g) : 0.0f
                                          two f32 divisions and one add: 0 for g <= 0 and for NaN, 0 for a g so small that 1 / g is
                                          infinite, exactly 1 for g = infinity (d2 -> 0), with no special case.
                                       4. The light term of a sample that reaches becomes T.c * (Le.c * m(g)) per channel, g computed as
                                          under the two flags; converted and capped as before, but m <= 1, T <= 1 and Le <= 64 keep it
                                          from ever reaching the cap.
                                       5. The bounce side.  The hit of a diffuse (marked) ray that RWR_FLAG_LIGHT_SAMPLING's item 4 or
                                          RWR_FLAG_LIGHT_PARTS' item 8 silences takes Le.c * m(g') per channel in place of 0, everywhere
                                          in RWR_FLAG_EMISSIVE's rule: shading, the ambient part, and the hit's count in
                                          rwr_last_emission_stats when a weighted channel is not zero.  g' is g for the direction the ray
                                          did take.  O: the ray's origin; D: its direction as its queue record holds it; n: the normal
                                          of the hit that sent it (item 3 of RWR_FLAG_LIGHT_SAMPLING); t: the hit's distance.
                                          nd = dot3(n, D).
                                          Sphere s (centre C, radius R): w = C - O; d2 = dot3(w, w) (> R*R, or the hit is not silenced);
                                          s2 = R*R / d2; cmax = sqrtf(fmaxf(0, 1 - s2)); kc = s2 / (1 + cmax);
                                          g' = ((2 * (float)L) * kc) * nd.
                                          Face f: N_f its unit normal as the kernels hold it; cf = fabsf(dot3(N_f, D)); d2 = t * t;
                                          inv_pdf that of f's part (every listed face of a part stores the same f32, item 2 of
                                          RWR_FLAG_LIGHT_PARTS); g' = (((((float)L * inv_pdf) * nd) * cf) * 0.318309886f) / d2.
                                          These hits still count in suppressed_hits (silenced or weighted).  Every hit the two flags
                                          leave its Le keeps all of it: h0, the hits of mirror, glass and glossy rays, a sphere hit from
                                          inside (!(d2 > R*R)), a sphere while only RWR_FLAG_LIGHT_PARTS is effective, a face while only
                                          RWR_FLAG_LIGHT_SAMPLING is.  (A face whose cdf interval is empty in f32 is never drawn; its
                                          bounce hits are weighted as if it were: the f32 limit RWR_FLAG_LIGHT_PARTS documents.)
                                       6. The sum is the same integral: at every direction omega towards an emitter the light sample
                                          contributes with weight p_l / (p_l + p_b) = 1 - m and the bounce ray with p_b / (p_l + p_b) = m.
                                          The balance heuristic only; no power heuristic, no power-proportional light choice, no light
                                          rays from glossy hits, no weighting of the gradient sky (the sky's image: RWR_FLAG_LIGHT_SKY).
                                       7. The bit (after item 1) is part of RWR_FLAG_ACCUMULATE's key and of RWR_FLAG_REPROJECT's
                                          effective flags.  With RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH or single-triangle passes:
                                          RWR_ERR_UNSUPPORTED. */
    RWR_FLAG_SOBOL = 1u << 23,         /* extension: an Owen-scrambled Sobol sample sequence (Burley 2020, "Practical Hash-based Owen
                                       Scrambling") in place of the independent hash.  Every random number the integrator draws — the
                                       pixel jitter, the disk points of the bounce rays, the glass and gloss choices, the soft-shadow
                                       disk points, the light stage's numbers — is (h >> 8) * 2^-24 of a 32-bit word h; without the
                                       flag h = rng_hash(pixel, sample, dim, seed), with it h = rng_sobol(pixel, sample, dim, seed).
                                       Dimension numbers, the order of draws, the conversion and everything downstream stay; only the
                                       word changes.  A pixel's samples are then stratified against each other and the error falls
                                       faster than 1 / spp.  Off by default; without the flag every frame is what it was, byte for byte.
                                       1. The word.  u32 wrapping arithmetic only; rev(x): the 32 bits of x reversed; rng_mix:
                                          rng_hash's mixer (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16).
                                            lk(x, s)   : x += s; x ^= x * 0x6c50b47c; x ^= x * 0xb82f1e52; x ^= x * 0xc7afe638;
                                                         x ^= x * 0x8d22f6e6
                                            owen(x, s) = rev(lk(rev(x), s))
                                            sobol1(i)  : r = 0; v = 1u << 31; while (i) { if (i & 1) r ^= v; i >>= 1; v ^= v >> 1; } -> r
                                            h0  = rng_mix((seed ^ 0x9E3779B9) ^ pixel)
                                            s   = rng_mix(h0 ^ ((dim >> 1) * 0xC2B2AE35))
                                            idx = owen(sample, s)
                                            x   = (dim & 1) ? sobol1(idx) : rev(idx)
                                            rng_sobol = owen(x, rng_mix(s ^ (0x85EBCA6B + (dim & 1))))
                                          pixel = y * width + x of the whole frame, sample the GLOBAL sample index (an accumulation's
                                          base included), as for rng_hash: K accumulated frames of s samples are one frame of K * s.
                                       2. Dimensions 2g and 2g + 1 are the two coordinates of one scrambled, shuffled (0,2)-sequence
                                          with a stream of its own per pixel, seed and g: the jitter pair, every disk try of a bounce
                                          ray and every soft-shadow point are such pairs.  The light stage's disk pairs start at an
                                          odd dimension behind generations 1, 3, 5, 7: those are stratified per coordinate only.
                                       3. The flag is effective only in a frame the wavefront integrator renders (several samples, a
                                          bounce, an accumulation, shadow rays, a stage behind the resolve, an emitter); it sends no
                                          frame there.  Otherwise it is cleared and the frame is the frame without it.
                                       4. Rays, counts and planes follow from the numbers: every rwr_last_*_stats count is that of the
                                          CPU reference drawing the same words.  Bands, strips, the gather, frames in flight,
                                          accumulation and every schedule give the same bytes.
                                       5. The bit (after item 3) is part of RWR_FLAG_ACCUMULATE's key and of RWR_FLAG_REPROJECT's
                                          effective flags.  With RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH or single-triangle passes:
                                          RWR_ERR_UNSUPPORTED. */
    RWR_FLAG_SKY_IMAGE = 1u << 24,     /* extension: sky light from an image — RWR_FLAG_SKY's radiance S(D) comes from an octahedral
                                       environment map (rwr_sky_set_image) instead of the two-colour gradient.  The flag implies
                                       nothing.  Off by default; without the flag every frame is what it was, byte for byte.
                                       1. With the flag in effect the S(D) of RWR_FLAG_SKY item 1 is S_img(D), f32 operations in
                                          exactly this order, no contraction, `/` the IEEE division:
                                            a  = (|D.x| + |D.y|) + |D.z|
                                            px = D.x / a;  pz = D.z / a
                                            if (D.y < 0) { qx = (1 - |pz|) * copysignf(1, px);  qz = (1 - |px|) * copysignf(1, pz);
                                                           px = qx;  pz = qz; }
                                            u  = px * 0.5 + 0.5;  v = pz * 0.5 + 0.5
                                            S_img = the bilinear fetch of the mesh textures (four taps, ClampToEdge, the blend
                                                    fma(t11, w11, fma(t01, w01, fma(t10, w10, t00 * w00))) per channel) of the
                                                    n x n image at texel-space position (u * n - 0.5, v * n - 0.5)
                                          Column i of the image is u, row j is v.  The upper hemisphere (+y, the reference's
                                          Camera.up) is the inner diamond |2u - 1| + |2v - 1| <= 1 with the zenith at the map's
                                          centre; the lower hemisphere is folded into the four corners, the nadir at all four.
                                       2. RWR_FLAG_SKY's items 2-7 hold as written: bounce rays only, the term is
                                          clamp(T * S_img(D), 0, 64), NaN counts as 0, primary misses are unchanged.  No random
                                          number is used and no ray or count changes: every rwr_last_*_stats count is that of the
                                          frame under the gradient.
                                       3. ClampToEdge at the map's outer border is not the octahedral wrap: within half a texel of
                                          the border — directions below the horizon only, and at most half a texel off — the fetch
                                          repeats the border texel where the true wrap would blend with the texel mirrored across
                                          the border's midpoint.  No mip levels: a map much finer than a glossy lobe is noisy.
                                       4. The flag is effective only while RWR_FLAG_SKY is in effect (max_bounces >= 1) and the
                                          context holds an image.  Otherwise it is cleared and the frame is the frame without it,
                                          byte for byte, in the same kernels.
                                       5. While the bit is effective, the image's generation (rwr_sky_get_image_info) is part of
                                          RWR_FLAG_ACCUMULATE's key and of RWR_FLAG_REPROJECT's, next to rwr_sky_params, which stay
                                          in both: a new image starts a new history.  Without the bit, rwr_sky_set_image disturbs
                                          neither.  With RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH or single-triangle passes:
                                          RWR_ERR_UNSUPPORTED. */
    RWR_FLAG_LIGHT_SKY = 1u << 25,     /* extension: light rays aimed at the sky's image — the light ray of an eligible (diffuse) hit may
                                       aim at RWR_FLAG_SKY_IMAGE's map, drawn in proportion to the map's radiance, so that a map with
                                       a small sun converges.  The flag implies nothing.  Off by default; without the flag every frame
                                       is what it was, byte for byte.  All arithmetic f32, no contraction, unless it says double.
                                       1. The distribution, made on the host once per image (by the first frame that asks for the flag
                                          after rwr_sky_set_image; rwr_sky_get_light_info).  All sums in double, rounded to f32 once, on
                                          storing.  For texel (row j, column i): lum = r + g + b; b_ji = the sum of lum over the 3 x 3
                                          neighbourhood, indices clamped to [0, n - 1], rows outer, columns inner (S_img's bilinear
                                          fetch reads exactly those texels from inside the cell: the density is positive wherever
                                          S_img is); p_c = the point of |x| + |y| + |z| = 1 at the cell's centre, u = (i + 0.5) / n,
                                          v = (j + 0.5) / n: px = 2u - 1, pz = 2v - 1, py = (1 - |px|) - |pz|, and where py < 0
                                          (px, pz) <- ((1 - |pz|) copysign(1, px), (1 - |px|) copysign(1, pz)); l2 = (px px + py py) + pz pz;
                                          w_ji = b_ji * (1 / (l2 * sqrt(l2))) — the cell du dv covers the solid angle 4 a^3 du dv, a the
                                          L1 norm of the unit direction, a = 1 / |p|.  W_j = sum_i w_ji, W = sum_j W_j, in index order.
                                          R_j = (float)((W_0 + ... + W_j) / W), C_ji = (float)((w_j0 + ... + w_ji) / W_j); in each cdf every
                                          entry from the last texel (row) of non-zero weight on is 1.0f; a row with W_j = 0 holds 1.0f
                                          throughout.  The cdf before index 0 is 0.
                                       2. Eligible hits, O, T, n and the RNG block d = 274 + 17 k are RWR_FLAG_LIGHT_SAMPLING's: one light
                                          ray per eligible hit, no random number moves, no dimension is added.  With M the emitting
                                          spheres in use while RWR_FLAG_LIGHT_SAMPLING is effective (else 0) and P = 1 while
                                          RWR_FLAG_LIGHT_PARTS is (else 0) there are L = M + P + 1 lights, the sky the last:
                                          i = min((uint32)(rng(d) * (float)L), L - 1), drawn only when L > 1.  i < M is the sphere rule,
                                          i == M with P = 1 the face rule, both with this L in their g; i == L - 1 is the sky lane.
                                       3. The sky lane's draw.  Row j: the first entry with rng(d + 1) < R_j; column i: the first with
                                          rng(d + 2) < C_ji (binary searches).  u = ((float)i + rng(d + 3)) / (float)n,
                                          v = ((float)j + rng(d + 4)) / (float)n; px = 2u - 1, pz = 2v - 1, py = (1 - |px|) - |pz|, folded
                                          as in item 1 where py < 0; len = sqrtf((px px + py py) + pz pz); omega = p / len per component.
                                       4. The factor, one function for both sides: sky_light_g(omega, ndw = dot3(n, omega), L).  omega is
                                          mapped forward with RWR_FLAG_SKY_IMAGE's item 1, giving a, u, v; the texel is
                                          i' = min((uint32)(u * (float)n), n - 1), j' likewise with v;
                                          P = (R_j' - R_(j'-1)) * (C_j'i' - C_j'(i'-1));
                                          g = ((((float)L * ndw) * 0.318309886f) * (4 * ((a * a) * a))) / (((float)n * (float)n) * P),
                                          which is p_b / p_l as in the other two rules.  !(P > 0) or !(ndw > 0): no sample, no ray.
                                          The light side calls it on the omega it drew: a bounce ray in that direction computes the
                                          same float.
                                       5. The ray (O, omega) REACHES the sky when it hits nothing — no sphere at any t, no face: the
                                          predicate by which a bounce ray counts as a miss.  The term is T.c * (S_img(omega).c * g) per
                                          channel, m(g) in g's place under RWR_FLAG_LIGHT_MIS, converted and capped to [0, 64] like a
                                          bounce term (NaN as 0) and added to the same sums.  A path adds no more terms than under
                                          RWR_FLAG_LIGHT_SAMPLING.
                                       6. No double counting: while the flag is effective a diffuse (marked) ray that leaves the scene
                                          adds no sky term; under RWR_FLAG_LIGHT_MIS it adds T.c * (S_img(D).c * m(g')) instead,
                                          g' = sky_light_g(D, dot3(n, D), L), n the normal of the hit that sent the ray, and where
                                          !(P > 0) — the sampler cannot go there — all of T.c * S_img(D).c.  Such misses, silenced or
                                          weighted, count as suppressed.  The misses of mirror, glass and glossy rays keep S.
                                       7. The flag is effective while RWR_FLAG_SKY_IMAGE is effective and W > 0; otherwise it is cleared
                                          and the frame is the frame without it, byte for byte, in the same kernels.  It does not need
                                          RWR_FLAG_EMISSIVE.  RWR_FLAG_LIGHT_MIS is effective while any of the three light flags is.
                                          The gradient sky gets no light rays: cosine-distributed bounce rays suit it.
                                       8. rwr_last_light_stats' three totals include the sky's rays, reached rays and suppressed misses;
                                          rwr_last_sky_light_stats reports the sky's share of each.
                                       9. The bit (after item 7) is part of RWR_FLAG_ACCUMULATE's key and of RWR_FLAG_REPROJECT's
                                          effective flags; the image's generation is in both already.  With RWR_FLAG_ORTHO_RAYS,
                                          RWR_FLAG_USE_BVH or single-triangle passes: RWR_ERR_UNSUPPORTED. */
    RWR_FLAG_TONEMAP = 1u << 26        /* extension: tone mapping and exposure — the frame's rgba8 plane becomes curve(E * colour) instead
                                       of the mean saturated at 1.0, so that a lamp, the sun of a sky image and the wall beside the
                                       lamp keep apart.  The third stage behind the resolve, after RWR_FLAG_REPROJECT's and
                                       RWR_FLAG_DENOISE's; parameters: rwr_tonemap_set_params.  Off by default; without the flag every
                                       frame is what it was, byte for byte.  All arithmetic f32, in exactly this order, no contraction,
                                       IEEE division.
                                       1. The frame path.  A frame with the flag always takes the path integrator and is rendered as if
                                          RWR_FLAG_AUX_OUTPUTS were set, like RWR_FLAG_DENOISE.  The stage runs last on the frame's
                                          stream: after either resolve, after the reprojection stage and after the filter.  Its bit is
                                          part neither of the effective flags nor of RWR_FLAG_ACCUMULATE's or RWR_FLAG_REPROJECT's key,
                                          and neither are its parameters: changing them between accumulating or reprojecting frames
                                          restarts nothing.  The histories never see the stage.
                                       2. The depth, id, t and color_f32 planes, every count and every history are those of the frame
                                          without the flag, bit for bit: color_f32 stays the linear radiance.
                                       3. The measure, only with auto_exposure.  A pixel counts when its alpha in color_f32 is not 0.
                                          For each counted pixel Y = (0.2126f r + 0.7152f g) + 0.0722f b,
                                          Yc = fminf(fmaxf(Y, 2^-16), 2^16) (a NaN Y gives 2^-16) and L = (int32)bits(Yc) - 0x3f800000:
                                          the piecewise-linear log2 in units of 2^-23, an exact integer.  log_sum is the sum of L as
                                          int64, count the number of counted pixels: the same bits in any order.
                                       4. The exposure.  M = floor(log_sum / count) — floor division, not C's truncation —,
                                          G = float_from_bits(0x3f800000 + M) and E = (key / G) * exposure.  With count == 0, or
                                          without auto_exposure, E = exposure.
                                       5. The map.  For every pixel and each of r, g, b: x = c * E, then
                                          RWR_TONEMAP_CLAMP     y = x
                                          RWR_TONEMAP_REINHARD  y = (x * (1.0f + x * iw2)) / (1.0f + x), iw2 = 1.0f / (white * white),
                                                                computed once on the host
                                          RWR_TONEMAP_ACES      y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f)
                                                                (Narkowicz's fit)
                                          and the byte is the rgba8 store's rule on y: times 255, saturated to [0, 255], nearest, ties
                                          to even, NaN gives 0.  The alpha byte is the one the resolve wrote.  Background pixels are 0
                                          under every curve.  There is no sRGB transfer function in the stage.
                                       6. rwr_render_rows and rwr_render_strips with a part of the frame: RWR_ERR_UNSUPPORTED (the measure
                                          is over the whole frame).  With RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH or single-triangle
                                          passes: RWR_ERR_UNSUPPORTED.
                                       7. rwr_last_tonemap_stats: log_sum, count and E of the frame rendered last; a manual frame gives
                                          0, 0 and exposure, a frame without the flag 0, 0 and 0. */
};
/* every flag above, and the bits between them that the library keeps for itself: a caller sets none of the latter */
#define RWR_FLAGS_RESERVED (0xfu << 17)
#define RWR_FLAGS_PUBLIC (((1u << 17) - 1u) | (1u << 21) | (1u << 22) | (1u << 23) | (1u << 24) | (1u << 25) | (1u << 26))

#define RWR_MAX_BOUNCES 8u

#define RWR_MAX_SPHERES 8
#define RWR_MAX_TRIANGLES 8

/* Object id plane encoding (aux output): >= 0 mesh face index
 * (instance * n_faces + face), -1 background, -2-k analytic sphere k, -10-k single triangle k. */

typedef struct rwr_context rwr_context;

/* ------------------------------------------------------ context / device -- */

/* Replaces wgpu Instance/Adapter/Device/Queue creation, src/lib.rs:266-303. */
RWR_API int rwr_ctx_create(int device_id, rwr_context **out_ctx);
RWR_API void rwr_ctx_destroy(rwr_context *ctx);
RWR_API const char *rwr_last_error_string(void);
RWR_API int rwr_device_count(int *out_count);
/* Name, CU count and wavefront size of the context's device. */
RWR_API int rwr_ctx_device_info(rwr_context *ctx, char *name, size_t name_cap, int *cu_count, int *wave_size);

/* Frames in flight (1..3, default 1).  With n > 1 the context owns n sets of targets and per-frame
 * buffers, each with its own HIP stream, and consecutive rwr_render calls take them in turn, the way a
 * swapchain hands out images (the reference takes each frame from wgpu's surface and presents it, lib.rs:1013,1227): the
 * next frame's kernels fill the GPU while the previous frame's last waves drain.  rwr_readback and
 * rwr_get_device_targets refer to the frame rendered last (rwr_readback waits for that frame only,
 * rwr_get_device_targets orders the context's stream after it); a frame's
 * targets stay valid until n further frames have been rendered.  rwr_synchronize, scene changes,
 * rwr_resize and rwr_ctx_set_stream wait for all frames in flight.  Slot 0 uses the context's stream
 * (rwr_ctx_set_stream), the others internal streams. */
RWR_API int rwr_ctx_set_frames_in_flight(rwr_context *ctx, uint32_t n);

/* Launch on a caller-owned hipStream_t (e.g. torch's current stream) instead of
 * the context's own stream.  NULL restores the context's stream. */
RWR_API int rwr_ctx_set_stream(rwr_context *ctx, void *hip_stream);
RWR_API void *rwr_ctx_get_stream(rwr_context *ctx);

/* ---------------------------------------------------------------- scene -- */

/* Replaces the storage/uniform/texture bindings TriangleList feeds the mesh pass:
 * vertice_list, face_list, material, texture_diffuse + sampler
 * (src/lib.rs:617-669, triangle_list.rs:212-250, resources.rs:189-203,215-261).
 * `rgba8_srgb` is tex_w*tex_h RGBA8 texels, row 0 = first row of the image
 * file, interpreted as Rgba8UnormSrgb with a ClampToEdge / linear-mag sampler
 * (texture.rs:122,151-159).  n_faces may be 0 (spheres only). */
RWR_API int rwr_scene_upload_mesh(rwr_context *ctx,
                                  const rwr_model_vertex_small *verts, uint32_t n_verts,
                                  const rwr_model_face_small *faces, uint32_t n_faces,
                                  const rwr_material_data *material,
                                  const uint8_t *rgba8_srgb, uint32_t tex_w, uint32_t tex_h);

/* Extension — scenes of several meshes, each with its own material and texture (what
 * resources::load_model_compute returns in Model{meshes, materials}; the reference's TriangleList
 * binds meshes[0]/materials[0] only, triangle_list.rs:212-245).  Faces form one list in part order,
 * then face order, so object ids and the lowest-index tie rule extend across parts.
 * rwr_scene_upload_mesh == clear + add_mesh + commit. */
RWR_API int rwr_scene_clear(rwr_context *ctx);
RWR_API int rwr_scene_add_mesh(rwr_context *ctx,
                               const rwr_model_vertex_small *verts, uint32_t n_verts,
                               const rwr_model_face_small *faces, uint32_t n_faces,
                               const rwr_material_data *material,
                               const uint8_t *rgba8_srgb, uint32_t tex_w, uint32_t tex_h);
RWR_API int rwr_scene_commit(rwr_context *ctx);

/* Extension (RWR_FLAG_NORMAL_MAP): the normal map of scene part `part` (0 for a scene uploaded with
 * rwr_scene_upload_mesh), tex_w*tex_h RGBA8 texels in file order, decoded as LINEAR rgba8unorm (vectors, not
 * colours), same ClampToEdge / bilinear sampler and texture coordinates as the diffuse texture.  Call after the part
 * was added (before or after rwr_scene_commit); NULL removes the map.  Shading: tangent frame of the FACE from its
 * corners and texture coordinates (T = dP/du, B = -dP/dv in sampling space, Gram-Schmidt against the face normal),
 * n' = normalize(T m.x + B m.y + N m.z), m = 2 texel - 1, in place of the flat normal in compute.wgsl:226-229
 * (full definition: oracle/rt_oracle.c normal_mapped). */
RWR_API int rwr_scene_set_normal_map(rwr_context *ctx, uint32_t part, const uint8_t *rgba8_linear, uint32_t tex_w, uint32_t tex_h);
/* Parts (meshes with faces) added to the scene so far. */
RWR_API int rwr_scene_part_count(rwr_context *ctx, uint32_t *n_parts);

/* RWR_FLAG_MIRRORS: the mirror attribute of a scene part (part < rwr_scene_part_count) or of a sphere index (sphere <
 * RWR_MAX_SPHERES; kept per index, whatever rwr_scene_set_spheres holds or sets later).  reflectance: 3 floats, each finite and
 * in [0, 1]; NULL = not a mirror (the default).  Anything else, NaN included: RWR_ERR_INVALID_ARGUMENT and the old state stays.
 * Host-side, waits for nothing; frames rendered after the call see the new state.  rwr_scene_clear and with it every
 * rwr_scene_upload_* reset the part attributes (a new upload is a new scene); the sphere attributes persist.  The getters
 * return *is_mirror = 0 / 1 and, for a mirror, its reflectance (zeros otherwise); either output may be NULL. */
RWR_API int rwr_scene_set_part_mirror(rwr_context *ctx, uint32_t part, const float *reflectance);
RWR_API int rwr_scene_set_sphere_mirror(rwr_context *ctx, uint32_t sphere, const float *reflectance);
RWR_API int rwr_scene_get_part_mirror(rwr_context *ctx, uint32_t part, int *is_mirror, float reflectance[3]);
RWR_API int rwr_scene_get_sphere_mirror(rwr_context *ctx, uint32_t sphere, int *is_mirror, float reflectance[3]);

/* RWR_FLAG_GLASS: the glass attribute of a scene part or of a sphere index, with the mirror attribute's index and reset rules.
 * tint: 3 floats, each finite and in [0, 1]; NULL = not glass (ior is then ignored).  ior: finite, in [1, 4].  Anything else, NaN
 * included: RWR_ERR_INVALID_ARGUMENT and the old state stays.  A surface has one model: an accepted call of a glass setter
 * clears the surface's mirror attribute, an accepted call of a mirror setter its glass attribute (with NULL either makes the
 * surface diffuse).  Every accepted call changes the scene's generation.  The getters return *is_glass = 0 / 1 and, for glass,
 * its ior and tint (zeros otherwise); every output may be NULL. */
RWR_API int rwr_scene_set_part_glass(rwr_context *ctx, uint32_t part, float ior, const float *tint);
RWR_API int rwr_scene_set_sphere_glass(rwr_context *ctx, uint32_t sphere, float ior, const float *tint);
RWR_API int rwr_scene_get_part_glass(rwr_context *ctx, uint32_t part, int *is_glass, float *ior, float tint[3]);
RWR_API int rwr_scene_get_sphere_glass(rwr_context *ctx, uint32_t sphere, int *is_glass, float *ior, float tint[3]);

/* RWR_FLAG_GLOSSY: the gloss attribute of a scene part or of a sphere index, with the mirror attribute's index and reset rules.
 * reflectance: 3 floats, each finite and in [0, 1]; NULL = not glossy (roughness is then ignored).  roughness: finite, in
 * [2^-10, 1] (a perfect mirror is the mirror setter's job).  Anything else, NaN included: RWR_ERR_INVALID_ARGUMENT and the old state
 * stays.  A surface has one model: an accepted call of a gloss setter clears the surface's mirror and glass attribute, an accepted
 * call of a mirror or glass setter its gloss (with NULL any of them makes the surface diffuse).  Every accepted call changes the
 * scene's generation.  The surface keeps 1.0f + roughness; the roughness the frame uses, and the getters return, is that minus
 * 1.0f (a multiple of 2^-23).  The getters return *is_glossy = 0 / 1 and, for a glossy surface, its reflectance and roughness
 * (zeros otherwise); every output may be NULL. */
RWR_API int rwr_scene_set_part_gloss(rwr_context *ctx, uint32_t part, const float *reflectance, float roughness);
RWR_API int rwr_scene_set_sphere_gloss(rwr_context *ctx, uint32_t sphere, const float *reflectance, float roughness);
RWR_API int rwr_scene_get_part_gloss(rwr_context *ctx, uint32_t part, int *is_glossy, float reflectance[3], float *roughness);
RWR_API int rwr_scene_get_sphere_gloss(rwr_context *ctx, uint32_t sphere, int *is_glossy, float reflectance[3], float *roughness);

/* RWR_FLAG_EMISSIVE: the emission attribute of a scene part or of a sphere index, with the mirror attribute's index and reset rules
 * (part < rwr_scene_part_count, reset by a new scene; sphere < RWR_MAX_SPHERES, kept per index whatever rwr_scene_set_spheres
 * holds).  radiance: 3 floats, each finite and in [0, RWR_MAX_EMISSION]; NULL or 0, 0, 0 = does not emit (-0.0 is kept as 0).
 * Anything else, NaN and inf included: RWR_ERR_INVALID_ARGUMENT and the old state stays.  Emission stands beside the surface's
 * model: these setters leave the mirror, glass and gloss attributes alone, and those setters leave the emission alone.  Every
 * accepted call changes the scene's generation, also one that sets the value the surface already has.  The getters return
 * *emits = 0 / 1 and the radiance (zeros for a surface that does not emit); every output may be NULL. */
#define RWR_MAX_EMISSION 64.0f
RWR_API int rwr_scene_set_part_emission(rwr_context *ctx, uint32_t part, const float *radiance);
RWR_API int rwr_scene_set_sphere_emission(rwr_context *ctx, uint32_t sphere, const float *radiance);
RWR_API int rwr_scene_get_part_emission(rwr_context *ctx, uint32_t part, int *emits, float radiance[3]);
RWR_API int rwr_scene_get_sphere_emission(rwr_context *ctx, uint32_t sphere, int *emits, float radiance[3]);

/* Replaces Sphere::new's uniform, one per analytic sphere pass, composited in
 * array order before the mesh (src/lib.rs:532-534, 1106-1173).  n <= RWR_MAX_SPHERES. */
RWR_API int rwr_scene_set_spheres(rwr_context *ctx, const rwr_sphere_buffer_data *spheres, uint32_t n);

/* Replaces Triangle::new's uniform (src/models/triangle/triangle.rs:37-45), one per single-triangle pass
 * (triangle/compute.wgsl:153-195).  The reference never dispatches this model, so where its passes sit
 * in a frame is defined here: after the spheres, before the mesh, in array order.  Its shading is the
 * sphere's with the face normal as triangleRayIntersect returns it there — flipped towards the ray, NOT
 * normalised (:120-124,171-187).  n <= RWR_MAX_TRIANGLES; reference frame only (spp 1, no bounce, no
 * RWR_FLAG_USE_BVH). */
RWR_API int rwr_scene_set_triangles(rwr_context *ctx, const rwr_triangle_buffer_data *triangles, uint32_t n);

/* Extension: rigid instances of the uploaded mesh (InstanceRaw layout).
 * n = 0 restores the single un-instanced mesh of the reference. */
RWR_API int rwr_scene_set_instances(rwr_context *ctx, const rwr_instance_raw *instances, uint32_t n);

/* ---------------------------------------------------------------- frame -- */

/* Replaces State::resize's target (re)creation: screen_texture (rgba8unorm),
 * depth_texture_input/output (r32float) — src/lib.rs:470-515, 772-860. */
RWR_API int rwr_resize(rwr_context *ctx, const rwr_screen *screen);

/* Replaces State::render's GPU work, src/lib.rs:1024-1184: clear, sphere passes,
 * depth copies and the mesh pass, as ONE fused launch when params are the
 * reference's (spp 1, no bounce); the wavefront integrator otherwise.
 * Asynchronous.  `params` may be NULL (= {1,0,0,0}). */
RWR_API int rwr_render(rwr_context *ctx, const rwr_camera_inv_uniform *camera, const rwr_render_params *params);

/* Same, restricted to framebuffer rows [row_begin,row_end): the band one rank
 * renders when a frame is split across GPUs.  Pixels are addressed and the RNG
 * is keyed by GLOBAL pixel coordinates, so bands assemble bit-identically. */
RWR_API int rwr_render_rows(rwr_context *ctx, const rwr_camera_inv_uniform *camera,
                            const rwr_render_params *params, uint32_t row_begin, uint32_t row_end);

/* Same, restricted to every strip_stride-th STRIP of RWR_STRIP_ROWS rows, starting with strip first_strip
 * (< strip_stride): rows 8 (first_strip + k strip_stride) + 0..7.  The INTERLEAVED partition of a frame across
 * GPUs — rwr_render_strips(ctx, camera, params, rank, world) — gives every rank the same share of whatever part
 * of the screen the scene covers; contiguous bands (rwr_render_rows) leave most ranks idle when it covers a few
 * rows (measured: the x16 instanced grid of BASELINE configs[4] sits in two of eight bands).  Same global pixel
 * addressing and RNG keys: strips assemble bit-identically. */
#define RWR_STRIP_ROWS 8u
RWR_API int rwr_render_strips(rwr_context *ctx, const rwr_camera_inv_uniform *camera,
                              const rwr_render_params *params, uint32_t first_strip, uint32_t strip_stride);

RWR_API int rwr_synchronize(rwr_context *ctx);

/* Copies finished targets to host memory (synchronises first).  Any pointer may
 * be NULL.  rgba8: W*H*4 bytes (screen_texture); depth: W*H floats
 * (depth_texture_output); the last three need RWR_FLAG_AUX_OUTPUTS on the render. */
RWR_API int rwr_readback(rwr_context *ctx, uint8_t *rgba8, float *depth,
                         float *rgba_f32, int32_t *obj_id, float *hit_t);

/* Device addresses of the targets of the frame rendered last, for zero-copy consumers
 * (presentation, interop).  Does not wait on the host: it orders the context's stream
 * (rwr_ctx_get_stream) after that frame, so work the caller enqueues there next sees the finished
 * targets; a consumer on another stream synchronises with rwr_synchronize.  The addresses stay the same from frame to
 * frame with one frame in flight (the default) and alternate between the target sets otherwise;
 * valid until the next rwr_resize / rwr_ctx_set_frames_in_flight. */
RWR_API int rwr_get_device_targets(rwr_context *ctx, void **d_rgba8, void **d_depth);

/* ------------------------------------------------------- multi-GPU frames -- */
/* The reference is single-device (one wgpu Adapter/Device, src/lib.rs:266-303, one surface, :1226); north_star asks
 * for frames partitioned across the GPUs of a node with a single RCCL gather of the finished tiles.  Model: ONE
 * PROCESS AND ONE CONTEXT PER GPU (rwr_ctx_create(device)), every rank holds the whole scene and renders its row
 * band with rwr_render_rows (pixels and the RNG are keyed by global coordinates: bands assemble bit-identically),
 * then every rank calls rwr_dist_gather_rgba8: its band goes to `root` over xGMI — RCCL point-to-point sends
 * grouped into one operation, enqueued on the stream of the frame just rendered, bands landing in final image
 * order in a buffer the root's context owns.  RCCL is loaded at run time by rwr_dist_get_unique_id / rwr_dist_init;
 * hosts that never call these need no RCCL.
 *   rank 0:  rwr_dist_get_unique_id(id)  -> the launcher hands `id` to every rank (any channel: a file, a socket,
 *            torchrun's store) ->  all ranks: rwr_dist_init(ctx, rank, world, id).                                */
#define RWR_DIST_ID_BYTES 128
RWR_API int rwr_dist_get_unique_id(uint8_t id[RWR_DIST_ID_BYTES]);
RWR_API int rwr_dist_init(rwr_context *ctx, int rank, int world, const uint8_t id[RWR_DIST_ID_BYTES]);
/* The band partition every rank must use: rows [rank*H/world, (rank+1)*H/world). */
RWR_API int rwr_dist_band(uint32_t rank, uint32_t world, uint32_t height, uint32_t *row_begin, uint32_t *row_end);
/* Collective, asynchronous (stream-ordered after the frame rendered last).  Every frame slot
 * (rwr_ctx_set_frames_in_flight) owns its own message / receive / frame buffers, so the gather of one frame runs beside
 * the render of the next; the RCCL exchanges themselves stay in call order. */
RWR_API int rwr_dist_gather_rgba8(rwr_context *ctx, int root);
/* The same for the interleaved partition (every rank rendered rwr_render_strips(ctx, ..., rank, world)): each rank packs
 * its strips into one message (one launch), the root deals the received strips out into the frame (one launch).  One
 * grouped exchange per frame. */
RWR_API int rwr_dist_gather_strips_rgba8(rwr_context *ctx, int root);
/* Root only: device address of the assembled W*H*4 frame gathered last / copy to the host (waits for that gather).  With
 * several frames in flight the address alternates between the slots' buffers. */
RWR_API int rwr_dist_frame(rwr_context *ctx, void **d_rgba8);
RWR_API int rwr_dist_readback(rwr_context *ctx, uint8_t *rgba8);
/* Collective: returns when every rank's frames in flight have finished (an all-reduce of one word). */
RWR_API int rwr_dist_barrier(rwr_context *ctx);
RWR_API int rwr_dist_destroy(rwr_context *ctx);

/* The layout of the interleaved partition's gather, as the library itself uses it (csrc/rwr_strips.h) — for a host that
 * wants to size buffers or exchange the messages by other means.  Rank `rank` of `world` owns `strips` strips of the
 * frame's `n_strips` (strip s belongs to rank s % world); its message is those strips back to back, `rows` rows
 * (a short last strip of the frame ends the message of the rank that owns it: owns_tail); in the root's receive buffer
 * (`recv_rows_total` rows) that message starts at row `recv_row` (messages start on whole-strip boundaries). */
typedef struct rwr_strip_layout {
    uint32_t n_strips, strips, rows, recv_row, recv_rows_total, owns_tail;
} rwr_strip_layout;
RWR_API int rwr_dist_strip_layout(uint32_t rank, uint32_t world, uint32_t height, rwr_strip_layout *out);
/* Pack and deal-out on HOST memory by the same layout (byte moves only; the render path stays on the GPU): for a host
 * that stages the exchange through CPU memory, and for the world-size-2/3 tests that run over gloo without a GPU.
 * message: rank's strips back to back (8 * strips rows of capacity); recv: recv_rows_total rows. */
RWR_API int rwr_dist_host_pack_strips(uint32_t rank, uint32_t world, uint32_t width, uint32_t height,
                                      const uint8_t *frame_rgba8, uint8_t *message);
RWR_API int rwr_dist_host_deal_strips(uint32_t world, uint32_t width, uint32_t height, const uint8_t *recv, uint8_t *frame_rgba8);
/* The frame kernel's form of a diffuse texture, computed on the HOST (for inspection and tests; the library builds it at
 * upload): (tex_w + 1) * (tex_h + 1) records of 4 uint32, row pitch tex_w + 1.  Record (px, py) holds the texels
 * (px-1, py-1), (px, py-1), (px-1, py), (px, py), each coordinate clamped to the texture, as r << 2 | g << 12 | b << 22 of
 * its sRGB bytes (alpha is not kept). */
RWR_API int rwr_host_texture_quads(const uint8_t *rgba8_srgb, uint32_t tex_w, uint32_t tex_h, uint32_t *out);
/* Self-test of the gather's own stages on ONE GPU for any world size, no communicator: the context plays every rank in
 * turn.  After rendering rank's share (rwr_render_strips(ctx, ..., rank, world), or rwr_render_rows of rwr_dist_band
 * with strips = 0) _deposit runs that rank's side of the gather on the frame just rendered — the same pack launch, message
 * size and receive address as rwr_dist_gather_[strips_]rgba8 — with a device copy in place of the ncclSend/ncclRecv
 * pair; after the last rank _finish runs the root's deal-out.  rwr_dist_readback / rwr_dist_frame then return the frame
 * a root would hold. */
RWR_API int rwr_dist_loopback_deposit(rwr_context *ctx, uint32_t rank, uint32_t world, int strips);
RWR_API int rwr_dist_loopback_finish(rwr_context *ctx, uint32_t world, int strips);

/* hipEvent timing on the stream(s) the kernels are launched on: rwr_timer_begin waits until nothing
 * is in flight and records; rwr_timer_end joins every frame in flight into the end event. */
RWR_API int rwr_timer_begin(rwr_context *ctx);
RWR_API int rwr_timer_end(rwr_context *ctx, float *elapsed_ms); /* synchronises on the end event */
/* The same end in two halves, for a caller that waits for the device itself: rwr_timer_stop only
 * enqueues the end event (no host wait), rwr_timer_elapsed waits for it and reads the interval. */
RWR_API int rwr_timer_stop(rwr_context *ctx);
RWR_API int rwr_timer_elapsed(rwr_context *ctx, float *elapsed_ms);

/* Per-kernel timing for roofline accounting: when every_n > 0, every n-th render call
 * brackets its DOMINANT kernel (k_primary; for the wavefront integrator all sample passes of
 * the frame) with hipEvents on the launch stream.  rwr_kernel_timing_stats synchronises and
 * returns the mean duration in microseconds over the brackets recorded since it was enabled
 * (at most 256 are kept) and their count. */
RWR_API int rwr_ctx_set_kernel_timing(rwr_context *ctx, uint32_t every_n);
RWR_API int rwr_kernel_timing_stats(rwr_context *ctx, double *mean_us, uint32_t *count);

/* Segments (rays) traced by the last render call, for Mray/s accounting:
 * W*rows*spp primary + bounce rays actually emitted, of every generation with RWR_FLAG_MULTI_BOUNCE (an accumulating frame:
 * its own spp; 0 past the cap). */
RWR_API int rwr_last_render_stats(rwr_context *ctx, uint64_t *primary_rays, uint64_t *bounce_rays);

/* k_frame_setup launches this context has put on its streams since it was created.  A frame slot keeps its per-frame records
 * (culling records, ray tables, per-tile face sets) while everything they are made from stands still — camera uniform,
 * screen, the call's rows, scene — and a frame that finds them made launches no setup: the count then stays where it was.
 * RWR_SETUP_CACHE=0 (read when the context is created) makes them every frame.  Frames are the same bytes either way.
 * Host-side, does not wait.  NULL ctx or launches: RWR_ERR_INVALID_ARGUMENT. */
RWR_API int rwr_frame_setup_launches(rwr_context *ctx, uint64_t *launches);

/* The kept plane of ray directions.  While the camera rests, the two-pixel frame kernel (the reference frame: spp 1, no bounce,
 * culled, no normal maps, two launches per frame) loads the normalised ray directions of its pixels from a plane the frame slot
 * keeps — 24 bytes per pixel pair of the launch's workgroups, allocated by the first build — instead of computing them from the
 * ray tables.  Per slot: a frame whose camera uniform, screen and rows are those of the slot's frame before fills the plane once
 * (one launch of k_ray_plane, which calls the frame kernel's own ray function); frames after it load; a frame with another
 * camera, screen or rows computes its rays as ever and leaves no plane.  Scene changes do not touch the plane.  Frames wider
 * than 3840 or higher than 2160 pixels, and frames whose plane cannot be allocated, compute their rays.
 * builds: k_ray_plane launches this context has put on its streams since it was created; frames: frames that loaded their rays
 * from a plane.  RWR_RAY_PLANE=0 (read when the context is created) switches the plane off: both stay 0.  Frames are the same
 * bytes either way.  Host-side, does not wait.  A NULL argument is RWR_ERR_INVALID_ARGUMENT. */
RWR_API int rwr_ray_plane_stats(rwr_context *ctx, uint64_t *builds, uint64_t *frames);

/* The tile classes of the frame rendered last.  With the per-tile face sets (above), k_frame_setup leaves one class word per
 * 32x4-pixel tile of the two-pixel frame kernel's grid, and the kernel takes one of three ways through a tile by it: a tile no
 * face and no sphere can show in stores the clear values; a tile with exactly one face and no sphere tests and shades that face
 * without the state of earlier passes; every other tile runs the whole kernel.  A word holds
 *   bits 0-1    0: no face survives the tile's culling, or the tile lies outside the mesh's screen rectangle; 1: one; 2: more
 *   bits 8-15   the face's index when bits 0-1 are 1
 *   bits 16-23  bit s set: sphere s's silhouette rectangle touches the tile
 * grid_x, grid_y: the kernel's grid of 64x8-pixel workgroups for the frame's rows; classes (may be NULL: the dimensions alone)
 * receives 4 * grid_x * grid_y words, word 4 * (by * grid_x + bx) + w for the tile at pixel (64 bx + 32 (w & 1), first row of
 * strip by + 4 (w >> 1)); capacity: words `classes` has room for.  Waits for that frame alone.  RWR_TILE_CLASS=0 (read when the
 * context is created) makes the kernel ignore the words — frames are the same bytes either way — the setup writes them all the
 * same.  RWR_ERR_NOT_READY when the last frame has none (another kernel or form, more than 256 faces, RWR_TILE_LISTS=0). */
RWR_API int rwr_debug_tile_classes(rwr_context *ctx, uint32_t *classes, size_t capacity, uint32_t *grid_x, uint32_t *grid_y);

/* The cover words of the frame rendered last: one word per tile beside the class words (same grid, same order, same arguments as
 * rwr_debug_tile_classes).  A frame that finds its slot's records made (rwr_frame_setup_launches: it adds no launch) runs the
 * tiles of class "one face, no sphere" and, where the kernel's own hit test finds that every pixel pair of the tile hits that
 * face, wins the depth test and stays in the domain of the short division and depth forms, sets the tile's word to 1; the slot's
 * later frames with the same records take such a tile without the edge-0 product, the compares and the selects that could only
 * confirm it — t, u, v, depth, shading and texture are computed as ever, frames are the same bytes.  Every k_frame_setup launch
 * zeroes the words it reaches, so they stand exactly as long as the records they were learnt from; a frame that made its records
 * neither reads nor writes them.  RWR_TILE_COVER=0 (read when the context is created): no frame does, the words stay 0.
 * Waits for that frame alone.  RWR_ERR_NOT_READY when the last frame has no class words. */
RWR_API int rwr_debug_tile_cover(rwr_context *ctx, uint32_t *cover, size_t capacity, uint32_t *grid_x, uint32_t *grid_y);

/* frames: frames of this context so far that looked at cover words (above).  tiles_last: tiles the frame rendered last took as
 * covered (0 when it did not look, and for a slot's first such frame, which learns them); counted on the host from the words, so
 * it waits for that frame when it is not 0 by rule.  A NULL argument is RWR_ERR_INVALID_ARGUMENT. */
RWR_API int rwr_tile_cover_stats(rwr_context *ctx, uint64_t *frames, uint64_t *tiles_last);

/* frames: frames of this context so far that the frame kernel's lean resting form rendered: a frame that looks at cover words
 * (above), loads its rays from the slot's kept plane and writes colour and depth alone — a resting camera's plain frame of a scene
 * with per-tile face sets and one material.  The form has no culling records in LDS and no workgroup barrier and stays within the
 * scalar registers at which a CU holds eight of its workgroups; frames are the same bytes as the cover form's.
 * RWR_LEAN_REST=0 (read when the context is created): such frames run the cover form, the count stays 0.
 * A NULL argument is RWR_ERR_INVALID_ARGUMENT. */
RWR_API int rwr_lean_rest_stats(rwr_context *ctx, uint64_t *frames);

/* How the last frame of the wavefront integrator walked the BVH per lane, for its trace stage (the bounce rays) and its shadow stage
 * (RWR_FLAG_SHADOWS) separately: {launches, nodes_in_lds, stack16, wide}.  launches: per-lane kernel launches the stage put on its
 * streams (the trace stage: one per generation and launch group, beside the packet kernel when the scene has one — which pools
 * each of the two traces is decided on the device; the shadow stage has no other kernel) — 0 for a stage the frame did not have
 * (no bounce / no shadow rays), and then the other three are 0 too, not a plan nobody used.  nodes_in_lds, stack16, wide: the form of
 * the stage's launches (one per frame: it depends on the scene and the context alone) — the nodelets staged in LDS, 16-bit
 * traversal stack entries (a scene of at most 4 095 world faces and 32 767 nodes), 1 024-thread workgroups around one copy of the
 * nodelets (the trace stage alone).  RWR_WF_STACK16=0 (read when the context is created) makes every frame keep 32-bit entries —
 * and so never the wide form, which needs the 16-bit ones; any other value leaves the rule alone: the variable cannot give 16-bit
 * entries to a scene beyond the limit.  Frames are the same bytes either way.  Recorded on the host when the frame is enqueued: no
 * wait.  Zeros before the first such frame.  A NULL argument is RWR_ERR_INVALID_ARGUMENT. */
RWR_API int rwr_last_traversal_plan(rwr_context *ctx, uint32_t trace[4], uint32_t shadow[4]);

/* RWR_FLAG_SHADOWS: shadow rays traced by the last render call (= hits shaded: primary hits and the bounce hits of every
 * generation; an accumulating frame: its own samples; 0 without the flag) and how many of them were occluded.  Exact counts.
 * Waits for the frame, as rwr_last_render_stats does.  A NULL argument is RWR_ERR_INVALID_ARGUMENT. */
RWR_API int rwr_last_shadow_stats(rwr_context *ctx, uint64_t *shadow_rays, uint64_t *occluded);

/* RWR_FLAG_GLASS: what the glass hits of the last render call did — Fresnel reflections, transmissions, total internal
 * reflections (an accumulating frame: its own samples; zeros for a frame the flag did nothing to).  Exact counts.  Waits for the
 * frame, as rwr_last_render_stats does.  A NULL argument is RWR_ERR_INVALID_ARGUMENT. */
RWR_API int rwr_last_glass_stats(rwr_context *ctx, uint64_t *reflected, uint64_t *transmitted, uint64_t *tir);

/* RWR_FLAG_GLOSSY: the rays the glossy hits of the last render call sent on (an accumulating frame: its own samples; zero for a
 * frame the flag did nothing to).  An exact count.  Waits for the frame, as rwr_last_render_stats does.  A NULL argument is
 * RWR_ERR_INVALID_ARGUMENT. */
RWR_API int rwr_last_gloss_stats(rwr_context *ctx, uint64_t *glossy_rays);

/* RWR_FLAG_EMISSIVE: the shaded hits of the last render call that lay on a surface with Le != 0 — h0 and every bounce hit, over all
 * samples the call traced (an accumulating frame: its own samples; zero for a frame the flag did nothing to).  An exact count.
 * Waits for the frame, as rwr_last_render_stats does.  A NULL argument is RWR_ERR_INVALID_ARGUMENT. */
RWR_API int rwr_last_emission_stats(rwr_context *ctx, uint64_t *emissive_hits);

/* RWR_FLAG_LIGHT_SAMPLING: of the last render call, over all samples it traced — the light rays traced (item 3: a sample with
 * d2 > R*R and ndw > 0), those that reached their sphere, and the hits item 4 silenced (Le taken as 0) or, under
 * RWR_FLAG_LIGHT_MIS, weighted (Le m(g') in its place: the count is the same).  Zeros for a frame the flag did nothing to.  Exact counts.  Waits for the frame, as rwr_last_render_stats does.  A NULL argument is RWR_ERR_INVALID_ARGUMENT. */
RWR_API int rwr_last_light_stats(rwr_context *ctx, uint64_t *light_rays, uint64_t *reached, uint64_t *suppressed_hits);

/* RWR_FLAG_LIGHT_PARTS: the mesh light's share of each of rwr_last_light_stats' counts (which stay the light stage's totals) — the
 * light rays aimed at a face (item 6: d2 > 0 and ndw > 0), those that reached it, and the hits on faces of emitting parts that
 * item 8 silenced or RWR_FLAG_LIGHT_MIS weighted.  Zeros for a frame the flag did nothing to.  Exact counts.  Waits for the frame.  A NULL argument is
 * RWR_ERR_INVALID_ARGUMENT. */
RWR_API int rwr_last_part_light_stats(rwr_context *ctx, uint64_t *light_rays, uint64_t *reached, uint64_t *suppressed_hits);
/* RWR_FLAG_LIGHT_SKY: the sky's share of rwr_last_light_stats' three counts — the light rays aimed at the image, those that reached it,
 * and the misses of diffuse rays that item 6 silenced or weighted.  Zeros for a frame without the flag in effect. */
RWR_API int rwr_last_sky_light_stats(rwr_context *ctx, uint64_t *light_rays, uint64_t *reached, uint64_t *suppressed_misses);

/* Progressive accumulation (RWR_FLAG_ACCUMULATE).  One context holds one accumulation.
 * rwr_accum_reset: the next accumulating frame starts over at N = 0 (host-side only, nothing waits).
 * rwr_accum_samples: samples per pixel held by the image of the frame rendered last — N + spp, or the N it showed past the
 * cap — and 0 when that frame did not accumulate.  Host-side, does not wait.  NULL ctx or samples: RWR_ERR_INVALID_ARGUMENT. */
RWR_API int rwr_accum_reset(rwr_context *ctx);
RWR_API int rwr_accum_samples(rwr_context *ctx, uint64_t *samples);

/* RWR_FLAG_DENOISE: the filter's parameters, per context.  iterations 1 ... 5 (default 5); sigma_color > 0, finite, with
 * 256 / (sigma_color * sigma_color) finite in f32 (default 0.04: the
 * filter sees textured radiance, and a wider tolerance blurs the texture by more than it removes noise — DESIGN.md §6); normal_cos_min, not NaN (default 0.95); depth_rel >= 0 (default
 * 0.05).  Anything else, NaN included: RWR_ERR_INVALID_ARGUMENT, and the parameters stay as they were.  params = NULL restores the
 * defaults.  Host-side, waits for nothing; frames rendered after the call use the new values.  An accumulation goes on. */
typedef struct rwr_denoise_params {
    uint32_t iterations;
    float sigma_color, normal_cos_min, depth_rel;
} rwr_denoise_params;
RWR_API int rwr_denoise_set_params(rwr_context *ctx, const rwr_denoise_params *params);
RWR_API int rwr_denoise_get_params(rwr_context *ctx, rwr_denoise_params *out);

/* RWR_FLAG_TONEMAP: the stage's parameters, per context.  curve: one of RWR_TONEMAP_* (default RWR_TONEMAP_ACES); auto_exposure 0
 * (default): E = exposure, 1: E = (key / G) * exposure with G, the log-average luminance, measured from the frame on the GPU (the
 * flag's items 3 and 4); exposure, a linear factor (default 1) and key (default 0.18), each finite and in [2^-16, 2^16]; white,
 * Reinhard's white point — the input that maps to 1 — (default 4), finite and in [2^-8, 2^16].  Anything else, NaN included,
 * curve > 2 or auto_exposure > 1: RWR_ERR_INVALID_ARGUMENT, and the parameters stay as they were.  params = NULL restores the
 * defaults.  Host-side, waits for nothing; frames rendered after the call use the new values.  An accumulation and a reprojection
 * history go on.
 * rwr_last_tonemap_stats: the measure's log_sum and count and the exposure E of the frame rendered last (the flag's item 7; E is
 * computed on the host from the two sums, by the function the GPU uses).  Waits for the frame, as rwr_last_render_stats does. */
enum { RWR_TONEMAP_CLAMP = 0, RWR_TONEMAP_REINHARD = 1, RWR_TONEMAP_ACES = 2 };
typedef struct rwr_tonemap_params {
    uint32_t curve;
    uint32_t auto_exposure;
    float exposure;
    float key;
    float white;
} rwr_tonemap_params;        /* 20 bytes */
#define RWR_TONEMAP_DEFAULTS {RWR_TONEMAP_ACES, 0u, 1.0f, 0.18f, 4.0f}   /* an initialiser of rwr_tonemap_params: what NULL restores */
RWR_API int rwr_tonemap_set_params(rwr_context *ctx, const rwr_tonemap_params *params);
RWR_API int rwr_tonemap_get_params(rwr_context *ctx, rwr_tonemap_params *out);
RWR_API int rwr_last_tonemap_stats(rwr_context *ctx, int64_t *log_sum, uint32_t *count, float *exposure);

/* RWR_FLAG_SKY: the sky's two colours, per context.  In S(D) at the flag u is 1 straight up, 1/2 along the geometric horizon and 0
 * straight down: `zenith` is the radiance at u = 1, `horizon` the radiance at u = 0, the mean of the two along the horizon.
 * Defaults: zenith (0.5, 0.7, 1.0), horizon (1, 1, 1); params = NULL restores them.  Every component must be finite and in
 * [0, 16]; anything else, NaN included: RWR_ERR_INVALID_ARGUMENT, and the parameters stay as they were.  Host-side, waits for
 * nothing; frames rendered after the call use the new values. */
typedef struct rwr_sky_params {
    float zenith[3];
    float horizon[3];
} rwr_sky_params;
#define RWR_SKY_DEFAULTS {{0.5f, 0.7f, 1.0f}, {1.0f, 1.0f, 1.0f}}   /* an initialiser of rwr_sky_params: what NULL restores */
#define RWR_SKY_COMPONENT_MAX 16.0f                                 /* the largest component rwr_sky_set_params takes */
RWR_API int rwr_sky_set_params(rwr_context *ctx, const rwr_sky_params *params);
RWR_API int rwr_sky_get_params(rwr_context *ctx, rwr_sky_params *out);

/* RWR_FLAG_SKY_IMAGE: the sky's image, per context — an octahedral map of n x n texels (the flag's item 1), n * n * 3 floats
 * (r, g, b), row-major, row j <-> v, column i <-> u.  2 <= n <= RWR_SKY_IMAGE_SIZE_MAX; every component finite and in
 * [0, RWR_SKY_IMAGE_COMPONENT_MAX] (the integrator's per-term clamp, the range of Le); anything else, NaN included:
 * RWR_ERR_INVALID_ARGUMENT naming the first offending index and value, and the image stays as it was.  rgb = NULL or n = 0 removes
 * the image.  The image is kept on the device as one float4 per texel (w = 0).  Every successful call, a removal included, advances
 * the 64-bit image generation, also with equal contents.  A frame already enqueued keeps the image it was enqueued with (its frame
 * slot holds on to that buffer); the call itself may wait for the device: the upload is synchronous, and so is the release of a buffer
 * that no frame slot holds any more.
 * rwr_sky_get_image_info: n (0 when no image is held) and the generation; either pointer may be NULL. */
#define RWR_SKY_IMAGE_SIZE_MAX 2048u
#define RWR_SKY_IMAGE_COMPONENT_MAX 64.0f
RWR_API int rwr_sky_set_image(rwr_context *ctx, const float *rgb, uint32_t n);
RWR_API int rwr_sky_get_image_info(rwr_context *ctx, uint32_t *n, uint64_t *generation);
/* RWR_FLAG_LIGHT_SKY: the sampling table a frame under the flag would use — n, the image's side (0 when there is no image or the image
 * has no weight: the flag is not effective), and the generation of the image it was built for.  Builds the table if the image has
 * changed since (what the first frame under the flag would do); either pointer may be NULL. */
RWR_API int rwr_sky_get_light_info(rwr_context *ctx, uint32_t *n, uint64_t *generation);
/* Host only, no context and no device: turns a latitude-longitude picture (w x h x 3 floats, row 0 = straight up, the centre column
 * = direction (0, 0, -1), columns increasing towards +x) into the n x n x 3 octahedral map `out` that rwr_sky_set_image takes.  Per
 * output texel the mean of 4 x 4 sub-positions; each is mapped to a direction by the inverse of the flag's mapping, the direction to
 * source coordinates with atan2 / acos in double, the source fetched bilinearly (wrapping in longitude, clamping in latitude); the
 * mean times `scale`, clamped to [0, 64], as float.  w, h >= 1, w * h <= 2^28, 2 <= n <= RWR_SKY_IMAGE_SIZE_MAX, scale finite and
 * >= 0, every source component finite: else RWR_ERR_INVALID_ARGUMENT. */
RWR_API int rwr_sky_image_from_equirect(const float *rgb, uint32_t w, uint32_t h, float scale, uint32_t n, float *out);

/* RWR_FLAG_SOFT_SHADOWS: the angular size of the two lights, per context.  A radius is the tangent of the half-angle under which a
 * hit sees the light: mesh_light_radius for the mesh shader's light (face hits), sphere_light_radius for the sphere shader's.
 * Defaults 0.05 and 0.05; params = NULL restores them.  Each radius must be finite and in [0, 1]; anything else, NaN included:
 * RWR_ERR_INVALID_ARGUMENT, and the parameters stay as they were.  Host-side, waits for nothing; frames rendered after the call
 * use the new values. */
typedef struct rwr_shadow_params {
    float mesh_light_radius, sphere_light_radius;
} rwr_shadow_params;
#define RWR_SHADOW_DEFAULTS {0.05f, 0.05f}   /* an initialiser of rwr_shadow_params: what NULL restores */
#define RWR_SHADOW_RADIUS_MAX 1.0f            /* the largest radius rwr_shadow_set_params takes */
RWR_API int rwr_shadow_set_params(rwr_context *ctx, const rwr_shadow_params *params);
RWR_API int rwr_shadow_get_params(rwr_context *ctx, rwr_shadow_params *out);

/* RWR_FLAG_REPROJECT: the stage's parameters, per context.  max_history 1 ... 1024 (default 32): the longest history a pixel's
 * blend weighs in, out = hist + (c_now - hist) / n' with n' <= max_history; normal_cos_min finite and in [-1, 1] (default 0.95) and
 * depth_rel finite and >= 0 (default 0.05): the tap tests of the flag's item 4, the denoiser's defaults.  Anything else, NaN
 * included: RWR_ERR_INVALID_ARGUMENT, and the parameters stay as they were.  params = NULL restores the defaults.  Host-side,
 * waits for nothing.  Every accepted call starts a new history, also one that sets the values the context already has. */
typedef struct rwr_reproject_params {
    uint32_t max_history;
    float normal_cos_min, depth_rel;
} rwr_reproject_params;
RWR_API int rwr_reproject_set_params(rwr_context *ctx, const rwr_reproject_params *params);
RWR_API int rwr_reproject_get_params(rwr_context *ctx, rwr_reproject_params *out);
/* rwr_reproject_reset: the next reprojecting frame starts a new history, k = 0 (host-side only, nothing waits).
 * rwr_reproject_frames: how many frames the history of the frame rendered last holds — k + 1, and 0 when that frame did not
 * reproject.  Host-side, does not wait.
 * rwr_last_reproject_stats: pixels of the last render call that blended with the history (reused), hit pixels that found none
 * (fresh) and background pixels; exact counts, reused + fresh + background = width * height (zeros when that frame did not
 * reproject).  Waits for the frame, as rwr_last_render_stats does.
 * rwr_reproject_readback: the width * height f32 plane n' of the frame rendered last (RWR_ERR_NOT_READY when it did not
 * reproject).  It synchronises, as rwr_readback does.  A NULL argument is RWR_ERR_INVALID_ARGUMENT. */
RWR_API int rwr_reproject_reset(rwr_context *ctx);
RWR_API int rwr_reproject_frames(rwr_context *ctx, uint64_t *frames);
RWR_API int rwr_last_reproject_stats(rwr_context *ctx, uint64_t *reused, uint64_t *fresh, uint64_t *background);
RWR_API int rwr_reproject_readback(rwr_context *ctx, float *history_len);

/* Self-test of the kernels' short exact forms ("Numerics"): the frame kernel replaces the
 * shader's  ((1/d) - (1/kNear)) / ((1/kFar) - (1/kNear))  (compute.wgsl:78-80) and the three divisions
 * of normalize() (:162) by shorter instruction sequences that return the same bits.  This runs both
 * forms on the GPU: every float of the depth form's domain (about 2^31 inputs) and `normalize_count`
 * pseudo-random vectors; out4 = {depth inputs compared, depth mismatches, vectors compared, vector
 * mismatches}.  A non-zero mismatch count is a bug. */
RWR_API int rwr_selftest_exact_math(rwr_context *ctx, uint32_t normalize_count, uint32_t seed, uint64_t out4[4]);

/* Self-test of the frame kernel's short exact form of the hit test's plane distance t = tnum / ndotd (compute.wgsl:99-102):
 * `count` rounds of pseudo-random operand pairs, a wave-uniform numerator per wave as in the hit test, plus the edges of
 * the form's domain.  out4 = {in-domain quotients compared with the IEEE division, mismatches, quotients the hit test
 * takes (|ndotd| >= kEpsilon or NaN) compared through the kernel's choice of short form or IEEE division, mismatches}.
 * A non-zero mismatch count is a bug. */
RWR_API int rwr_selftest_exact_div(rwr_context *ctx, uint32_t count, uint32_t seed, uint64_t out4[4]);

/* Self-test of RWR_FLAG_SOBOL's word: out[i] = rng_sobol(pixel[i], sample[i], dim[i], seed[i]) (the flag's item 1) as the kernels'
 * device function evaluates it, for n tuples (at most 2^24 a call).  A word that differs from the definition's is a bug. */
RWR_API int rwr_selftest_sobol(rwr_context *ctx, const uint32_t *pixel, const uint32_t *sample, const uint32_t *dim, const uint32_t *seed,
                               size_t n, uint32_t *out);

/* Self-test of RWR_FLAG_SKY_IMAGE's S_img: out_rgb[3 i ...] = S_img(dirs[3 i ...]) of the context's image as the kernels' device
 * function evaluates it, for `count` directions (at most 2^24 a call).  RWR_ERR_NOT_READY while the context holds no image.  A
 * value that differs from the definition's bits is a bug. */
RWR_API int rwr_selftest_sky_image(rwr_context *ctx, const float *dirs, size_t count, float *out_rgb);
/* Self-test of RWR_FLAG_LIGHT_SKY's items 3 and 4 as the kernels' device functions evaluate them on the context's image: for tuple i,
 * out[8 i ...] = {omega.x, omega.y, omega.z, column, row (uint32 bits), P, g, 0} of the draw from the four uniforms u4[4 i ...] (in
 * [0, 1)) and of sky_light_g(omega, dot3(normal, omega), n_lights).  RWR_ERR_NOT_READY without an image or with an image of no weight. */
RWR_API int rwr_selftest_sky_light(rwr_context *ctx, const float *u4, size_t count, const float normal[3], uint32_t n_lights, float *out);

/* Measurement aid for roofline accounting (bench.py): runs a short f32 VALU loop with `waves_per_simd` (1..8)
 * waves on every SIMD and stamps the shader cycle counter against the constant 100 MHz counter.
 * out4 = {shader clock in MHz under v_fma_f32 load, shader cycles a SIMD spends per wave64 v_fma_f32,
 *         shader cycles per wave64 v_pk_fma_f32, shader clock in MHz under v_pk_fma_f32 load}. */
RWR_API int rwr_measure_valu_clock(rwr_context *ctx, uint32_t waves_per_simd, double out4[4]);
/* The shader clock under the caller's OWN workload: _start launches one idle-spinning wave on a private stream for
 * `micros` microseconds (asynchronous; render while it runs), _read waits for it and returns
 * d(shader cycle counter) / d(100 MHz counter) x 100 MHz. */
RWR_API int rwr_clock_probe_start(rwr_context *ctx, uint32_t micros);
RWR_API int rwr_clock_probe_read(rwr_context *ctx, double *shader_mhz);

/* ---------------------------------------------- host-side L2 surface (CPU) -- */

/* CameraInvUniform::update_view_proj, src/lib.rs:105-111 with camera.rs:20-30. */
RWR_API int rwr_camera_build_inv_uniform(const rwr_camera *camera, rwr_camera_inv_uniform *out);

/* CircleCameraController::update_camera, src/circle_camera_control.rs:76-105. */
enum { RWR_KEY_FORWARD = 1, RWR_KEY_BACKWARD = 2, RWR_KEY_LEFT = 4, RWR_KEY_RIGHT = 8,
       RWR_KEY_UP = 16, RWR_KEY_DOWN = 32 };
RWR_API int rwr_circle_controller_update(float speed, uint32_t pressed_keys, rwr_camera *camera);

/* resources::load_model_compute, src/resources.rs:163-264: OBJ + MTL + diffuse
 * texture from `res_dir`.  Only meshes[0]/materials[0] are exposed, as in
 * TriangleList (triangle_list.rs:212-245). */
typedef struct rwr_model rwr_model;
RWR_API int rwr_load_model_compute(const char *res_dir, const char *file_name, rwr_model **out_model);
RWR_API void rwr_model_free(rwr_model *model);
RWR_API int rwr_model_info(const rwr_model *model, uint32_t *n_meshes, uint32_t *n_materials,
                           uint32_t *n_verts, uint32_t *n_faces, uint32_t *tex_w, uint32_t *tex_h);
RWR_API const rwr_model_vertex_small *rwr_model_vertices(const rwr_model *model);
RWR_API const rwr_model_face_small *rwr_model_faces(const rwr_model *model);
RWR_API const rwr_material_data *rwr_model_material(const rwr_model *model);
RWR_API const uint8_t *rwr_model_texture_rgba8(const rwr_model *model);
/* Convenience: rwr_scene_upload_mesh(ctx, <meshes[0] / materials[0] of model>) — the reference's scene. */
RWR_API int rwr_scene_upload_model(rwr_context *ctx, const rwr_model *model);
/* Extension: every mesh of the model with ITS material (mesh.material, resources.rs:257). */
RWR_API int rwr_model_part_count(const rwr_model *model, uint32_t *n_parts);
RWR_API int rwr_model_part(const rwr_model *model, uint32_t part,
                           const rwr_model_vertex_small **verts, uint32_t *n_verts,
                           const rwr_model_face_small **faces, uint32_t *n_faces,
                           rwr_material_data *material, const uint8_t **rgba8, uint32_t *tex_w, uint32_t *tex_h);
RWR_API int rwr_scene_upload_model_all(rwr_context *ctx, const rwr_model *model);
/* Extension: the decoded map_Bump image of a part's material (cube.mtl:13), *rgba8 = NULL when the material names none
 * or the file is not there.  rwr_scene_upload_model / _all hand it to rwr_scene_set_normal_map; only renders with
 * RWR_FLAG_NORMAL_MAP look at it. */
RWR_API int rwr_model_part_normal_map(const rwr_model *model, uint32_t part, const uint8_t **rgba8, uint32_t *tex_w, uint32_t *tex_h);

/* texture::Texture::from_bytes, src/texture.rs:98-106: decode PNG/JPEG bytes to
 * RGBA8.  *out_rgba is malloc'd; free with rwr_free(). */
RWR_API int rwr_decode_image_rgba8(const uint8_t *bytes, size_t n_bytes,
                                   uint8_t **out_rgba, uint32_t *out_w, uint32_t *out_h);
RWR_API void rwr_free(void *p);

/* Presentation step (role of src/screenquad.wgsl + the sRGB swapchain,
 * src/lib.rs:39-64, 310-315, 1186-1224): writes a framebuffer as an RGBA8 PNG.
 * flip_vertical != 0 puts framebuffer row 0 at the BOTTOM of the image, as the
 * reference's blit does; encode_srgb != 0 applies the linear->sRGB transfer the
 * sRGB surface format applies on store. */
RWR_API int rwr_write_png_rgba8(const char *path, const uint8_t *rgba8, uint32_t width, uint32_t height,
                                int flip_vertical, int encode_srgb);

/* The grid of Instance{position,rotation}.to_raw() of src/lib.rs:400-421 for a
 * given NUM_INSTANCES_PER_ROW / SPACE_BETWEEN; out must hold per_row*per_row. */
RWR_API int rwr_make_instance_grid(uint32_t per_row, float space_between, rwr_instance_raw *out);

#ifdef __cplusplus
}
#endif
#endif /* RWR_HIP_H */
