// k_ray_plane: fills a frame slot's kept plane of ray directions (rwr_internal.h RayPlane) for a camera at rest.
// The grid is the two-pixel frame kernel's own (kernels_primary_p2.hip: 64x8 pixels per workgroup, two pixels per lane) and
// every lane calls the function that kernel calls — pixel_pair_ray_dir_tab on the slot's ray tables, with its domain test and
// its fallback, in a translation unit built with the same floating-point flags — and stores what it returns.  Same function,
// same inputs, same flags: the frame kernel that loads the entry gets the bits it would have computed.
#include "rwr_internal.h"
#include "rwr_p2_tile.h"

namespace rwr {

__global__ void __launch_bounds__(256)
k_ray_plane(const float4 *__restrict__ ray_colp, const float4 *__restrict__ ray_row, uint32_t row_begin, uint32_t row_pitch,
            const rwr_camera_inv_uniform cam, const RayPlane plane)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t px0, py;
    p2_lane_pixel(wave, lane, blockIdx.x * 64u, row_begin + blockIdx.y * row_pitch, px0, py);
    // (lanes off the frame too: the tables cover whole workgroup columns and 8 rows below any band, frame_records.cpp frame_tables)
    const v3 D = pixel_pair_ray_dir_tab(cam, ray_colp, ray_row, px0, py);
    const uint32_t i = (blockIdx.y * gridDim.x + blockIdx.x) * 256u + threadIdx.x;   // < 2^24 (kRayPlaneMaxW x kRayPlaneMaxH)
    plane.xy[i] = make_float4(D.x.x, D.x.y, D.y.x, D.y.y);
    plane.z[i] = make_float2(D.z.x, D.z.y);
}

hipError_t launch_ray_plane(hipStream_t s, const FrameParams &fp, const RayPlane &plane)
{
    if (fp.row_end <= fp.row_begin || fp.width == 0) return hipSuccess;
    if (fp.width > kRayPlaneMaxW || fp.height > kRayPlaneMaxH || !plane.xy || !plane.z || !fp.ray_colp || !fp.ray_row) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ray_plane, dim3((fp.width + 63u) / 64u, band_strips(fp)), dim3(256), 0, s, fp.ray_colp, fp.ray_row,
                       fp.row_begin, fp.row_pitch, fp.cam, plane);
    return hipGetLastError();
}

hipError_t preload_kernels_ray_plane()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&k_ray_plane));
}

}  // namespace rwr
