// The two-pixel frame kernel's tile shape, shared with the kernel that fills its kept ray plane (kernels_ray_plane.hip): both
// must give lane l of wave w of a workgroup the same pixel pair.
#pragma once

#include "rwr_device_p2.h"

// Tile of a wave: 32x4 pixels (default) or 16x8.  With 32x4 every row of a tile is one whole 128-byte line
// of the RGBA8 and the R32F target, which the streaming stores then write without a partial-line pass
// through the L2 (WRITE_SIZE = 8 B/pixel exactly; 16x8 tiles measured 10 % more); the frame time is the same.
#ifndef RWR_P2_TILE_32x4
#define RWR_P2_TILE_32x4 1
#endif

namespace rwr {

// First pixel (x even) and row of the pair of lane `lane` of wave `wave` in the workgroup whose 64x8 pixels start at
// (blk_x0, strip_y0) — k_primary_p2's px0 / py
RWR_DEV void p2_lane_pixel(uint32_t wave, uint32_t lane, uint32_t blk_x0, uint32_t strip_y0, uint32_t &px0, uint32_t &py)
{
#if RWR_P2_TILE_32x4
    px0 = blk_x0 + (wave & 1u) * 32u + 2u * (lane & 15u);
    py = strip_y0 + (wave >> 1) * 4u + (lane >> 4);
#else
    px0 = blk_x0 + wave * 16u + 2u * (lane & 7u);
    py = strip_y0 + (lane >> 3);
#endif
}

}  // namespace rwr
