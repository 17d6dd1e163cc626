// csrc/rwr_part_lights.h for the host test (test_part_light_host.py): the library's own builder of the mesh light's table
// (RWR_FLAG_LIGHT_PARTS item 2), compiled without HIP, so that its records can be held against the reference's bit for bit.
#include <stdint.h>
#include <string.h>

#include "rwr_part_lights.h"

// corners: 9 floats per world face; face_part: the part of every base face; glow: 4 floats per part.  Writes at most cap records
// (16 bytes each: rwr::PartLightRec) and returns the list's length.
extern "C" uint32_t part_light_host_build(const float *corners, uint32_t n_world_faces, const uint32_t *face_part, uint32_t n_base_faces,
                                          const float *glow, uint32_t n_parts, void *out, uint32_t cap)
{
    const std::vector<rwr::PartLightRec> list = rwr::build_part_lights(corners, n_world_faces, face_part, n_base_faces, glow, n_parts);
    const size_t n = list.size() < cap ? list.size() : cap;
    if (n) memcpy(out, list.data(), n * sizeof(rwr::PartLightRec));
    return (uint32_t)list.size();
}
