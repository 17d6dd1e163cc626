// host/image_codec.hpp's Radiance .hdr reader for the host tests (test_cli_sky_image.py), built the way bvh_host.cpp is.
#include <cstdint>
#include <cstring>
#include <string>

#include "image_codec.hpp"

// 0 and w, h, rgb (at most `capacity` floats are written) on success; 1 and the reader's message in err on failure
extern "C" __attribute__((visibility("default"))) int hdr_host_decode(const uint8_t *bytes, size_t n, uint32_t *w, uint32_t *h, float *rgb,
                                                                      size_t capacity, char *err, size_t err_capacity)
{
    rwr::codec::ImageF img;
    std::string msg;
    if (!rwr::codec::decode_hdr(bytes, n, img, msg)) {
        std::strncpy(err, msg.c_str(), err_capacity - 1);
        err[err_capacity - 1] = '\0';
        return 1;
    }
    *w = img.width;
    *h = img.height;
    std::memcpy(rgb, img.rgb.data(), sizeof(float) * (img.rgb.size() < capacity ? img.rgb.size() : capacity));
    return 0;
}
