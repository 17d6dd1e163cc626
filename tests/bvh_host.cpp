// build_bvh (csrc/bvh.hpp, header-only host code) behind a C interface, for tests/test_large_scenes_host.py: built into a pytest
// temporary directory by tests/bvh_host.py.  The tree is kept between the call that builds it and the call that copies it out.
#include "bvh.hpp"

namespace {
rwr::Bvh g_bvh;
}

extern "C" {

// tri: n faces x 9 floats.  out6: {nodes, leaf_faces entries, depth of the tree build_bvh returned, depth of the binned-SAH tree
// of the same faces (build_bvh rebuilds with object-median splits when that is beyond kBvhMaxDepth), kBvhMaxDepth, kBvhMaxLeafDefault}
void bvh_host_build(const float *tri, uint32_t n, uint32_t out6[6])
{
    g_bvh = rwr::build_bvh(tri, n);
    out6[0] = (uint32_t)g_bvh.nodes.size();
    out6[1] = (uint32_t)g_bvh.leaf_faces.size();
    out6[2] = g_bvh.max_depth;
    out6[3] = rwr::build_bvh_with(tri, n, rwr::kBvhMaxLeafDefault, false).max_depth;
    out6[4] = rwr::kBvhMaxDepth;
    out6[5] = rwr::kBvhMaxLeafDefault;
}

// nodes: room for out6[0] * 32 words (a BvhNode4 is 24 floats of boxes, 4 links, 4 words of padding); leaf_faces: out6[1] words
void bvh_host_copy(uint32_t *nodes, uint32_t *leaf_faces)
{
    static_assert(sizeof(rwr::BvhNode4) == 32 * sizeof(uint32_t), "32 words a node");
    if (!g_bvh.nodes.empty()) std::memcpy(nodes, g_bvh.nodes.data(), g_bvh.nodes.size() * sizeof(rwr::BvhNode4));
    if (!g_bvh.leaf_faces.empty()) std::memcpy(leaf_faces, g_bvh.leaf_faces.data(), g_bvh.leaf_faces.size() * sizeof(uint32_t));
}

}  // extern "C"
