// mesh_build.hpp — device-side build of the mesh BVHs: an LBVH with 4-triangle leaves (include/
// rrte_hip_build.h); see mesh_build.hip.
//
// The first part is the integer core of the build (Morton code, keys, Karras' radix-tree range and
// split search, the parent walk) as __host__ __device__ inline functions with no HIP dependency: a
// plain C++ compiler takes it too (tests/cpp/lbvh_host_check.cpp runs exactly these functions under
// the sanitizers).  The second part, hipcc only, is the builder the library calls.
#pragma once

#include <cstdint>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#define RRTE_LBVH_PLAIN_CXX 1
#endif

namespace rrte {

constexpr uint32_t kLbvhLeafMax = 4;       // triangles per leaf
constexpr uint32_t kLbvhLeafBit = 0x80000000u;
constexpr uint32_t kLbvhNoParent = 0xFFFFFFFFu;  // (= kRefitRoot)
constexpr uint32_t kLbvhWalkCap = 64;      // parent-walk steps; a walk that needs more reports kLbvhWalkCap
constexpr uint32_t kLbvhMaxRecords = 31;   // records on a root-to-leaf path the traversal stack (kMeshStack 32) takes

// 10 bits -> every third bit (bit i -> bit 3 i).
__host__ __device__ inline uint32_t lbvh_spread(uint32_t v) {
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// 30-bit Morton code of a cell: within each bit triple x is the most significant bit, then y, then z.
__host__ __device__ inline uint32_t lbvh_morton(uint32_t qx, uint32_t qy, uint32_t qz) {
    return (lbvh_spread(qx) << 2) | (lbvh_spread(qy) << 1) | lbvh_spread(qz);
}

// The cell of centre coordinate c in a centroid box [lo, lo + ext] (f32, every operation rounded on
// its own; the library is compiled with -ffp-contract=off and a correctly rounded divide).
__host__ __device__ inline uint32_t lbvh_cell(float c, float lo, float ext) {
    if (!(ext > 0.0f)) return 0u;
    const float f = (c - lo) / ext * 1024.0f;
    int q = (int)f;
    q = q < 0 ? 0 : q;
    q = q > 1023 ? 1023 : q;
    return (uint32_t)q;
}

// Sort key of a triangle: ranges follow each other, a range's triangles lie in Morton order.
__host__ __device__ inline uint64_t lbvh_tri_key(uint32_t range, uint32_t morton) {
    return ((uint64_t)range << 32) | morton;
}

// Key of leaf j of a range: the code of its first slot, then its position (unique, ascending).
__host__ __device__ inline uint64_t lbvh_leaf_key(uint32_t morton_first, uint32_t j) {
    return ((uint64_t)morton_first << 32) | j;
}

__host__ __device__ inline int lbvh_clz64(uint64_t x) { return x ? __builtin_clzll((unsigned long long)x) : 64; }

// Length of the common prefix of keys i and j; -1 when j lies outside [0, n).
__host__ __device__ inline int lbvh_delta(const uint64_t* keys, uint32_t n, uint32_t i, int64_t j) {
    if (j < 0 || j >= (int64_t)n) return -1;
    return lbvh_clz64(keys[i] ^ keys[(uint32_t)j]);
}

// Record i (0 <= i < n - 1) of the binary radix tree over n >= 2 ascending unique keys (Karras 2012):
// the leaves [first, last] it covers and its split: children cover [first, split] and [split + 1, last].
// A child that covers one leaf is that leaf, else record `split` (left) or `split + 1` (right).
struct LbvhNode {
    uint32_t first, last, split;
};

__host__ __device__ inline LbvhNode lbvh_node(const uint64_t* keys, uint32_t n, uint32_t i) {
    const int d = lbvh_delta(keys, n, i, (int64_t)i + 1) - lbvh_delta(keys, n, i, (int64_t)i - 1) >= 0 ? 1 : -1;
    const int dmin = lbvh_delta(keys, n, i, (int64_t)i - d);
    int64_t lmax = 2;
    for (int it = 0; it < 32; ++it) {  // (n < 2^32: lmax reaches past the array within 32 doublings)
        if (!(lbvh_delta(keys, n, i, (int64_t)i + lmax * d) > dmin)) break;
        lmax *= 2;
    }
    int64_t l = 0;
    for (int it = 0; it < 34; ++it) {
        lmax /= 2;
        if (lmax < 1) break;
        if (lbvh_delta(keys, n, i, (int64_t)i + (l + lmax) * d) > dmin) l += lmax;
    }
    const int64_t j = (int64_t)i + l * d;
    const int dnode = lbvh_delta(keys, n, i, j);
    int64_t s = 0, t = l;
    for (int it = 0; it < 34; ++it) {
        t = (t + 1) / 2;
        if (lbvh_delta(keys, n, i, (int64_t)i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    const int64_t gamma = (int64_t)i + s * d + (d < 0 ? -1 : 0);
    LbvhNode nd;
    nd.first = (uint32_t)(d > 0 ? (int64_t)i : j);
    nd.last = (uint32_t)(d > 0 ? j : (int64_t)i);
    nd.split = (uint32_t)gamma;
    return nd;
}

// The axis word of a record split between leaves `split` and `split + 1`: the axis of the highest
// Morton bit in which their keys differ (x 0, y 1, z 2); 0 when the codes are equal (a split by position).
__host__ __device__ inline uint32_t lbvh_axis(uint64_t ka, uint64_t kb) {
    const uint32_t x = (uint32_t)((ka ^ kb) >> 32);
    if (!x) return 0u;
    const uint32_t bit = 31u - (uint32_t)__builtin_clz(x);
    return 2u - bit % 3u;
}

// Depth of a record (root 0): the number of parent steps to a record without parent.  parent[r] is a
// parent code (record * 2 + side) or kLbvhNoParent.  A walk longer than the cap reports kLbvhWalkCap.
__host__ __device__ inline uint32_t lbvh_depth(const uint32_t* parent, uint32_t rec) {
    uint32_t d = 0;
    for (uint32_t it = 0; it < kLbvhWalkCap; ++it) {
        const uint32_t p = parent[rec];
        if (p == kLbvhNoParent) return d;
        rec = p >> 1;
        ++d;
    }
    return kLbvhWalkCap;
}

}  // namespace rrte

#ifndef RRTE_LBVH_PLAIN_CXX

#include <hip/hip_runtime.h>

#include <vector>

#include "bvh.hpp"

namespace rrte {

// One distinct range's place in the scene-wide arrays, known on the host before anything runs.
struct BuildRange {
    uint32_t first, count;   // the caller's triangle range
    uint32_t slot_base;      // first triangle slot (= first sorted position)
    uint32_t leaf_base, leaves;
    uint32_t rec_base;       // leaves - 1 records (none for leaves <= 1)
    float cb_lo[3], cb_ext[3];  // centroid box: lo and hi - lo
};

constexpr int kBuildParts = 19;  // sub-arrays of the scratch allocation (mesh_build.hip)

enum class BuildResult { Built, Fallback, HipError };

// Host times of one device build, microseconds (RRTE_HOST_PROFILE).
struct BuildTimes {
    double host_scan = 0, enqueue = 0, depth_wait = 0, boxes_enqueue = 0, readback = 0;
    uint64_t n = 0;
};

// The device-side builder of one context: plan() on the host (ranges, the finite scan, the scratch
// layout), then run() on the context's upload stream into scratch the context owns.
class DeviceBuilder {
public:
    // Lays out the build of the ranges `s` names.  False = the host builder must take this scene (a
    // non-finite named vertex position, a range above 2^24 triangles, more slots than a link can name).
    bool plan(const rrte_scene_ir* s);
    size_t scratch_bytes() const { return total_; }
    // Builds into `out` (empty on entry) through `scratch` (scratch_bytes() bytes of device memory),
    // waiting on `st` only.  `check`: the RRTE_DEBUG bit 2 check word or null.  Fallback = the measured
    // depth exceeds kLbvhMaxRecords records on a path; `out` is then left empty.  *depth = the most
    // records on a root-to-leaf path.
    BuildResult run(const rrte_scene_ir* s, uint8_t* scratch, hipStream_t st, unsigned long long* check, MeshData& out,
                    uint32_t* depth, hipError_t* err, BuildTimes* times);

private:
    std::vector<BuildRange> ranges_;
    std::vector<MeshRange> mesh_ranges_;
    uint32_t n_tris_ = 0, n_leaves_ = 0, n_recs_ = 0;
    uint32_t sort_bits_ = 32, sort_n_ = 0;  // the sort whose temporary size sort_temp_ is
    size_t sort_temp_ = 0, total_ = 0;
    size_t off_[kBuildParts + 1] = {};
};

}  // namespace rrte

#endif  // !RRTE_LBVH_PLAIN_CXX
