// scene_accel.hpp — host-side build of the scene accelerator (include/rrte_hip_accel.h):
// a bounding-volume tree over the objects' culling spheres; see scene_accel.hip.  Plain C++ (no HIP
// types), so tests/cpp/accel_host_check.cpp links the builder without a device compiler.
#pragma once

#include <cstdint>
#include <vector>

namespace rrte {

constexpr uint32_t kAccelMaxPrims = 16384u;  // = RRTE_ACCEL_MAX_PRIMS: the per-wave candidate mask is 2 KiB of LDS
constexpr uint32_t kAccelStack = 32u;        // the wave's stack of links: most records on a root-to-leaf path
constexpr uint32_t kAccelLeaf = 4u;          // most objects of one leaf
constexpr uint32_t kAccelLeafBit = 0x80000000u;

// A link is an interior record index (bit 31 clear) or a leaf (bit 31 set, object count - 1 in bits
// 24-30, first entry of `leaf_prims` in bits 0-23): the mesh BVH's link (scene_view.hpp MeshView).
// Record k = nodes[16k .. 16k+15], four float4 as the mesh record's: child 0 box min (w = child 0
// link), child 0 box max (w = split axis), child 1 box min (w = child 1 link), child 1 box max.
struct AccelTree {
    std::vector<float> nodes;          // 16 floats per interior record
    std::vector<uint32_t> leaf_prims;  // object indices, leaf after leaf (ascending within a leaf)
    std::vector<uint32_t> always;      // ceil(n / 32) dwords: bit i set = object i has no finite bound
    uint32_t root = kAccelLeafBit;
    uint32_t depth = 0;                // most records on a root-to-leaf path (0: the root is a leaf)
    uint32_t bounded = 0, unbounded = 0;
    // The candidate loop reads the mask in groups of (1 << group_shift) dwords, at most 64 groups, and
    // skips a group no walk touched: bit g of always_groups = some dword of group g of `always` is not 0
    uint32_t group_shift = 0;
    uint64_t always_groups = 0;
};

enum class AccelBuild { Built, NoBound, TooDeep, TooMany };

// Builds the tree over `n` culling spheres (`bounds`: centre x y z and radius per object, radius
// +inf or any non-finite number = never culled).  Objects with a finite sphere go into leaves of at
// most kAccelLeaf objects, the others into `always`.  Anything but Built leaves `out` empty: no object
// with a finite bound (n == 0 included), more than kAccelMaxPrims objects, or more than `max_depth`
// records on some root-to-leaf path.
AccelBuild accel_build(const float* bounds, uint32_t n, uint32_t max_depth, AccelTree& out);

// The box of a culling sphere as the tree stores it: [c - r, c + r] per axis, evaluated in double and
// rounded to f32 outwards and then one more ulp out.  lo/hi: three floats each.
void accel_sphere_box(const float* sphere, float* lo, float* hi);

}  // namespace rrte
