// mesh_refit.hpp — device-side refit of the mesh BVHs after a deformation (include/rrte_hip_refit.h,
// DESIGN.md §17); see mesh_refit.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "bvh.hpp"

namespace rrte {

// "No parent": the leaf is its range's root (<= 4 triangles, no record).
constexpr uint32_t kRefitRoot = 0xFFFFFFFFu;

// What a refit needs besides the vertices, fixed by the topology: built once per built MeshData on
// the host (build_refit_static) and uploaded beside the vertices with every deformed scene version.
// A parent code is record * 2 + side: the child slot of that record which holds the node's box.
struct RefitStatic {
    std::vector<uint32_t> slot_vtx;   // 3 per triangle slot: its vertex indices (through tris[3k].w and the indices)
    std::vector<uint2> leaves;        // per leaf with triangles: {link, parent code or kRefitRoot}
    std::vector<uint32_t> parent;     // per interior record: parent code, or kRefitRoot for a range's root
    std::vector<uint2> order;         // records below a root, deepest first: {record, parent code}
    std::vector<uint32_t> level_off;  // level l = order[level_off[l], level_off[l + 1]); one launch each
    uint32_t levels() const { return level_off.empty() ? 0u : (uint32_t)level_off.size() - 1u; }
};

// False if `md`'s links or original indices do not describe trees over `num_indices / 3` triangles
// (cannot happen for data build_mesh_ranges made).
bool build_refit_static(const MeshData& md, const uint32_t* indices, uint32_t num_indices, RefitStatic& out);

// Each range's lo / hi from the deformed vertices: inflate() of the box over the vertices its indices
// name.  Contains the device's refitted root box (a leaf's extent and magnitude are at most the
// range's, inflate is monotone, interior boxes are exact unions); feeds only the culling spheres.
void refit_range_bounds(const rrte_scene_ir* s, MeshData& md);

// The device arrays of one scene version (all inside its one allocation).
struct RefitDevice {
    float4* nodes;
    float4* tris;
    float4* norms;
    const float2* verts;  // rrte_mesh_vertex as 3 x float2 (24-byte stride)
    const uint32_t* slot_vtx;
    const uint2* leaves;
    const uint2* order;
    uint32_t n_verts, n_slots, n_recs;
    unsigned long long* check;  // RRTE_DEBUG bit 2: the check word (bit 128 a slot or vertex index out of
                                // range, 256 a record index out of range); null = unchecked
};

// refit_leaves, then refit_level once per level, on `st`.
hipError_t launch_refit(const RefitStatic& rs, const RefitDevice& d, hipStream_t st);

// The same launches from counts alone (level l = d.order[level_off[l], level_off[l + 1])): for a
// caller whose leaves and order tables exist only on the device (mesh_build.hip).
hipError_t launch_refit_levels(uint32_t n_leaves, const uint32_t* level_off, uint32_t levels, const RefitDevice& d,
                               hipStream_t st);

}  // namespace rrte
