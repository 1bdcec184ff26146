// bvh.hpp — host-side BVH build for triangle meshes (RRTE_PRIM_MESH); see bvh.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/rrte_hip.h"
#include "device_scene.hpp"

namespace rrte {

// One distinct triangle range (sdf_first, sdf_count) of the scene's mesh arrays: built and stored once,
// whichever RRTE_PRIM_MESH / RRTE_PRIM_MESH_INSTANCE objects name it.
struct MeshRange {
    uint32_t first, count;  // the caller's triangle range
    uint32_t root;          // root link (an empty range: a leaf with no triangles)
    uint32_t slot_base;     // first triangle slot = base of its part of perm
    double lo[3], hi[3];    // the root's (inflated) box in object space
};

// Device-ready mesh data for the whole scene (layout: MeshView in scene_view.hpp).
struct MeshData {
    std::vector<float4> nodes;   // 4 per interior record: child 0 box (w link), child 1 box (w link)
    std::vector<float4> tris;    // 3 per triangle slot: v0 (w = index within the mesh), e1, e2
    std::vector<float4> norms;   // 3 per triangle slot: n0, n1, n2
    std::vector<uint32_t> perm;  // mesh's first slot + original index -> slot
    std::vector<MeshRange> ranges;  // in build order (first appearance in the object list)
    uint32_t max_depth = 0;
    bool too_deep = false;       // a subtree hit the depth cap with > 128 triangles (build refused)
};

// The distinct ranges the mesh objects (kinds 8 and 9) of `s` name, in order of first appearance.
std::vector<std::pair<uint32_t, uint32_t>> mesh_ranges_of(const rrte_scene_ir* s);

// Builds one BVH per distinct range of `s`, appending to `out`.
void build_mesh_ranges(const rrte_scene_ir* s, MeshData& out);

// Points every mesh object of `s` at its range of `md` (which must hold it): DPrim sdf_first = root
// link, sdf_count = triangles, p[0] = first triangle slot.  `bounds` (one float4 per object, may be
// null) receives each object's bounding sphere: for RRTE_PRIM_MESH the range's own, for an instance
// the range's object-space sphere through the object's xf (sphere_bound).
void assign_mesh_prims(const rrte_scene_ir* s, const MeshData& md, DPrim* prims, float4* bounds);

// build_mesh_ranges + assign_mesh_prims.
void build_mesh_bvhs(const rrte_scene_ir* s, DPrim* prims, MeshData& out, float4* bounds);

// The conservative culling sphere of an object whose intersector reports only points inside the
// sphere (c, r): given in object space when `xf` is non-null (centre through xf, radius by the
// largest column norm), then inflated so f32 rounding in the intersectors stays inside.  Radius
// +inf = never culled (r = +inf, non-finite data, or an object that reaches beyond kCullReachHost).
constexpr double kCullReachHost = 0x1p40;  // = kCullReach of mesh_walk.hpp
float4 sphere_bound(const double c[3], double r, const float* xf);

}  // namespace rrte
