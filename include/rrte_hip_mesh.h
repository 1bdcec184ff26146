/*
 * rrte_hip_mesh.h — mesh sharing diagnostics: how the context stores the triangle ranges that
 * RRTE_PRIM_MESH and RRTE_PRIM_MESH_INSTANCE objects name.
 *
 * A triangle range (sdf_first, sdf_count) of rrte_scene_ir.mesh_indices is stored on the device
 * once and gets one BVH, however many kind-8 and kind-9 prims name it, and the last built mesh data
 * stays on the host with the context: a scene change that leaves the mesh arrays (their addresses,
 * counts and mesh_version, or their content when mesh_version is 0) and the set of ranges as they
 * were copies it into the next scene version instead of building it again.  So
 * moving a mesh entity as an instance, or moving anything else in a scene that holds meshes, costs
 * no BVH build.
 *
 * Conventions are those of rrte_hip.h.  The render ABI (rrte_hip.h, RRTE_ABI_VERSION) is unchanged
 * by this header.
 */
#ifndef RRTE_HIP_MESH_H
#define RRTE_HIP_MESH_H

#include "rrte_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rrte_mesh_info {
    uint64_t bvh_builds;  /* BVH builds since the context was created, one per distinct range built */
    uint32_t ranges;      /* distinct triangle ranges of the current scene                          */
    uint32_t tri_slots;   /* device triangle slots of the current scene                             */
    uint32_t bvh_nodes;   /* device BVH interior records of the current scene                       */
    uint32_t _pad;
} rrte_mesh_info;   /* 24 bytes */

/* Host only: no device work, nothing is drained.  Describes the scene the context holds after its
 * last render or query (all zero but bvh_builds before the first). */
rrte_status rrte_hip_mesh_info(rrte_ctx* ctx, rrte_mesh_info* out);

#ifdef __cplusplus
}
#endif

#endif /* RRTE_HIP_MESH_H */
