/*
 * rrte_hip_refit.h — deforming meshes: the vertices of the scene's mesh arrays move, the topology
 * (vertex count, index count, every index value) stays.  Skinned characters, cloth, morph targets.
 *
 * Handing the library new vertices with a new mesh_version alone makes the next render rebuild every
 * range's BVH on the host and upload all of it.  Announcing the change with
 * rrte_hip_mesh_refit first keeps the trees: the next scene version copies the stored mesh data, ships
 * the 24-byte vertices beside it and recomputes the triangle records, the boxes (bottom-up) and the
 * culling spheres on the device.  A mesh is still the closest hit over its triangles
 * in index order, ties to the lower index: a refitted tree reports bit for bit the hits a rebuilt one
 * does, because its boxes stay conservative; it may traverse slower once the deformation is large.
 *
 * Conventions are those of rrte_hip.h.  The render ABI (rrte_hip.h, RRTE_ABI_VERSION) is unchanged
 * by this header.
 */
#ifndef RRTE_HIP_REFIT_H
#define RRTE_HIP_REFIT_H

#include "rrte_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The mesh arrays of `scene` are a deformation of the arrays the context's mesh data was last built
 * (or last refitted) from: same num_mesh_vertices, same num_mesh_indices, the same index values;
 * positions and normals may differ.  Host only: no device work, nothing is drained, no collective,
 * an open gather batch stays open.  On RRTE_OK the context's mesh cache is re-keyed to the identity
 * of `scene`'s arrays (addresses, counts, mesh_version; their content when mesh_version is 0) and
 * marked deformed.  The next render or query of a scene with these arrays takes the mesh-cache-hit
 * path and refits on the device instead of building.
 *
 * RRTE_INVALID_ARG (message in rrte_hip_last_error, the context exactly as it was, so the caller's
 * next plain render simply builds): no valid mesh cache; a count differs; an index value differs from
 * the indices the cache was built from; the set of ranges `scene`'s objects name differs from the
 * cached set; a vertex position is not finite. */
rrte_status rrte_hip_mesh_refit(rrte_ctx* ctx, const rrte_scene_ir* scene);

typedef struct rrte_refit_info {
    uint64_t refits;        /* accepted rrte_hip_mesh_refit calls since the context was created   */
    uint64_t device_refits; /* scene versions whose mesh data was produced by the refit kernels   */
    uint32_t levels;        /* launches of the propagate kernel per device refit (tree depth)     */
    uint32_t deformed;      /* 1 while the cache is in the deformed state                         */
} rrte_refit_info;          /* 24 bytes */

/* Host only.  `levels` describes the cached topology once it has been refitted (0 before). */
rrte_status rrte_hip_refit_info(rrte_ctx* ctx, rrte_refit_info* out);

/* Diagnostic read-back of the current scene version's BVH interior records (64 bytes each: child 0
 * box lo + link, hi + axis, child 1 box lo + link, hi).  Waits for that version's upload event, copies
 * min(bytes, all) bytes, writes the record count to *records (0 without a current scene).  `out` may
 * be null when bytes is 0. */
rrte_status rrte_hip_mesh_nodes(rrte_ctx* ctx, void* out, size_t bytes, uint32_t* records);

/* Diagnostic, host only: which triangle each device triangle slot holds, as its index within its
 * range (slots lie range after range, ranges in order of first appearance in the object list; a leaf
 * link of the node records names its first slot and count).  Fixed by the build, unchanged by a
 * refit.  Writes min(count, all) values and the slot count to *slots.  With rrte_hip_mesh_nodes
 * this lets a checker recompute every box from the vertices. */
rrte_status rrte_hip_mesh_slots(rrte_ctx* ctx, uint32_t* out, size_t count, uint32_t* slots);

#ifdef __cplusplus
}
#endif

#endif /* RRTE_HIP_REFIT_H */
