/*
 * rrte_hip_build.h — the mesh build policy: who builds the BVH of a new mesh or a changed topology.
 *
 * Every distinct triangle range gets one BVH, built when the mesh arrays or the set of ranges change
 * (a mesh-cache miss).  By default a binned-SAH builder on the host makes it; under
 * RRTE_MESH_BUILD_DEVICE an LBVH (Morton order, 4-triangle leaves, Karras' radix tree) is built by
 * kernels on the context's upload stream and read back into the same mesh cache.  A
 * mesh is the closest hit over its triangles in index order, ties to the lower index, whatever tree
 * finds it: both builders report bit for bit the same hits.  What each policy costs to build and to
 * traverse is measured in DESIGN.md §19.
 *
 * Conventions are those of rrte_hip.h.  The render ABI (rrte_hip.h, RRTE_ABI_VERSION) is unchanged
 * by this header.
 */
#ifndef RRTE_HIP_BUILD_H
#define RRTE_HIP_BUILD_H

#include "rrte_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RRTE_MESH_BUILD_HOST 0u
#define RRTE_MESH_BUILD_DEVICE 1u

/* Host only: no device work, nothing is drained, an open gather batch stays open.  Any other value of
 * `policy` is RRTE_INVALID_ARG.  Affects the next mesh-cache miss only: the cache is never
 * invalidated, so switching the policy alone rebuilds nothing.  A context starts with HOST, or with
 * what the environment variable RRTE_MESH_BUILD=host|device said at rrte_hip_create.
 *
 * Under DEVICE the host builder still takes the whole cache miss (counted in host_fallbacks, nothing
 * reported: the frame is the same frame) when a vertex position a range names is not finite, a range
 * has more than 2^24 triangles, or the built tree is deeper than the traversal stack allows (more than
 * 31 records on a root-to-leaf path). */
rrte_status rrte_hip_set_mesh_build(rrte_ctx* ctx, uint32_t policy);

typedef struct rrte_build_info {
    uint64_t device_builds;   /* distinct ranges whose tree the device built since the context was created */
    uint64_t host_fallbacks;  /* mesh-cache misses under policy DEVICE that the host built                   */
    uint32_t policy;          /* RRTE_MESH_BUILD_*                                                          */
    uint32_t depth;           /* most records on a root-to-leaf path in the last device build, 0 before     */
} rrte_build_info;            /* 24 bytes */

/* Host only. */
rrte_status rrte_hip_build_info(rrte_ctx* ctx, rrte_build_info* out);

#ifdef __cplusplus
}
#endif

#endif /* RRTE_HIP_BUILD_H */
