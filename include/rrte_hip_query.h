/*
 * rrte_hip_query.h — batched ray queries against a scene: closest hit, occlusion and pixel picking.
 *
 * The render entry points of rrte_hip.h turn a scene and a camera into pixels; these answer which
 * object a given ray hits: the object under the mouse in an editor (the reference keeps
 * Camera::screen_to_ray, crates/rrte-core/src/camera.rs:85-101, for it), line-of-sight tests,
 * physics and placement probes.  They run the same intersectors, SDF sphere tracer and mesh BVH as
 * the frame kernel, on the same cached device scene, and are bit-identical to a loop over
 * SceneObject::intersect (raytracer.rs:103-113).
 *
 * Conventions are those of rrte_hip.h: plain C, POD structs, caller-owned buffers, an rrte_status
 * from every call with the message in rrte_hip_last_error, nothing aborts across the ABI.  The
 * render ABI (rrte_hip.h, RRTE_ABI_VERSION) is unchanged by this header.
 *
 * Queries are local calls: they never issue a collective, never close an open gather batch, and
 * leave rrte_hip_stats (frames, ray counts, jit_active) untouched.  They always run the
 * runtime-scene kernel; scene-specialised (hiprtc) kernels are not involved.
 */
#ifndef RRTE_HIP_QUERY_H
#define RRTE_HIP_QUERY_H

#include "rrte_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rrte_ray {
    float origin[3];
    float t_min;
    float direction[3];
    float t_max;
} rrte_ray;   /* 32 bytes */
/* The direction need not be unit length.  It is normalised exactly as Ray::new does
 * (ray.rs:13-18).  t is measured along the normalised direction, as SceneObject::intersect
 * reports it.  t_max may be +inf.  A non-finite or zero direction gets whatever the intersectors
 * report for it, as in the reference. */

typedef struct rrte_ray_hit {
    float t;              /* +inf on a miss */
    int32_t prim;         /* index into scene->prims; -1 = miss */
    float point[3];
    float normal[3];      /* HitInfo::new: flipped to face the ray */
    uint32_t front_face;
    uint32_t tri;         /* RRTE_PRIM_MESH: triangle index within the mesh's own range, in the
                             caller's index order; else 0 */
    int32_t material;     /* scene->prims[prim].material; -1 on a miss */
    uint32_t _pad;
} rrte_ray_hit;   /* 48 bytes */

/* RRTE_QUERY_CLOSEST: ray_color's search (raytracer.rs:103-113) with the ray's own interval.
 * Objects are visited in list order, each through its own intersect(ray, t_min, t_max); the
 * selection is a strict '<' (the lower index wins a tie); an SDF object marches only up to
 * min(t_max, closest t so far) once something has been found; the attributes come from the same
 * path the frame kernel uses.
 * RRTE_QUERY_ANY: `prim` is the first object in list order whose any-hit test (the form shadow
 * rays use) reports a hit in [t_min, t_max], `material` is its material; t, point, normal,
 * front_face and tri are zero.  A miss is prim = -1, material = -1 (and t = 0). */
#define RRTE_QUERY_CLOSEST 0u
#define RRTE_QUERY_ANY     1u

/* Upper bound of `n` per call. */
#define RRTE_QUERY_MAX_RAYS (1u << 24)

/* Blocking, host buffers: n rays in, n hits out.  `scene` goes through the context's scene cache:
 * a query after a render of the same scene uploads nothing.  `flags` is RRTE_QUERY_CLOSEST or
 * RRTE_QUERY_ANY (other bits: RRTE_INVALID_ARG); n in [1, RRTE_QUERY_MAX_RAYS]. */
rrte_status rrte_hip_raycast(rrte_ctx* ctx, const rrte_scene_ir* scene, const rrte_ray* rays, uint32_t n,
                             uint32_t flags, rrte_ray_hit* hits_out);

/* Device buffers (16-byte aligned): enqueues the query on `stream` (a hipStream_t, or null for the
 * context's stream) and returns without synchronising, like rrte_hip_render_async; the same
 * stream-lifetime rule applies (the stream stays valid until the next rrte_hip_synchronize). */
rrte_status rrte_hip_raycast_async(rrte_ctx* ctx, const rrte_scene_ir* scene, const void* d_rays, uint32_t n,
                                   uint32_t flags, void* d_hits, void* stream);

/* Closest hit under n pixels: xy holds n pairs (x, y) of pixel coordinates of a params->width x
 * params->height frame seen by scene->camera.  The device generates each pair's pixel-centre
 * camera ray -- the frame's primary ray for RRTE_JITTER_CENTER (same generate_ray, same f32 u and
 * v), t_min = params->t_min, t_max = +inf.  Of `params` only width, height and t_min are read.  A
 * coordinate outside the frame is RRTE_INVALID_ARG (nothing is written). */
rrte_status rrte_hip_pick(rrte_ctx* ctx, const rrte_scene_ir* scene, const rrte_render_params* params,
                          const uint32_t* xy, uint32_t n, rrte_ray_hit* hits_out);

#ifdef __cplusplus
}
#endif

#endif /* RRTE_HIP_QUERY_H */
