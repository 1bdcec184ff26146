/*
 * rrte_hip_aov.h — frame AOVs: per-pixel depth, object and material ids, triangle index, normal,
 * position and albedo of a view.
 *
 * The render entry points of rrte_hip.h turn a scene and a camera into colour, and rrte_hip_pick
 * (rrte_hip_query.h) answers single pixels.  These answer, for a whole view or a rectangle of it,
 * what the primary ray of every pixel hit: the id buffer of selection outlines and marquee
 * selection, the depth that rasterised gizmos are composited against, the normal / albedo / depth
 * guides of a denoiser, the world position of decals and placement.  Only the requested planes
 * are computed into and moved, each as its own tightly packed array.
 *
 * The rule every plane value satisfies: pixel (x0 + i, y0 + j) of a plane holds, bit for bit, the
 * corresponding field of the rrte_ray_hit that rrte_hip_pick documents for that pixel -- the
 * pixel-centre primary ray (RRTE_JITTER_CENTER: same generate_ray, same f32 u and v, t_min =
 * params->t_min, t_max = +inf) through the loop over SceneObject::intersect in list order with a
 * strict '<' (rrte_hip_query.h RRTE_QUERY_CLOSEST).  RRTE_AOV_ALBEDO is derived from that record
 * and the scene.
 *
 * Conventions are those of rrte_hip.h: plain C, POD structs, caller-owned buffers, an rrte_status
 * from every call with the message in rrte_hip_last_error, nothing aborts across the ABI.  The
 * render ABI (rrte_hip.h, RRTE_ABI_VERSION) is unchanged by this header.
 *
 * These are local calls, like the ray queries: they never issue a collective, never close an open
 * gather batch, and leave rrte_hip_stats (frames, ray counts, jit_active) untouched.  The scene
 * goes through the context's scene cache, so the AOVs of the scene just rendered upload nothing.
 * They always run the runtime-scene kernel; scene-specialised (hiprtc) kernels are not involved.
 */
#ifndef RRTE_HIP_AOV_H
#define RRTE_HIP_AOV_H

#include "rrte_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The planes.  4-byte planes hold one element per pixel, float[4] planes four floats per pixel. */
#define RRTE_AOV_DEPTH    0x01u /* float    : t of the closest hit along the normalised primary ray; +inf on a miss   */
#define RRTE_AOV_PRIM     0x02u /* int32_t  : index into scene->prims; -1 on a miss                                    */
#define RRTE_AOV_MATERIAL 0x04u /* int32_t  : scene->prims[prim].material; -1 on a miss                                */
#define RRTE_AOV_TRI      0x08u /* uint32_t : rrte_ray_hit.tri (mesh / mesh instance: triangle within its range); else 0 */
#define RRTE_AOV_NORMAL   0x10u /* float[4] : normal xyz (HitInfo::new: flipped to face the ray), w = front_face ? 1 : 0; all 0 on a miss */
#define RRTE_AOV_POSITION 0x20u /* float[4] : hit point xyz, w = 1; all 0 on a miss                                    */
#define RRTE_AOV_ALBEDO   0x40u /* float[4] : materials[material].albedo; a material index outside
                                              scene->materials (-1: no material) -> 0,0,0,0 (ray_color's BLACK);
                                              a miss -> params->background                                             */
#define RRTE_AOV_ALL      0x7Fu

/* What to compute: the planes (a mask of RRTE_AOV_*) and the rectangle [x0, x0 + width) x
 * [y0, y0 + height) of the params->width x params->height frame seen by scene->camera.
 * width == height == 0 with x0 == y0 == 0 means the whole frame.  _pad must be zero. */
typedef struct rrte_aov_desc {
    uint32_t planes, x0, y0, width, height, _pad[3];
} rrte_aov_desc;   /* 32 bytes */

/* Where each plane goes: row-major over the rectangle, pitch = the rectangle's width, row 0 = top,
 * tightly packed.  Only the pointers of requested planes are read; the memory behind the others
 * is left untouched.  _reserved must be null. */
typedef struct rrte_aov_buffers {
    float* depth;
    int32_t* prim;
    int32_t* material;
    uint32_t* tri;
    float* normal;
    float* position;
    float* albedo;
    void* _reserved;
} rrte_aov_buffers;   /* 64 bytes */

/* Blocking, host buffers.  Of `params` only width, height, t_min and background are read.  The
 * planes are staged through context-owned device memory in chunks of whole 8-row tile rows, so a
 * call of any size uses a bounded amount of it.
 *
 * RRTE_INVALID_ARG (nothing is written, the context stays usable): a null argument; planes == 0 or
 * unknown bits; a requested plane whose pointer is null; a non-zero _pad or _reserved; an empty
 * rectangle or one that leaves the frame; a frame of zero or of more than 2^30 pixels. */
rrte_status rrte_hip_render_aov(rrte_ctx* ctx, const rrte_scene_ir* scene, const rrte_render_params* params,
                                const rrte_aov_desc* desc, const rrte_aov_buffers* out);

/* Device buffers (float[4] planes 16-byte aligned, the others 4-byte aligned; else RRTE_INVALID_ARG):
 * enqueues the work on `stream` (a hipStream_t, or null for the context's stream) and returns
 * without synchronising, like rrte_hip_render_async; the same stream-lifetime rule applies (the
 * stream stays valid until the next rrte_hip_synchronize). */
rrte_status rrte_hip_render_aov_async(rrte_ctx* ctx, const rrte_scene_ir* scene, const rrte_render_params* params,
                                      const rrte_aov_desc* desc, const rrte_aov_buffers* d_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RRTE_HIP_AOV_H */
