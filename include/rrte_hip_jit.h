/*
 * rrte_hip_jit.h — diagnostics of the frame kernels: which kernel entry a context's last ray launch
 * ran, and the camera-ray tile rectangles the host computes for a frame.
 *
 * A straight-line FULL specialised kernel's module has two entry points (rrte_amd/csrc/jit.hip): the
 * general one, for any launch, and a plain one for the frame an engine renders in a stream -- one
 * RGBA8 frame into device memory, all rows, gamma 2.2, one sample per pixel, no RRTE_DEBUG bit -- whose
 * launch constants are compiled in.  The host picks the plain entry only when the launch meets every
 * condition it assumes; env RRTE_JIT_PLAIN=0 sends every launch to the general entry (A/B runs, tests).
 * Both entries render the same bytes.
 *
 * Conventions are those of rrte_hip.h.  The render ABI (rrte_hip.h, RRTE_ABI_VERSION) is unchanged
 * by this header.
 */
#ifndef RRTE_HIP_JIT_H
#define RRTE_HIP_JIT_H

#include "rrte_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RRTE_ENTRY_NONE    0u  /* no ray launch yet                          */
#define RRTE_ENTRY_GENERIC 1u  /* the generic kernel (no specialised kernel) */
#define RRTE_ENTRY_GENERAL 2u  /* a specialised kernel's general entry       */
#define RRTE_ENTRY_PLAIN   3u  /* a specialised kernel's plain entry         */

/* Host only: no device work, nothing is drained.  *entry = RRTE_ENTRY_* of the last ray launch the
 * context issued (a frame, a rank's share, a chunk of a blocking frame; ray queries do not count). */
rrte_status rrte_hip_jit_entry(rrte_ctx* ctx, uint32_t* entry);

/* Host only (no device, no context): the camera-ray tile rectangles of a whole frame of `scene` under
 * `params`, as a context computes them with tile culling on.  *tile_shift = 3 (8x8-pixel tiles), 4
 * (16x16 blocks) or 0 (no culling for this frame: *count = 0); rects[0..*count), *count <= 32, one per
 * object in list order: bx0 | bx1 << 8 | by0 << 16 | by1 << 24, the inclusive range of tiles whose
 * camera rays can meet the object's culling sphere (bx0 > bx1: none).  A tile outside object i's
 * rectangle skips its test; a tile outside every rectangle of a scene whose objects are all in the
 * table writes the background without casting a ray. */
rrte_status rrte_hip_tile_rects(const rrte_scene_ir* scene, const rrte_render_params* params, uint32_t* tile_shift,
                                uint32_t* count, uint32_t* rects);

#ifdef __cplusplus
}
#endif

#endif /* RRTE_HIP_JIT_H */
