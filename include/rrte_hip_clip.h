/*
 * rrte_hip_clip.h — diagnostics of the march clip of two-sphere CSG objects (rrte_amd/csrc/march_clip.hpp):
 * the enclosure a FULL specialised kernel tests a ray against before it marches such an object.
 *
 * Conventions are those of rrte_hip.h.  The render ABI (rrte_hip.h, RRTE_ABI_VERSION) is unchanged
 * by this header.
 */
#ifndef RRTE_HIP_CLIP_H
#define RRTE_HIP_CLIP_H

#include "rrte_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RRTE_CLIP_NONE         0u /* not clip-able: the object marches as every other SDF object   */
#define RRTE_CLIP_DIFFERENCE   1u /* (smooth) difference: the ball around part a                   */
#define RRTE_CLIP_INTERSECTION 2u /* (smooth) intersection: the two balls' intersection            */
#define RRTE_CLIP_UNION        4u /* (smooth) union: the two balls' union                          */

/* The enclosure of every point a march of the object can report as a hit.  For a ray with origin o and
 * unit direction d, part x is the ball around x_center of radius x_c0 + c1 |(o - x_center).d| + c2 |o|_1. */
typedef struct rrte_clip_info {
    uint32_t cls;       /* RRTE_CLIP_* */
    float c1, c2;
    float a_center[3];
    float a_c0;
    float b_center[3];
    float b_c0;
    uint32_t reserved;
} rrte_clip_info; /* 48 bytes */

/* Host only (no device, no context): the enclosure of object `object` of `scene`, from the function the
 * scene's FULL specialised kernel evaluates at compile time (clip::info), evaluated here by the host
 * compiler: the same f32 operations in the same order, so at most a last-bit difference from what
 * hiprtc folds, which the (1 + 2^-10) growth of every constant covers many times over.  The kernel's
 * run-time arithmetic on these constants (march_clip.hpp part_exit, reach) is not exported; the GPU
 * frames hold it.  cls = RRTE_CLIP_NONE (and zeros) for an object that is no "sphere, sphere, CSG
 * operator" program or whose constants make the kernel stand down. */
rrte_status rrte_hip_march_clip(const rrte_scene_ir* scene, uint32_t object, rrte_clip_info* out);

#ifdef __cplusplus
}
#endif

#endif /* RRTE_HIP_CLIP_H */
