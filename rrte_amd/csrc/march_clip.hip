// march_clip.hip — rrte_hip_march_clip (include/rrte_hip_clip.h): the enclosure constants a FULL
// specialised kernel folds in for one object, computed by the very function the kernel evaluates at
// compile time (march_clip.hpp clip::info, included here without its device overloads).  Host only.
#include "context.hpp"
#include "sdf_guard.hpp"
#include "../../include/rrte_hip_clip.h"

#define RRTE_MARCH_CLIP_HOST 1
#include "march_clip.hpp"

using namespace rrte;

extern "C" rrte_status rrte_hip_march_clip(const rrte_scene_ir* s, uint32_t object, rrte_clip_info* out) {
    if (!s || !out || object >= s->num_prims || !s->prims || (s->num_sdf_nodes && !s->sdf_nodes)) return RRTE_INVALID_ARG;
    if ((s->num_mesh_indices && !s->mesh_indices) || (s->num_mesh_vertices && !s->mesh_vertices)) return RRTE_INVALID_ARG;
    std::vector<DPrim> prims;
    std::vector<DMaterial> mats;
    std::vector<DLight> lights;
    lower_scene(s, prims, mats, lights);
    // (the nodes as a kernel gets them: with the guard links of the CSG early-out)
    const std::vector<rrte_sdf_node> nodes = decorate_scene_sdf(s, env_guard_setting());
    *out = rrte_clip_info{};
    const DPrim& pr = prims[object];
    if (pr.kind == RRTE_PRIM_SDF && (uint64_t)pr.sdf_first + pr.sdf_count > nodes.size()) return RRTE_INVALID_ARG;
#if RRTE_MARCH_CLIP
    const clip::Info ci = clip::info(pr, nodes.data());
    out->cls = ci.cls;
    out->c1 = ci.c1;
    out->c2 = ci.c2;
    for (int j = 0; j < 3; ++j) {
        out->a_center[j] = ci.a.c[j];
        out->b_center[j] = ci.b.c[j];
    }
    out->a_c0 = ci.a.c0;
    out->b_c0 = ci.b.c0;
#endif
    return RRTE_OK;
}
