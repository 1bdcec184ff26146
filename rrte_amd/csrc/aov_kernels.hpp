// aov_kernels.hpp — frame AOVs (include/rrte_hip_aov.h) for gfx950: what the pixel-centre primary
// ray of every pixel of a rectangle hits, stored as separate planes.
//
// One wave64 per 8x8 pixel tile of the rectangle (tile origin = the rectangle's corner), one lane per
// pixel (lane & 7 = column, lane >> 3 = row), one wave per 64-thread workgroup like the frame kernel
// (mesh_stack() sizes its LDS by kBlockThreads).  A lane's ray is rrte_hip_pick's ray of its pixel;
// the search is closest_hit_search (ray_query.hpp), the one body the query kernels run, over every
// object or over the accelerator's candidates.  So a plane value is bit for bit the field of the
// rrte_ray_hit that rrte_hip_pick returns for the pixel.
//
// Lanes outside the rectangle (the right and bottom partial tiles; 63 of 64 lanes of a 1x1 rectangle)
// follow ray_query.hpp's rule: the search holds wave-wide operations (the __all of the CSG guards,
// readfirstlane in the winner walk, the accelerator's walk), so such a lane never returns early.  It
// stays in the wave with a benign ray over the empty interval [+inf, -inf], for which every
// intersector reports no hit, and it neither loads nor stores.
//
// Stores: one plain vector store per requested plane per lane, a float[4] plane as one 16-byte
// store.  The plane mask is a launch argument, so every store sits behind a wave-uniform branch.  No
// LDS staging, no atomics.
//
// Included by aov.hip only (not embedded for hiprtc: AOVs always take the runtime-scene path; no
// header of the Makefile's DEVICE_HDR may include this one).
#pragma once

#include "../../include/rrte_hip_aov.h"
#include "accel_kernels.hpp"

namespace rrte {

static_assert(kBlockThreads == 64u, "one wave per workgroup: one lane per pixel of an 8x8 tile");
constexpr uint32_t kAovTile = 8u;  // tile edge in pixels

// One launch: the frame's camera, the rectangle [x0, x0 + w) x [y0, y0 + h) in frame pixels, and the
// planes, row-major over that rectangle with pitch w (a null pointer where planes lacks the bit).
struct AovArgs {
    QueryCam qc;
    uint32_t x0, y0, w, h;
    uint32_t planes, tiles_x;
    float bg[4];  // rrte_render_params::background (ALBEDO of a miss)
    float* depth;
    int32_t* prim;
    int32_t* material;
    uint32_t* tri;
    float4* normal;
    float4* position;
    float4* albedo;
};

template <class S, class Visit>
__device__ __forceinline__ void aov_tile(const S& sc, const AovArgs& a, Visit&& make_visit) {
    // (a 1-D grid: the tile rows of a tall rectangle exceed gridDim.y's limit)
    const uint32_t tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const uint32_t i = tx * kAovTile + (threadIdx.x & (kAovTile - 1u));
    const uint32_t j = ty * kAovTile + (threadIdx.x >> 3);
    const bool live = i < a.w && j < a.h;
    // idle lanes: a benign ray over the empty interval
    Ray r{V(0.0f, 0.0f, 0.0f), V(0.0f, 1.0f, 0.0f)};
    float t_min = kInf, t_max = -kInf;
    if (live) {
        // rrte_hip_pick's ray of pixel (x0 + i, y0 + j): the frame kernel's u, v for RRTE_JITTER_CENTER
        const float u = ((float)(a.x0 + i) + 0.5f) / (float)a.qc.width;
        const float v = ((float)(a.y0 + j) + 0.5f) / (float)a.qc.height;
        r = generate_ray(a.qc.cam, u, v);
        t_min = a.qc.t_min;
        t_max = kInf;
    }
    const ClosestHit c = closest_hit_search(sc, r, t_min, t_max, live, make_visit(r, t_min, t_max));
    if (live) {
        const size_t o = (size_t)j * a.w + i;
        const Hit& h = c.h;
        const int material = c.idx >= 0 ? sc.prims[c.idx].material : -1;
        if (a.planes & RRTE_AOV_DEPTH) a.depth[o] = h.t;
        if (a.planes & RRTE_AOV_PRIM) a.prim[o] = c.idx;
        if (a.planes & RRTE_AOV_MATERIAL) a.material[o] = material;
        if (a.planes & RRTE_AOV_TRI) a.tri[o] = c.tri;
        if (a.planes & RRTE_AOV_NORMAL) a.normal[o] = make_float4(h.n.x, h.n.y, h.n.z, h.front ? 1.0f : 0.0f);
        if (a.planes & RRTE_AOV_POSITION) a.position[o] = make_float4(h.p.x, h.p.y, h.p.z, c.idx >= 0 ? 1.0f : 0.0f);
        if (a.planes & RRTE_AOV_ALBEDO) {
            float4 al = make_float4(a.bg[0], a.bg[1], a.bg[2], a.bg[3]);
            if (c.idx >= 0) {
                // material_of (shade.hpp): an index outside the materials is no material -> BLACK
                al = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if ((uint32_t)material < sc.num_materials) al = *reinterpret_cast<const float4*>(sc.mats[material].albedo);
            }
            a.albedo[o] = al;
        }
    }
}

// F: the scene features compiled in (the host picks the variant as launch_query does).
template <uint32_t F>
__global__ __launch_bounds__(kBlockThreads) void aov_kernel(SceneView scv, AovArgs a) {
    SceneViewF<F> sc;
    static_cast<SceneView&>(sc) = scv;
    aov_tile(sc, a, [&](const Ray&, float, float) { return visit_all(sc); });
}

// The accelerated form: the search over the candidates of one walk of the scene accelerator.
__global__ __launch_bounds__(kBlockThreads) void aov_accel_kernel(SceneView scv, AccelView av, AovArgs a) {
    SceneViewAccel sc;
    static_cast<SceneView&>(sc) = scv;
    sc.acc = av;
    aov_tile(sc, a, [&](const Ray& r, float t_min, float t_max) {
        return visit_candidates(sc.acc, accel_candidates(sc.acc, r, t_min, t_max));
    });
}

inline dim3 aov_grid(AovArgs& a) {
    a.tiles_x = (a.w + kAovTile - 1u) / kAovTile;
    return dim3(a.tiles_x * ((a.h + kAovTile - 1u) / kAovTile));
}

// The variant for a scene with features `need`, chosen as launch_query chooses a query's.
inline void launch_aov(uint32_t need, hipStream_t st, const SceneView& sv, AovArgs a) {
    const dim3 grid = aov_grid(a), block(kBlockThreads);
    if (need == 0u)
        hipLaunchKernelGGL((aov_kernel<0u>), grid, block, 0, st, sv, a);
    else if ((need & ~kFeatAnalytic) == 0u)
        hipLaunchKernelGGL((aov_kernel<kFeatAnalytic>), grid, block, 0, st, sv, a);
    else if ((need & ~kFeatSdf) == 0u)
        hipLaunchKernelGGL((aov_kernel<kFeatSdf>), grid, block, 0, st, sv, a);
    else if ((need & kFeatInstance) == 0u)
        hipLaunchKernelGGL((aov_kernel<kFeatAll>), grid, block, 0, st, sv, a);
    else
        hipLaunchKernelGGL((aov_kernel<kFeatEvery>), grid, block, 0, st, sv, a);
}

inline void launch_aov_accel(hipStream_t st, const SceneView& sv, const AccelView& av, AovArgs a) {
    const dim3 grid = aov_grid(a), block(kBlockThreads);
    hipLaunchKernelGGL(aov_accel_kernel, grid, block, 0, st, sv, av, a);
}

}  // namespace rrte
