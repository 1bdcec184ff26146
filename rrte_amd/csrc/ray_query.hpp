// ray_query.hpp — batched ray queries (include/rrte_hip_query.h) for gfx950: closest hit, any hit
// and pixel picking over the uploaded runtime scene.
//
// One wave64 lane per ray, one wave per 64-thread workgroup (mesh_stack() sizes its LDS by
// kBlockThreads).  The object loop is wave-uniform exactly as in the frame kernel: every lane tests
// object k at the same time, its record read with scalar loads (load_uniform), however incoherent
// the rays are.  The search and the attribute path are the frame kernel's own functions
// (search.hpp intersect_at / any_hit_at, mesh_walk.hpp mesh_tri_hit, intersect.hpp
// sdf_hit_attributes) with the caller's interval in place of [kp.t_min, +inf), so a query is
// bit-identical to a loop over SceneObject::intersect (raytracer.rs:103-113).
//
// Tail and finished lanes: the search contains wave-wide operations (the __all of the CSG guards in
// sdf_guard, readfirstlane in the attribute walk, __all in the any-hit loop), so a lane past
// `n` -- and an any-hit lane that has its answer -- never returns early.  It stays in the wave with
// a benign ray and the empty interval [+inf, -inf], for which every intersector reports no hit, and
// it neither loads a ray nor stores a hit.
//
// Included by the host translation unit only (not embedded for hiprtc: queries always take the
// runtime-scene path).
#pragma once

#include "../../include/rrte_hip_query.h"
#include "shade.hpp"

namespace rrte {

static_assert(kBlockThreads == 64u, "one wave per workgroup: lane = threadIdx.x, LDS stack of 64 lanes");
static_assert(sizeof(rrte_ray) == 32 && sizeof(rrte_ray_hit) == 48, "query record layout");

// rrte_hip_pick: the frame whose pixel-centre camera rays are cast.
struct QueryCam {
    FrameCam cam;
    uint32_t width, height;
    float t_min;
};

typedef uint32_t qu32x4 __attribute__((ext_vector_type(4)));

// Attributes of the winning object i of the lanes that call it (i wave-uniform): attributes_at of
// the frame kernel with the search's own t_max, so an analytic object is re-intersected with the
// search's exact arguments.  Also gives the mesh triangle's index in the caller's order.
template <class S>
__device__ __forceinline__ void query_attributes(const S& sc, uint32_t i, const Ray& r, float t_min, float t_max,
                                                 float t, uint32_t sub, Hit& out, uint32_t& tri) {
    const DPrim pr = load_uniform(sc.prims + i);
    constexpr uint32_t F = S::kFeat;
    if (pr.kind == RRTE_PRIM_SPHERE) {
        sphere_attributes(pr, r, t, out);
        return;
    }
    if constexpr ((F & kFeatSdf) != 0u) {
        if (pr.kind == RRTE_PRIM_SDF) {
            const rrte_sdf_node* nd = sc.nodes + pr.sdf_first;
            if (RRTE_SDF_LEAF_DISPATCH && pr.sdf_count == 1u) {
                with_leaf_program(nd, [&](auto, const auto& prog) { sdf_hit_attributes(prog, r, t, out); });
                return;
            }
            sdf_hit_attributes(SdfProgramT<F>{nd, pr.sdf_count}, r, t, out);
            return;
        }
    }
    if constexpr ((F & kFeatMesh) != 0u) {
        if (pr.kind == RRTE_PRIM_MESH) {
            mesh_tri_hit(sc.mesh, sub, r, t_min, t_max, out);
            tri = __float_as_uint(sc.mesh.tris[3u * sub].w);  // the slot's index within its mesh
            return;
        }
    }
    if constexpr ((F & kFeatInstance) != 0u) {
        if (pr.kind == RRTE_PRIM_MESH_INSTANCE) {
            mesh_instance_hit(pr, sc.mesh, sub, r, t_min, t_max, out);
            tri = __float_as_uint(sc.mesh.tris[3u * sub].w);
            return;
        }
    }
    if constexpr ((F & kFeatAnalytic) != 0u) intersect_at<true>(sc, i, r, t_min, t_max, out);
}

// What the closest-hit search returns: the winning object (-1: none), its hit record (the miss
// record t = +inf, everything else zero, when there is none) and, for a mesh or mesh instance, the
// triangle's index within its range.
struct ClosestHit {
    int idx;
    Hit h;
    uint32_t tri;
};

// The closest-hit search of a query, one body for every kernel that runs it (the query kernels below,
// the accelerated ones of accel_kernels.hpp, the view kernels of aov_kernels.hpp).  `visit(f)` calls
// f(k) for the objects to test, in list order: every object, or the accelerator's candidates.
//
// Idle lanes (`live` false) stay in the wave -- the search holds wave-wide operations -- with a benign
// ray over the empty interval [+inf, -inf] and never win.  raytracer.rs:103-113: list order, strict
// '<'; an SDF object marches only up to the closest hit so far (closest_t of the frame kernel, with the
// ray's own t_max).  The wave then walks its distinct winners (hit_attributes of the frame kernel).
template <class S, class Visit>
__device__ __forceinline__ ClosestHit closest_hit_search(const S& sc, const Ray& r, float t_min, float t_max, bool live,
                                                         Visit&& visit) {
    ClosestHit c;
    c.idx = -1;
    c.h.t = kInf;
    c.h.p = V(0.0f, 0.0f, 0.0f);
    c.h.n = V(0.0f, 0.0f, 0.0f);
    c.h.front = false;
    c.h.sub = 0u;
    c.tri = 0u;
    float best_t = kInf;
    uint32_t best_sub = 0u;
    visit([&](uint32_t k) {
        Hit hk;
        hk.sub = 0u;
        const bool sdf = load_uniform(&sc.prims[k].kind) == RRTE_PRIM_SDF;
        const float tm = (sdf && c.idx >= 0) ? (t_max < best_t ? t_max : best_t) : t_max;
        if (intersect_at<false>(sc, k, r, t_min, tm, hk) && live) {
            if (c.idx < 0 || hk.t < best_t) {
                best_t = hk.t;
                best_sub = hk.sub;
                c.idx = (int)k;
            }
        }
    });
    bool pending = c.idx >= 0;
    while (pending) {
        const uint32_t w = __builtin_amdgcn_readfirstlane((uint32_t)c.idx);
        if ((uint32_t)c.idx == w) {
            query_attributes(sc, w, r, t_min, t_max, best_t, best_sub, c.h, c.tri);
            pending = false;
        }
    }
    return c;
}

// `visit` of closest_hit_search for the plain scene: every object.
template <class S>
__device__ __forceinline__ auto visit_all(const S& sc) {
    return [&sc](auto&& f) {
        for (uint32_t k = 0; k < sc.num_prims; ++k) f(k);
    };
}

// ANY: RRTE_QUERY_ANY, else RRTE_QUERY_CLOSEST.  PICK: `in` holds n (x, y) pixel pairs and the rays
// are qc's pixel-centre camera rays; else `in` holds n rrte_ray records.  F: the scene features
// compiled in (the host picks the variant as launch_generic does).
template <bool ANY, bool PICK, uint32_t F>
__global__ __launch_bounds__(kBlockThreads) void ray_query_kernel(SceneView scv, const void* __restrict__ in, uint32_t n,
                                                                  QueryCam qc, qu32x4* __restrict__ hits) {
    SceneViewF<F> sc;
    static_cast<SceneView&>(sc) = scv;
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    const bool live = i < n;
    // idle lanes: a benign ray over the empty interval
    Ray r{V(0.0f, 0.0f, 0.0f), V(0.0f, 1.0f, 0.0f)};
    float t_min = kInf, t_max = -kInf;
    if (live) {
        if constexpr (PICK) {
            const uint2 p = reinterpret_cast<const uint2*>(in)[i];
            // the frame kernel's u, v for RRTE_JITTER_CENTER (ray_kernel_body camera_ray)
            const float u = ((float)p.x + 0.5f) / (float)qc.width;
            const float v = ((float)p.y + 0.5f) / (float)qc.height;
            r = generate_ray(qc.cam, u, v);
            t_min = qc.t_min;
            t_max = kInf;
        } else {
            const float4* q = reinterpret_cast<const float4*>(in) + 2u * (size_t)i;
            const float4 a = q[0], b = q[1];
            r = ray_new(V(a.x, a.y, a.z), V(b.x, b.y, b.z));  // Ray::new normalises (ray.rs:13-18)
            t_min = a.w;
            t_max = b.w;
        }
    }
    int idx = -1;
    Hit h;
    h.t = ANY ? 0.0f : kInf;
    h.p = V(0.0f, 0.0f, 0.0f);
    h.n = V(0.0f, 0.0f, 0.0f);
    h.front = false;
    h.sub = 0u;
    uint32_t tri = 0u;
    if constexpr (ANY) {
        // the first object in list order whose any-hit test reports a hit; a lane that has its
        // answer keeps testing the empty interval until every lane of the wave has one
        for (uint32_t k = 0; k < sc.num_prims; ++k) {
            Hit hk;
            const bool hit = any_hit_at(sc, k, r, t_min, idx >= 0 ? -kInf : t_max, hk);
            if (hit && idx < 0 && live) idx = (int)k;
            if (__all(idx >= 0 || !live)) break;
        }
    } else {
        const ClosestHit c = closest_hit_search(sc, r, t_min, t_max, live, visit_all(sc));
        idx = c.idx;
        h = c.h;
        tri = c.tri;
    }
    if (live) {
        const int material = idx >= 0 ? sc.prims[idx].material : -1;
        qu32x4* o = hits + 3u * (size_t)i;
        o[0] = qu32x4{__float_as_uint(h.t), (uint32_t)idx, __float_as_uint(h.p.x), __float_as_uint(h.p.y)};
        o[1] = qu32x4{__float_as_uint(h.p.z), __float_as_uint(h.n.x), __float_as_uint(h.n.y), __float_as_uint(h.n.z)};
        o[2] = qu32x4{h.front ? 1u : 0u, tri, (uint32_t)material, 0u};
    }
}

// The variant for a scene with features `need`: the first of the feature sets launch_generic's
// REFCOMPAT frames use that covers it.
template <bool ANY, bool PICK>
inline void launch_query(uint32_t need, uint32_t n, hipStream_t st, const SceneView& sv, const void* in,
                         const QueryCam& qc, void* hits) {
    const dim3 grid((n + kBlockThreads - 1u) / kBlockThreads), block(kBlockThreads);
    qu32x4* out = static_cast<qu32x4*>(hits);
    if (need == 0u)
        hipLaunchKernelGGL((ray_query_kernel<ANY, PICK, 0u>), grid, block, 0, st, sv, in, n, qc, out);
    else if ((need & ~kFeatAnalytic) == 0u)
        hipLaunchKernelGGL((ray_query_kernel<ANY, PICK, kFeatAnalytic>), grid, block, 0, st, sv, in, n, qc, out);
    else if ((need & ~kFeatSdf) == 0u)
        hipLaunchKernelGGL((ray_query_kernel<ANY, PICK, kFeatSdf>), grid, block, 0, st, sv, in, n, qc, out);
    else if ((need & kFeatInstance) == 0u)
        hipLaunchKernelGGL((ray_query_kernel<ANY, PICK, kFeatAll>), grid, block, 0, st, sv, in, n, qc, out);
    else
        hipLaunchKernelGGL((ray_query_kernel<ANY, PICK, kFeatEvery>), grid, block, 0, st, sv, in, n, qc, out);
}

}  // namespace rrte
