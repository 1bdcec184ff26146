// accel_kernels.hpp — the scene accelerator on the device (include/rrte_hip_accel.h)
// for gfx950: the wave-level walk of the top-level tree, the ordered candidate loops of the closest-hit
// and any-hit searches, and the frame and query kernels compiled with them.
//
// The tree only culls.  A wave walks it once per search: every lane slab-tests its own ray against a
// record's two child boxes, a ballot decides the descent (a child is visited if any lane accepts it),
// and a reached leaf sets its objects' bits in a per-wave mask in LDS that starts as the scene's
// always-mask.  The search then visits the set bits in ascending order -- list order -- and calls the
// frame kernel's own intersect_at / any_hit_at with exactly the linear scan's arguments.  An object
// that is skipped would have missed on every lane, so best_t, the winner, the SDF t_max narrowing and
// the tie rule are the linear scan's.
//
// The searches are overloads of search.hpp's closest_t / occluded on the accelerated scene type:
// ray_kernel_body, shade_lambert, path_step and closest_hit reach them through argument-dependent
// lookup.  They stay here, with the walk they need, and out of the embedded headers.
//
// Includes ray_kernels.hpp (ray_kernel_body, which the accelerated frame kernel instantiates),
// ray_query.hpp (the query kernels' attribute path) and scene_accel.hpp.  Included by context.hpp, so by
// the host translation units only (scene-specialised kernels have no accelerated form).
#pragma once

#include "ray_kernels.hpp"
#include "ray_query.hpp"
#include "scene_accel.hpp"

namespace rrte {

// Part of neither kFeatAll nor kFeatEvery (as kFeatInstance is no part of kFeatAll): no existing variant
// changes.  The accelerated kernels are compiled for kFeatEvery | kFeatAccel, instances included.
constexpr uint32_t kFeatAccel = 32u;

struct AccelView {
    const float4* __restrict__ nodes;          // 4 per record (scene_accel.hpp AccelTree)
    const uint32_t* __restrict__ leaf_prims;
    const uint32_t* __restrict__ always;       // `words` dwords
    unsigned long long* __restrict__ count;    // RRTE_ACCEL_COUNT: [0] walks, [1] candidates; else nullptr
    uint64_t always_groups;
    uint32_t root, words, group_shift, num_prims;
};

struct SceneViewAccel : SceneView {
    static constexpr uint32_t kFeat = kFeatEvery | kFeatAccel;
    AccelView acc;
};

__device__ __forceinline__ uint32_t* accel_mask() {
    __shared__ uint32_t m[kAccelMaxPrims / 32u];  // the wave's candidate set, one bit per object
    return m;
}
__device__ __forceinline__ uint32_t* accel_stack() {
    __shared__ uint32_t s[kAccelStack];  // the wave's stack of links (one entry per record on the path)
    return s;
}

// The lanes that take part in a walk.  The searches are called from inside the shading code's
// branches (a shadow ray exists only for lanes that hit and face the light; a path only while it is
// alive), so a walk runs with whatever lanes execute it: the others are simply not in the ballots.
// Every wave-wide step below therefore uses only __ballot / readfirstlane of the executing lanes and
// LDS words that every executing lane reads after the whole wave's writes (one wave per workgroup,
// LDS instructions of a wave complete in order; the fence keeps the compiler from reordering them).
struct AccelLanes {
    uint32_t rank, count;  // this lane's index among the executing lanes; how many execute
};
__device__ __forceinline__ AccelLanes accel_lanes() {
    const uint64_t ex = __ballot(1);
    const uint32_t lo = (uint32_t)ex, hi = (uint32_t)(ex >> 32);
    return AccelLanes{__builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u)), (uint32_t)__popcll(ex)};
}
__device__ __forceinline__ void accel_lds_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// The lane test: may this lane's ray meet the box [lo, hi] within [t_min, t_max]?  Conservative by
// construction: the box is first widened per lane by e_k = 2^-21 (max(|lo_k|, |hi_k|) +
// |o_k|) -- at least twice the distance between the exact point o + t d and the f32 point the
// intersectors report and the bounds contain -- and the slab test then accepts when tn <= tf + 2^-22
// (|tn| + |tf|) + 2^-120, which covers its own three roundings per product (and a flushed or denormal
// product).  Infinite tn / tf compare without slack; a NaN in the comparison accepts.  `mo` =
// 2^-21 |o|, `inv` = 1 / d with an overflowed reciprocal of a non-zero component replaced by NaN (that
// axis then bounds nothing).
__device__ __forceinline__ bool accel_box_hit(float4 lo, float4 hi, f3 o, f3 inv, f3 mo, float t_min, float t_max) {
    const float ex = 0x1p-21f * fmaxf(fabsf(lo.x), fabsf(hi.x)) + mo.x;
    const float ey = 0x1p-21f * fmaxf(fabsf(lo.y), fabsf(hi.y)) + mo.y;
    const float ez = 0x1p-21f * fmaxf(fabsf(lo.z), fabsf(hi.z)) + mo.z;
    const float tx0 = ((lo.x - ex) - o.x) * inv.x, tx1 = ((hi.x + ex) - o.x) * inv.x;
    const float ty0 = ((lo.y - ey) - o.y) * inv.y, ty1 = ((hi.y + ey) - o.y) * inv.y;
    const float tz0 = ((lo.z - ez) - o.z) * inv.z, tz1 = ((hi.z + ez) - o.z) * inv.z;
    const float tn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), t_min));
    const float tf = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fminf(fmaxf(tz0, tz1), t_max));
    const float a = fabsf(tn) + fabsf(tf);
    const float slack = a < kInf ? 0x1p-22f * a + 0x1p-120f : 0.0f;
    return !(tn > tf + slack);
}
__device__ __forceinline__ float accel_rcp(float d) {
    const float inv = 1.0f / d;
    return (d != 0.0f && fabsf(inv) == kInf) ? __builtin_nanf("") : inv;
}

// Sets the wave's candidate mask for the rays (r, [t_min, t_max]) of the executing lanes and returns
// which groups of its dwords hold a set bit (AccelTree::group_shift).  Lanes idled the usual way --
// t_min = +inf (a frame's lanes without a pixel) or t_max = -inf (a query's lanes past n, latched
// any-hit lanes) -- accept nothing and stay in the wave.  If a live lane's ray is non-finite or starts
// beyond kCullReach the wave takes every object: the stand-down of isect_mesh and wave_hit_bound.
__device__ __forceinline__ uint64_t accel_candidates(const AccelView& av, const Ray& r, float t_min, float t_max) {
    uint32_t* mask = accel_mask();
    uint32_t* stk = accel_stack();
    const AccelLanes ln = accel_lanes();
    const bool idle = t_min == kInf || t_max == -kInf;
    const bool wild = !idle && (!(finite3(r.o) && finite3(r.d)) ||
                                !(fmaxf(fmaxf(fabsf(r.o.x), fabsf(r.o.y)), fabsf(r.o.z)) < kCullReach));
    const bool all = __any(wild);
    const uint32_t words = av.words, gs = av.group_shift;
    uint64_t groups;
    if (all) {
        for (uint32_t w = ln.rank; w < words; w += ln.count) {
            const uint32_t left = av.num_prims - 32u * w;  // (>= 1: words = ceil(num_prims / 32))
            mask[w] = left >= 32u ? ~0u : ~(~0u << left);
        }
        const uint32_t ng = ((words - 1u) >> gs) + 1u;
        groups = ng >= 64u ? ~0ull : ~(~0ull << ng);
        accel_lds_fence();
    } else {
        for (uint32_t w = ln.rank; w < words; w += ln.count) mask[w] = av.always[w];
        groups = av.always_groups;
        accel_lds_fence();
        const f3 inv = V(accel_rcp(r.d.x), accel_rcp(r.d.y), accel_rcp(r.d.z));
        const f3 mo = V(0x1p-21f * fabsf(r.o.x), 0x1p-21f * fabsf(r.o.y), 0x1p-21f * fabsf(r.o.z));
        uint32_t link = av.root, sp = 0u;
        for (;;) {
            if (!(link & kAccelLeafBit)) {
                const float4* rec = av.nodes + 4u * (size_t)link;  // (link is wave-uniform: scalar loads)
                const float4 l0 = load_uniform(rec), h0 = load_uniform(rec + 1), l1 = load_uniform(rec + 2),
                             h1 = load_uniform(rec + 3);
                const bool a0 = __any(!idle && accel_box_hit(l0, h0, r.o, inv, mo, t_min, t_max));
                const bool a1 = __any(!idle && accel_box_hit(l1, h1, r.o, inv, mo, t_min, t_max));
                const uint32_t c0 = __float_as_uint(l0.w), c1 = __float_as_uint(l1.w);
                if (a0 && a1) {
                    stk[sp++] = c1;  // (every executing lane stores the same word)
                    link = c0;
                    continue;
                }
                if (a0 || a1) {
                    link = a0 ? c0 : c1;
                    continue;
                }
            } else {
                const uint32_t a = link & 0xFFFFFFu, n = ((link >> 24) & 0x7Fu) + 1u;
                for (uint32_t k = 0; k < n; ++k) {
                    const uint32_t i = load_uniform(av.leaf_prims + a + k);
                    mask[i >> 5] |= 1u << (i & 31u);  // (the same read-modify-write on every executing lane)
                    groups |= 1ull << ((i >> 5) >> gs);
                }
            }
            if (sp == 0u) break;
            link = __builtin_amdgcn_readfirstlane(stk[--sp]);
        }
        accel_lds_fence();
    }
    groups = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(groups >> 32)) << 32) |
             __builtin_amdgcn_readfirstlane((uint32_t)groups);
    if (av.count) {  // RRTE_ACCEL_COUNT: a launch value, so one wave-uniform branch when off
        uint32_t pop = 0u;
        for (uint32_t w = 0; w < words; ++w) pop += __popc(__builtin_amdgcn_readfirstlane(mask[w]));
        // one atomic instruction per walk: the first executing lane adds the walk, the second its candidates
        if (ln.rank < 2u) atomicAdd(av.count + ln.rank, ln.rank ? (unsigned long long)pop : 1ull);
        if (ln.count == 1u) atomicAdd(av.count + 1, (unsigned long long)pop);
    }
    return groups;
}

// Calls f(i) for every candidate i in ascending order until f returns false.  A dword is read
// wave-uniformly, its set bits are found on the scalar unit.
template <class F>
__device__ __forceinline__ void accel_for_each(const AccelView& av, uint64_t groups, F&& f) {
    const uint32_t* mask = accel_mask();
    const uint32_t gs = av.group_shift, words = av.words;
    for (uint64_t g = groups; g; g &= g - 1ull) {
        const uint32_t w0 = (uint32_t)__builtin_ctzll(g) << gs;
        const uint32_t w1 = w0 + (1u << gs) < words ? w0 + (1u << gs) : words;
        for (uint32_t w = w0; w < w1; ++w) {
            for (uint32_t m = __builtin_amdgcn_readfirstlane(mask[w]); m; m &= m - 1u)
                if (!f(32u * w + (uint32_t)__builtin_ctz(m))) return;
        }
    }
}

// closest_t of search.hpp over the candidates: the same body, the same arguments.
__device__ __forceinline__ int closest_t(const SceneViewAccel& sc, const Ray& r, float t_min, float& best_t,
                                         uint32_t& best_sub, uint32_t pmask = ~0u) {
    int idx = -1;
    best_t = kInf;
    best_sub = 0u;
    const uint64_t groups = accel_candidates(sc.acc, r, t_min, kInf);
    accel_for_each(sc.acc, groups, [&](uint32_t i) {
        if (i < 32u && !((pmask >> i) & 1u)) return true;
        Hit h;
        h.sub = 0u;
        const float tmax = (load_uniform(&sc.prims[i].kind) == RRTE_PRIM_SDF && idx >= 0) ? best_t : kInf;
        if (intersect_at<false>(sc, i, r, t_min, tmax, h)) {
            if (idx < 0 || h.t < best_t || (h.t == best_t && (int)i < idx)) {
                best_t = h.t;
                best_sub = h.sub;
                idx = (int)i;
            }
        }
        return true;
    });
    return idx;
}

// occluded of search.hpp over the candidates (`mask`: the shadow cull's, all ones here -- the
// accelerated kernels are compiled without it -- kept so that the call is the same call).
__device__ __forceinline__ bool occluded(const SceneViewAccel& sc, const Ray& r, float t_min, float t_max, uint64_t mask,
                                         int self = -1) {
    bool hit_any = false;
    const uint64_t groups = accel_candidates(sc.acc, r, t_min, t_max);
    accel_for_each(sc.acc, groups, [&](uint32_t i) {
        if (i < 64u && !((mask >> i) & 1ull)) return true;
        Hit h;
        if (!hit_any && (int)i != self && any_hit_at(sc, i, r, t_min, t_max, h)) hit_any = true;
        return !__all(hit_any);
    });
    return hit_any;
}

// The accelerated frame kernel: ray_kernel_body over the accelerated scene type, every feature
// compiled in, no shadow cull (it needs <= 64 objects; the tree culls shadow rays instead).  LDS: the
// mesh stack (8 KiB) + the candidate mask (2 KiB) + the link stack (128 B) per wave.
template <int MODE>
__global__ __launch_bounds__(kBlockThreads, 4) void ray_kernel_accel(KParams kp, SceneView sc, AccelView av,
                                                                    uint32_t* __restrict__ out_rgba8,
                                                                    float4* __restrict__ out_f32,
                                                                    unsigned long long* __restrict__ counters) {
    SceneViewAccel s;
    static_cast<SceneView&>(s) = sc;
    s.acc = av;
    ray_kernel_body<MODE, SceneViewAccel, false, false>(kp, s, Cull{nullptr, 0u}, out_rgba8, out_f32, counters);
}

// `visit` of closest_hit_search (ray_query.hpp) for the accelerated scene: the candidates `groups` of
// a walk, in list order.
__device__ __forceinline__ auto visit_candidates(const AccelView& av, uint64_t groups) {
    return [&av, groups](auto&& f) {
        accel_for_each(av, groups, [&](uint32_t k) {
            f(k);
            return true;
        });
    };
}

// The accelerated query kernel: ray_query_kernel (ray_query.hpp) with its object loops over the
// candidates: the any-hit loop here, the closest-hit search the one body of closest_hit_search.  Ray
// set-up, idle lanes and the stores are that kernel's, statement for statement.
template <bool ANY, bool PICK>
__global__ __launch_bounds__(kBlockThreads) void ray_query_accel_kernel(SceneView scv, AccelView av,
                                                                        const void* __restrict__ in, uint32_t n, QueryCam qc,
                                                                        qu32x4* __restrict__ hits) {
    SceneViewAccel sc;
    static_cast<SceneView&>(sc) = scv;
    sc.acc = av;
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    const bool live = i < n;
    Ray r{V(0.0f, 0.0f, 0.0f), V(0.0f, 1.0f, 0.0f)};
    float t_min = kInf, t_max = -kInf;
    if (live) {
        if constexpr (PICK) {
            const uint2 p = reinterpret_cast<const uint2*>(in)[i];
            const float u = ((float)p.x + 0.5f) / (float)qc.width;
            const float v = ((float)p.y + 0.5f) / (float)qc.height;
            r = generate_ray(qc.cam, u, v);
            t_min = qc.t_min;
            t_max = kInf;
        } else {
            const float4* q = reinterpret_cast<const float4*>(in) + 2u * (size_t)i;
            const float4 a = q[0], b = q[1];
            r = ray_new(V(a.x, a.y, a.z), V(b.x, b.y, b.z));
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
    const uint64_t groups = accel_candidates(sc.acc, r, t_min, t_max);
    if constexpr (ANY) {
        accel_for_each(sc.acc, groups, [&](uint32_t k) {
            Hit hk;
            const bool hit = any_hit_at(sc, k, r, t_min, idx >= 0 ? -kInf : t_max, hk);
            if (hit && idx < 0 && live) idx = (int)k;
            return !__all(idx >= 0 || !live);
        });
    } else {
        const ClosestHit c = closest_hit_search(sc, r, t_min, t_max, live, visit_candidates(sc.acc, groups));
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

template <bool ANY, bool PICK>
inline void launch_query_accel(uint32_t n, hipStream_t st, const SceneView& sv, const AccelView& av, const void* in,
                               const QueryCam& qc, void* hits) {
    const dim3 grid((n + kBlockThreads - 1u) / kBlockThreads), block(kBlockThreads);
    hipLaunchKernelGGL((ray_query_accel_kernel<ANY, PICK>), grid, block, 0, st, sv, av, in, n, qc,
                       static_cast<qu32x4*>(hits));
}

}  // namespace rrte
