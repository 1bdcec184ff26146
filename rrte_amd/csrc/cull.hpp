// cull.hpp — which objects a wave's shadow rays can reach.
//
// The objects' bounding spheres (Cull), the wave reductions (wave_min / wave_max), the bound of a
// wave's hit points (HitBound, wave_hit_bound) and the per-light candidate masks built from them
// (shadow_cull, light_cullable, shadow_cull_lanes).  A cull only skips tests that would have missed.
//
// Includes mesh_walk.hpp (kCullReach).  Included by shade.hpp.  Embedded for hiprtc (the Makefile's
// DEVICE_HDR).
#pragma once

#include "mesh_walk.hpp"

namespace rrte {

// --------------------------------------------------------------- culling
// Shadow-ray culling.  Conservative per-object bounding spheres (host-
// computed, inflated; radius +inf = never culled) let a wave drop the objects
// none of its shadow rays towards a light can reach.  The 64 object tests run
// lane-parallel (lane j tests object j) and __ballot turns them into a
// wave-uniform candidate mask, so occluded() skips culled objects with scalar
// branches.  An object that is not culled runs its exact intersector: culling
// never changes a result.  (Culling primary rays against the tile's view cone
// was measured too and did not pay: a miss is already a cheap bound test.)
struct Cull {
    const float4* __restrict__ bounds;  // one per object; nullptr = culling off
    uint32_t n;                         // objects with a bound (culling needs n <= 64)
};

// Wave-wide min / max as a wave-uniform value, on order-preserving integer keys of the floats
// (key(f) = bits ^ ((bits >> 31) & 0x7fffffff): signed-integer order = float order, -0 < +0, and the
// map is its own inverse): four DPP steps reduce each 16-lane row (quad_perm [1,0,3,2], quad_perm
// [2,3,0,1], row_half_mirror, row_mirror -- each a v_min_i32 / v_max_i32 with its DPP source, where
// a float min needs a canonicalising v_max_f32 per operand and a separate v_mov_b32_dpp), then the
// four rows' lanes 0, 16, 32, 48 are read into SGPRs and combined on the scalar unit.  No LDS round
// trips (the ds_bpermute butterfly of __shfl_xor took six dependent ones).  Call with all 64 lanes
// active; NaN-free inputs (the callers select +/-inf for unused lanes).
__device__ __forceinline__ int fkey(float f) {
    const int b = __float_as_int(f);
    return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float funkey(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }
template <bool MAX>
__device__ __forceinline__ int wave_reduce_key(int v) {
    auto op = [](int a, int b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); };
    v = op(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true));
    v = op(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true));
    v = op(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, true));
    v = op(v, __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, true));
    const int r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
    const int r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    return op(op(r0, r1), op(r2, r3));
}
__device__ __forceinline__ float wave_min(float v) { return funkey(wave_reduce_key<false>(fkey(v))); }
__device__ __forceinline__ float wave_max(float v) { return funkey(wave_reduce_key<true>(fkey(v))); }
__device__ __forceinline__ bool cull_on(const Cull& cl) { return cl.bounds != nullptr && cl.n <= 64u; }

// Bounding sphere of the wave's shading points (lanes with `hit`) grown by each lane's shadow-origin
// offset |n|*bias (normals need not be unit): centred on one used lane's point (the tile's centre
// lane 36 when it is used, else the first used lane), radius = max over used lanes of
// |p - c| + offset -- one wave reduction (the bounding box took seven: min and max of three
// coordinates and the largest offset).  `ext` stays 0 (folded into r).
struct HitBound { f3 c; float r, ext; bool any, unsafe; };
__device__ __forceinline__ HitBound wave_hit_bound(bool hit, f3 p, f3 n, float bias) {
    // the pre-pass only has to be conservative, so it uses cheap bounds: one finiteness test on a sum
    // (a NaN or infinite term, or an overflowing sum, marks the lane unusable -- the wave is then
    // not culled), the 1-ulp hardware square root scaled up by 2^-20, and the offset bound
    // bias * |n|_1 >= bias * |n|_2; the cull margin (1e-3 + 1e-4 * scale) dwarfs their rounding
    // A point beyond kCullReach also marks its lane unusable: the culls rest on "a hit the reference
    // reports lies inside the object's bound", which holds only while the intersectors' products of up
    // to three coordinates stay finite -- past that the reference reports hits with t = NaN or inf
    // for rays that pass nowhere near the object (sphere: hb^2 and a cc both +inf, disc = NaN).
    const bool use = hit && __builtin_isfinite(((p.x + p.y) + (p.z + n.x)) + (n.y + n.z)) &&
                     fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z)) < kCullReach;
    HitBound b;
    b.ext = 0.0f;
    b.unsafe = __any(hit && !use);
    const uint64_t used = __ballot(use);
    b.any = used != 0ull;
    if (!b.any) {
        b.c = V(0.0f, 0.0f, 0.0f);
        b.r = 0.0f;
        return b;
    }
    const int src = ((used >> 36) & 1ull) ? 36 : (int)__builtin_ctzll(used);
    b.c = V(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.x), src)),
            __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.y), src)),
            __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.z), src)));
    const f3 d = vsub(p, b.c);
    const float reach = __builtin_amdgcn_sqrtf(vdot(d, d)) * 1.000001f +
                        bias * ((fabsf(n.x) + fabsf(n.y)) + fabsf(n.z));  // >= 0, NaN-free on used lanes
    b.r = __int_as_float(wave_reduce_key<true>(use ? __float_as_int(reach) : 0));  // keys of floats >= 0 = bits
    return b;
}

// Shadow rays of one light: every ray runs from within `hb` (grown by the
// origin offset) to the light (point/spot; the segment ends at the light plus
// the same offset) or towards -direction (directional), so all of them lie in
// the capsule of radius hb.r + hb.ext around the axis from hb.c.  Waves with
// a non-finite hit point or normal, and directional lights whose direction is
// not unit length (the sphere tracer's bound test assumes |d| = 1), are not
// culled.  Wave-uniform inputs only: call with all 64 lanes active.
// `bnd`: lane j's object bound (load_bound, once per wave for every light).  The projection
// parameter uses the approximate reciprocal of |AB|^2: a relative error of ~1 ulp in t moves the
// capsule point by ~|AB| t 2^-23, far inside the 1e-3 + 1e-4 * scale margin.
__device__ __forceinline__ float4 load_bound(const Cull& cl) {
    const uint32_t j = threadIdx.x & 63u;
    return cl.bounds[j < cl.n ? j : 0u];
}
__device__ __forceinline__ uint64_t shadow_cull(const Cull& cl, const HitBound& hb, const DLight& l, float4 b) {
    if (!cull_on(cl) || hb.unsafe || l.kind == RRTE_LIGHT_AMBIENT) return ~0ull;
    if (!hb.any) return 0ull;
    const bool directional = l.kind == RRTE_LIGHT_DIRECTIONAL;
    const f3 ld = V(l.direction[0], l.direction[1], l.direction[2]);
    if (directional && !(fabsf(vdot(ld, ld) - 1.0f) <= 1e-3f)) return ~0ull;
    const f3 A = hb.c;
    const f3 B = directional ? vsub(A, ld) : V(l.position[0], l.position[1], l.position[2]);
    const f3 AB = vsub(B, A);
    const float ab2 = vdot(AB, AB);
    const float inv_ab2 = __builtin_amdgcn_rcpf(ab2);
    const float scale = fmaxf(fmaxf(fabsf(A.x), fabsf(A.y)), fmaxf(fabsf(A.z), fmaxf(fmaxf(fabsf(B.x), fabsf(B.y)), fabsf(B.z))));
    const float R = hb.r + hb.ext + 1e-3f + 1e-4f * scale;
    const uint32_t j = threadIdx.x & 63u;
    const f3 P = V(b.x, b.y, b.z);
    float t = vdot(vsub(P, A), AB) * inv_ab2;
    t = directional ? fmaxf(t, 0.0f) : clampf_(t, 0.0f, 1.0f);
    const f3 q = vsub(P, vadd(A, vmuls(AB, t)));
    const float rr = R + b.w;
    const bool near = vdot(q, q) <= rr * rr * 1.0001f;
    const bool cand = j < cl.n && (!(__builtin_isfinite(b.w) && ab2 > 0.0f) || near);
    return __ballot(cand);
}

// All lights' masks in one lane-parallel pass (scene-specialised kernels with objects x lights <= 64):
// lane L tests object j = L mod n against light l = L div n's capsule -- the same test as
// shadow_cull, whose per-light wave-uniform prologue (capsule axis, |AB|^2, its reciprocal, the
// margin) every light repeated on all 64 lanes -- and one ballot carries every light's n bits.
// Lights shadow_cull never culls (ambient; directional with a non-unit direction) get all-ones.
// Whether shadow_cull may cull for light I (not ambient; a directional light only with a unit
// direction): from the constant record of a full scene, by the host for a topology scene.
constexpr bool light_record_cullable(const DLight& L) {
#pragma clang fp contract(off)
    if (L.kind == RRTE_LIGHT_AMBIENT) return false;
    if (L.kind != RRTE_LIGHT_DIRECTIONAL) return true;
    const float d2 = (L.direction[0] * L.direction[0] + L.direction[1] * L.direction[1]) + L.direction[2] * L.direction[2];
    return (d2 - 1.0f <= 1e-3f) && (1.0f - d2 <= 1e-3f);
}
template <class S, uint32_t I>
constexpr bool light_cullable() {
    if constexpr (S::kTopo) {
        return S::topo_lights[I].cullable;
    } else {
        constexpr bool c = light_record_cullable(S::lights[I]);
        return c;
    }
}
template <class S>
__device__ __forceinline__ void shadow_cull_lanes(const S& sc, const Cull& cl, const HitBound& hb, uint64_t* smask) {
    constexpr uint32_t n = S::num_prims, nl = S::num_lights;
    static_assert(n * nl <= 64u && n > 0u, "one lane per (light, object)");
    auto cullable = [](auto lii) { return light_cullable<S, (uint32_t)decltype(lii)::value>(); };
    if (!cull_on(cl) || hb.unsafe || !hb.any) {
        auto fill = [&](auto lii) { smask[(uint32_t)lii] = (cullable(lii) && cull_on(cl) && !hb.unsafe) ? 0ull : ~0ull; };
        static_for<0, nl>(fill);
        return;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t l = lane / n, j = lane - l * n;
    const f3 A = hb.c;
    f3 B = A;
    bool directional = false;
    auto pick = [&](auto lii) {
        const DLight L = light_at(sc, lii);
        if (l == (uint32_t)lii) {
            if constexpr (light_kind<S, (uint32_t)decltype(lii)::value>() == RRTE_LIGHT_DIRECTIONAL) {
                B = vsub(A, V(L.direction[0], L.direction[1], L.direction[2]));
                directional = true;
            } else {
                B = V(L.position[0], L.position[1], L.position[2]);
            }
        }
    };
    static_for<0, nl>(pick);
    const f3 AB = vsub(B, A);
    const float ab2 = vdot(AB, AB);
    const float inv_ab2 = __builtin_amdgcn_rcpf(ab2);
    const float scale = fmaxf(fmaxf(fabsf(A.x), fabsf(A.y)), fmaxf(fabsf(A.z), fmaxf(fmaxf(fabsf(B.x), fabsf(B.y)), fabsf(B.z))));
    const float R = hb.r + hb.ext + 1e-3f + 1e-4f * scale;
    const float4 b = cl.bounds[j < cl.n ? j : 0u];
    const f3 P = V(b.x, b.y, b.z);
    float t = vdot(vsub(P, A), AB) * inv_ab2;
    t = directional ? fmaxf(t, 0.0f) : clampf_(t, 0.0f, 1.0f);
    const f3 q = vsub(P, vadd(A, vmuls(AB, t)));
    const float rr = R + b.w;
    const bool near = vdot(q, q) <= rr * rr * 1.0001f;
    const bool cand = l < nl && j < cl.n && (!(__builtin_isfinite(b.w) && ab2 > 0.0f) || near);
    const uint64_t m = __ballot(cand);
    constexpr uint64_t kBits = n >= 64u ? ~0ull : ((1ull << n) - 1ull);
    auto split = [&](auto lii) {
        constexpr uint32_t li = (uint32_t)lii;
        smask[li] = cullable(lii) ? ((m >> (li * n)) & kBits) : ~0ull;
    };
    static_for<0, nl>(split);
}

}  // namespace rrte
