// sdf_eval.hpp — the value of an SDF program at a point.
//
// The leaf distances (sdf_leaf), smooth min, the deformers, one step of the postfix stack machine
// (sdf_node_step), the exact CSG early-out (sdf_guard), and the three program types a march is
// instantiated with: SdfProgramT (runtime nodes), SdfLeafProgram (one leaf, kind at compile time) and
// SdfStaticProgram (a compile-time scene's node range); with them the compile-time facts about a
// program that the secant early miss needs (leaf_convex, sdf_convex, sdf_leaf_scale).
//
// Includes scene_view.hpp.  Included by intersect.hpp.  Embedded for hiprtc (the Makefile's DEVICE_HDR).
#pragma once

#include "scene_view.hpp"

namespace rrte {

// ------------------------------------------------------------- SDF program
__device__ __forceinline__ float len2f(float a, float b) { return sqrt_rn(a * a + b * b); }
__device__ __forceinline__ float len3f(float a, float b, float c) { return sqrt_rn((a * a + b * b) + c * c); }

__device__ __forceinline__ float sdf_leaf(uint32_t op, const float* __restrict__ f, f3 p) {
    f3 q = vsub(p, V(f[0], f[1], f[2]));
    switch (op) {
    case RRTE_SDF_SPHERE:
        return len3f(q.x, q.y, q.z) - f[3];
    case RRTE_SDF_BOX: {
        float dx = fabsf(q.x) - f[4] * 0.5f, dy = fabsf(q.y) - f[5] * 0.5f, dz = fabsf(q.z) - f[6] * 0.5f;
        float outside = len3f(smx(dx, 0.0f), smx(dy, 0.0f), smx(dz, 0.0f));
        float inside = smn(smx(dx, smx(dy, dz)), 0.0f);
        return outside + inside;
    }
    case RRTE_SDF_CYLINDER: {
        float dx = len2f(q.x, q.z) - f[3], dy = fabsf(q.y) - f[4] * 0.5f;
        return smn(smx(dx, dy), 0.0f) + len2f(smx(dx, 0.0f), smx(dy, 0.0f));
    }
    case RRTE_SDF_PRISM: {
        float a = smx(fabsf(q.x) * 0.866025f + q.y * 0.5f, -q.y) - f[5] * 0.25f;
        return smx(fabsf(q.z) - f[6] * 0.5f, a);
    }
    case RRTE_SDF_TORUS: {
        float qx = len2f(q.x, q.z) - f[3];
        return len2f(qx, q.y) - f[4];
    }
    case RRTE_SDF_TUBE: {
        float rad = len2f(q.x, q.z);
        float mid = (f[3] + f[4]) * 0.5f, half = (f[3] - f[4]) * 0.5f;
        float dx = fabsf(rad - mid) - half, dy = fabsf(q.y) - f[5] * 0.5f;
        return smn(smx(dx, dy), 0.0f) + len2f(smx(dx, 0.0f), smx(dy, 0.0f));
    }
    case RRTE_SDF_RING: {
        float qx = len2f(q.x, q.y) - f[3];
        return len2f(qx, q.z) - f[4];
    }
    case RRTE_SDF_CONE: {
        float r1 = f[3], hh = f[4] * 0.5f;
        float qx = len2f(q.x, q.z), qy = q.y;
        float k2x = -r1, k2y = hh * 2.0f;
        float cax = qx - smn(qx, (qy < 0.0f) ? r1 : 0.0f);
        float cay = fabsf(qy) - hh;
        float k1mqx = 0.0f - qx, k1mqy = hh - qy;
        float tnum = k1mqx * k2x + k1mqy * k2y;
        float tden = k2x * k2x + k2y * k2y;
        float t = sclamp(div_rn(tnum, tden), 0.0f, 1.0f);
        float cbx = (qx - 0.0f) + k2x * t;
        float cby = (qy - hh) + k2y * t;
        float s = (cbx < 0.0f && cay < 0.0f) ? -1.0f : 1.0f;
        float da = cax * cax + cay * cay, db = cbx * cbx + cby * cby;
        return s * sqrt_rn(smn(da, db));
    }
    case RRTE_SDF_CAPSULE: {
        float hh = f[4] * 0.5f;
        float y = q.y - sclamp(q.y, -hh, hh);
        return len3f(q.x, y, q.z) - f[3];
    }
    case RRTE_SDF_ELLIPSOID: {
        float rx = f[4], ry = f[5], rz = f[6];
        float k0 = len3f(div_rn(q.x, rx), div_rn(q.y, ry), div_rn(q.z, rz));
        float k1 = len3f(div_rn(q.x, rx * rx), div_rn(q.y, ry * ry), div_rn(q.z, rz * rz));
        if (!(k1 > 0.0f)) return -smn(rx, smn(ry, rz));
        return k0 * (k0 - 1.0f) / k1;
    }
    default:
        return kInf;
    }
}

// smooth_min (README.md:485-488)
__device__ __forceinline__ float smin(float a, float b, float k) {
    float h = sclamp(0.5f + div_rn(0.5f * (b - a), k), 0.0f, 1.0f);
    float om = 1.0f - h;
    return (a * h + b * om) - (k * h) * om;
}

__device__ __forceinline__ f3 sdf_deform(uint32_t op, const uint32_t* __restrict__ iarg, const float* __restrict__ f,
                                         f3 p) {
    f3 c = V(f[0], f[1], f[2]);
    f3 q = vsub(p, c);
    switch (op) {
    case RRTE_SDF_TWIST:
    case RRTE_SDF_BEND: {
        uint32_t ax = iarg[0];
        uint32_t drive = (op == RRTE_SDF_TWIST) ? ax : iarg[1];
        uint32_t u = (ax + 1) % 3, w = (ax + 2) % 3;
        float s, co;
        sincos_rrte(f[3] * comp(q, drive), s, co);
        float qu = comp(q, u), qw = comp(q, w);
        q = setcomp(q, u, co * qu - s * qw);
        q = setcomp(q, w, s * qu + co * qw);
        break;
    }
    case RRTE_SDF_TAPER: {
        uint32_t ax = iarg[0];
        uint32_t u = (ax + 1) % 3, w = (ax + 2) % 3;
        float t = sclamp(div_rn(comp(q, ax) + f[5] * 0.5f, f[5]), 0.0f, 1.0f);
        float s = f[3] + (f[4] - f[3]) * t;
        q = setcomp(q, u, comp(q, u) / s);
        q = setcomp(q, w, comp(q, w) / s);
        break;
    }
    case RRTE_SDF_NOISE: {
        uint32_t oct = iarg[0], seed = iarg[1];
        f3 x = vmuls(q, f[3]);
        // q += amplitude * sum_o persistence^o * noise3(x * 2^o, seed + o * 0x85ebca6b)
        float acc[3] = {0.0f, 0.0f, 0.0f};
#if defined(RRTE_ABLATE_NOISE)  // (timing only, wrong images: the noise deformer's cost, tools/stress_ab.sh)
        (void)oct; (void)seed; (void)x;
#else
        float amp = 1.0f, fr = 1.0f;
        for (uint32_t o = 0; o < oct; ++o) {
            float nv[3];
            value_noise3(x.x * fr, x.y * fr, x.z * fr, seed + o * 0x85ebca6bu, nv);
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] = acc[k] + amp * nv[k];
            amp = amp * f[5];
            fr = fr * 2.0f;
        }
#endif
        q = V(q.x + f[4] * acc[0], q.y + f[4] * acc[1], q.z + f[4] * acc[2]);
        break;
    }
    case RRTE_SDF_WAVE: {
        uint32_t ax = iarg[0], disp = iarg[1];
        float s, co;
        sincos_rrte(f[4] * comp(q, ax), s, co);
        q = setcomp(q, disp, comp(q, disp) + f[3] * s);
        break;
    }
    default:
        break;
    }
    return vadd(q, c);
}

// One postfix node applied to the value / point stacks (leaves push a
// distance, CSG ops pop two and push one, deformers push the point and
// replace it, POP_POINT restores it).
// (op and the integer arguments separately from the float arguments: a topology kernel has the
// first two at compile time and reads the third.)
template <bool DEFORM = true>
__device__ __forceinline__ void sdf_node_step(uint32_t op, const uint32_t* iargs, const float* fargs, float* vs, f3* ps,
                                              uint32_t& sp, uint32_t& pp, f3& p) {
    if (op < 32) {
        vs[sp] = sdf_leaf(op, fargs, p);
        ++sp;
    } else if (op < 64) {
        float b = vs[sp - 1], a = vs[sp - 2], r;
        float k = fargs[0];
        switch (op) {
        case RRTE_SDF_UNION: r = smn(a, b); break;
        case RRTE_SDF_DIFFERENCE: r = smx(a, -b); break;
        case RRTE_SDF_INTERSECTION: r = smx(a, b); break;
        case RRTE_SDF_SMOOTH_UNION: r = smin(a, b, k); break;
        case RRTE_SDF_SMOOTH_DIFFERENCE: r = -smin(-a, b, k); break;
        default: r = -smin(-a, -b, k); break;
        }
        sp -= 2;
        vs[sp] = r;
        ++sp;
    } else if constexpr (DEFORM) {  // (a program of a scene without deformers has none: kFeatDeform)
        if (op < 96) {
            ps[pp] = p;
            ++pp;
            p = sdf_deform(op, iargs, fargs, p);
        } else {
            --pp;
            p = ps[pp];
        }
    }
}

// Exact CSG early-out (host analysis: sdf_guard.hip).  g = the CSG op node whose right operand B
// starts here, a = its left operand's value (top of the value stack).  Inside the guard's range
// |p - c| in [R, smax], B >= L = lambda (|p - c| - R) (inflated bound), and when L alone decides
// the op its result is exactly a (union: b >= L >= a; difference: -b <= -L <= a; smooth union /
// difference: h computed with L is 1, so h(b) is 1 by monotone rounding, and with b >= L >= 0 the
// formula reduces to a + 0 / -(-a + 0)).  Wave-uniform: taken only when every active lane may take
// it, so the result never depends on the guard.
__device__ __forceinline__ bool sdf_guard(uint32_t gop, const float* gf, float a, f3 p, float& r) {
    const float dx = p.x - gf[4], dy = p.y - gf[5], dz = p.z - gf[6];
    const float s = __builtin_amdgcn_sqrtf((dx * dx + dy * dy) + dz * dz);
    const float L = gf[8] * (s - gf[7]);
    bool ok = s >= gf[7] && s <= gf[9];
    switch (gop) {
    case RRTE_SDF_UNION:
        ok = ok && L >= a;
        r = a;
        break;
    case RRTE_SDF_DIFFERENCE:
        ok = ok && -L <= a;  // a NaN left operand fails the guard (smx(NaN, -b) is -b, not a)
        r = a;
        break;
    case RRTE_SDF_SMOOTH_UNION:
        ok = ok && sclamp(0.5f + div_rn(0.5f * (L - a), gf[0]), 0.0f, 1.0f) == 1.0f;
        r = a + 0.0f;
        break;
    default: {  // RRTE_SDF_SMOOTH_DIFFERENCE: -smin(-a, b, k)
        const float na = -a;
        ok = ok && sclamp(0.5f + div_rn(0.5f * (L - na), gf[0]), 0.0f, 1.0f) == 1.0f;
        r = -(na + 0.0f);
        break;
    }
    }
    return __all(ok);
}

// Runtime program: the program counter, op and stack pointers are
// wave-uniform (every lane runs the same program), so the stacks stay in
// registers indexed by SGPR values.  A guarded operand is skipped when its
// guard holds for the whole wave.
#ifndef RRTE_SDF_FASTPATH
#define RRTE_SDF_FASTPATH 1  // generic kernel: one-leaf / leaf-leaf-op programs off the stack machine (A/B)
#endif
template <uint32_t F = kFeatAll>
struct SdfProgramT {
    static constexpr bool kSmall = false;
    const rrte_sdf_node* __restrict__ nodes;
    uint32_t count;
    __device__ __forceinline__ float operator()(f3 p) const {
        // The two shapes most objects have -- one leaf, or two leaves under one CSG op (no deformer,
        // no guard: guards need operands of >= 2 leaves) -- evaluate without the stack machine: no
        // per-node loop, no dynamically indexed stack, and the nodes' scalar loads do not depend on
        // a loop counter (the march loop around this call can keep them in SGPRs).  Same operations
        // in the same order as the loop below, so the same bits.
        // (the program's nodes are wave-uniform: read through load_uniform, scalar loads)
        const rrte_sdf_node n0 = load_uniform(nodes);
        const uint32_t op0 = n0.op;
        if (RRTE_SDF_FASTPATH && count == 1u && op0 < 32u) return sdf_leaf(op0, n0.f, p);
        const rrte_sdf_node n1 = load_uniform(nodes + (count > 1u ? 1u : 0u));
        const rrte_sdf_node n2 = load_uniform(nodes + (count > 2u ? 2u : 0u));
        if (RRTE_SDF_FASTPATH && count == 3u && op0 < 32u && n1.op < 32u && n2.op >= 32u && n2.op < 64u && n1.i[2] == 0u) {
            const float a = sdf_leaf(op0, n0.f, p);
            const float b = sdf_leaf(n1.op, n1.f, p);
            const float k = n2.f[0];
            switch (n2.op) {
            case RRTE_SDF_UNION: return smn(a, b);
            case RRTE_SDF_DIFFERENCE: return smx(a, -b);
            case RRTE_SDF_INTERSECTION: return smx(a, b);
            case RRTE_SDF_SMOOTH_UNION: return smin(a, b, k);
            case RRTE_SDF_SMOOTH_DIFFERENCE: return -smin(-a, b, k);
            default: return -smin(-a, -b, k);
            }
        }
        float vs[RRTE_SDF_MAX_STACK];
        f3 ps[(F & kFeatDeform) ? RRTE_SDF_MAX_POINT_STACK : 1];
        uint32_t sp = 0, pp = 0;
        for (uint32_t i = 0; i < count; ++i) {
            const rrte_sdf_node ni = load_uniform(nodes + i);
            const uint32_t link = ni.i[2];
            float r;
            if (link != 0u) {
                const rrte_sdf_node gn = load_uniform(nodes + (link - 1u));
                if (sdf_guard(gn.op, gn.f, vs[sp - 1], p, r)) {
                    vs[sp - 1] = r;
                    i = link - 1u;  // continue after the op
                    continue;
                }
            }
            sdf_node_step<(F & kFeatDeform) != 0u>(ni.op, ni.i, ni.f, vs, ps, sp, pp, p);
        }
        return vs[0];
    }
};
using SdfProgram = SdfProgramT<kFeatAll>;

#ifndef RRTE_SDF_LEAF_DISPATCH
#define RRTE_SDF_LEAF_DISPATCH 1  // generic kernel: one-leaf objects march with a compile-time leaf kind (A/B)
#endif
// A one-leaf program of the generic kernel with its leaf kind known at compile time: the runtime
// scene dispatches on the leaf once per object (intersect_at), so the sphere-tracing loop runs that
// leaf's straight-line distance, as a scene-specialised kernel does, with only the leaf's sizes read
// (through scalar loads, hoisted out of the loop).  leaf_scale is sdf_leaf_scale of the one node.
template <uint32_t OP>
struct SdfLeafProgram {
    static constexpr bool kSmall = true;
    NodeArgs a;  // the node's arguments (load_uniform)
    __device__ __forceinline__ float leaf_scale() const {
        float k = 0.0f;
#pragma unroll
        for (int j = 0; j < 7; ++j) k += a.f[j] < 0.0f ? -a.f[j] : a.f[j];
        return k;
    }
    __device__ __forceinline__ float operator()(f3 p) const { return sdf_leaf(OP, a.f, p); }
};
// Leaves whose one-leaf program is convex and 1-Lipschitz whatever their sizes (sdf_convex; the cone
// only for radius and height > 0, a runtime fact, so not here): the secant early miss applies.
template <uint32_t OP>
constexpr bool leaf_convex() {
    return OP == RRTE_SDF_SPHERE || OP == RRTE_SDF_BOX || OP == RRTE_SDF_CYLINDER || OP == RRTE_SDF_PRISM ||
           OP == RRTE_SDF_CAPSULE;
}

// Is the postfix program a convex, 1-Lipschitz function of p?  Convex leaves (exact SDFs of convex
// solids -- the signed distance of a convex set is a supremum of affine functions -- and the prism's
// max of 1-Lipschitz convex terms) and intersections (max) of such; union, difference, smooth ops,
// the other leaves and every deformer are not.  Evaluated at compile time for the scene-specialised
// kernels (sdf_march CONVEX).
#ifndef RRTE_SECANT_EXIT
#define RRTE_SECANT_EXIT 2
#endif
constexpr int kSecantExit = RRTE_SECANT_EXIT;  // 0 off, 1 any-hit marches, 2 closest-hit marches too
constexpr bool sdf_convex(const rrte_sdf_node* n, uint32_t count) {
    bool st[RRTE_SDF_MAX_STACK] = {};
    uint32_t sp = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t op = n[i].op;
        if (op < 32u) {
            if (sp >= RRTE_SDF_MAX_STACK) return false;
            // (box, cylinder and capsule stay convex for any sizes: a degenerate one drops the
            // inside term; the cone formula is the exact SDF only for radius, height > 0)
            st[sp++] = op == RRTE_SDF_SPHERE || op == RRTE_SDF_BOX || op == RRTE_SDF_CYLINDER ||
                       op == RRTE_SDF_PRISM || op == RRTE_SDF_CAPSULE ||
                       (op == RRTE_SDF_CONE && n[i].f[3] > 0.0f && n[i].f[4] > 0.0f);
        } else if (op < 64u) {
            if (sp < 2u) return false;
            // max, and the smooth max -smin(-a, -b, k) = (a + b)/2 + phi(a - b) with phi(u) = k/4 + u^2/(4k)
            // for |u| <= k, |u|/2 beyond (convex, nondecreasing in a and b, 1-Lipschitz), k > 0
            const bool c = (op == RRTE_SDF_INTERSECTION || (op == RRTE_SDF_SMOOTH_INTERSECTION && n[i].f[0] > 0.0f)) &&
                           st[sp - 1] && st[sp - 2];
            sp -= 2;
            st[sp++] = c;
        } else {
            return false;  // deformers (and their point-stack pops)
        }
    }
    return sp == 1u && st[0];
}
// Scale of a program's leaves for sdf_march's error bound: max over leaves of |center|_1 + the sum
// of |size parameters| (an intersection's leaves may reach far outside the object's bound), plus
// every smooth op's |k|.
constexpr float sdf_leaf_scale(const rrte_sdf_node* n, uint32_t count) {
    float k = 0.0f, ks = 0.0f;
    for (uint32_t i = 0; i < count; ++i) {
        if (n[i].op >= 32u) {
            if (n[i].op < 64u) ks += n[i].f[0] < 0.0f ? -n[i].f[0] : n[i].f[0];
            continue;
        }
        float s = 0.0f;
        for (int j = 0; j < 7; ++j) s += n[i].f[j] < 0.0f ? -n[i].f[j] : n[i].f[j];
        k = s > k ? s : k;
    }
    return k + ks;
}

// Static program (scene-specialised kernel): nodes [FIRST, FIRST+COUNT) of a
// constexpr scene, unrolled at compile time; ops fold, stack slots become
// fixed registers.  A guarded operand [I, J) becomes a uniform branch around
// its straight-line code.
template <class S, uint32_t K>
constexpr TopoNode node_topo() {
    if constexpr (S::kTopo) return S::topo_nodes[K];
    else return TopoNode{S::nodes[K].op, {S::nodes[K].i[0], S::nodes[K].i[1], S::nodes[K].i[2]}};
}
template <class S, uint32_t FIRST, uint32_t I, uint32_t END, bool CHECK>
__device__ __forceinline__ void sdf_static_range(const S& sc, float* vs, f3* ps, uint32_t& sp, uint32_t& pp, f3& p) {
    if constexpr (I < END) {
        constexpr TopoNode tn = node_topo<S, FIRST + I>();
        constexpr uint32_t link = tn.i[2];
        if constexpr (CHECK && link != 0u) {
            constexpr uint32_t gop = node_topo<S, FIRST + link - 1u>().op;
            float r;
            bool taken;
            if constexpr (S::kTopo) {
                const NodeArgs na = load_uniform(reinterpret_cast<const NodeArgs*>(sc.nodes[FIRST + link - 1u].f));
                taken = sdf_guard(gop, na.f, vs[sp - 1], p, r);
            } else {
                constexpr rrte_sdf_node g = S::nodes[FIRST + link - 1u];
                taken = sdf_guard(gop, g.f, vs[sp - 1], p, r);
            }
            if (taken) vs[sp - 1] = r;
            else sdf_static_range<S, FIRST, I, link, false>(sc, vs, ps, sp, pp, p);
            sdf_static_range<S, FIRST, link, END, true>(sc, vs, ps, sp, pp, p);
        } else {
            if constexpr (S::kTopo) {
                const NodeArgs na = load_uniform(reinterpret_cast<const NodeArgs*>(sc.nodes[FIRST + I].f));
                sdf_node_step(tn.op, tn.i, na.f, vs, ps, sp, pp, p);
            } else {
                constexpr rrte_sdf_node n = S::nodes[FIRST + I];
                sdf_node_step(n.op, n.i, n.f, vs, ps, sp, pp, p);
            }
            sdf_static_range<S, FIRST, I + 1u, END, true>(sc, vs, ps, sp, pp, p);
        }
    }
}

template <class S, uint32_t FIRST, uint32_t COUNT>
struct SdfStaticProgram {
    const S& sc;
    static constexpr bool kSmall = COUNT <= 8u;
    // the secant exit's leaf scale (sdf_leaf_scale): folded for a full scene, the host's value in the
    // program's first node's spare slot f[11] for a topology scene (rrte_hip.hip upload_scene)
    __device__ __forceinline__ float leaf_scale() const {
        if constexpr (S::kTopo) {
            return load_uniform(reinterpret_cast<const NodeArgs*>(sc.nodes[FIRST].f)).f[11];
        } else {
            constexpr float k = sdf_leaf_scale(S::nodes + FIRST, COUNT);
            return k;
        }
    }
    __device__ __forceinline__ float operator()(f3 p) const {
        float vs[RRTE_SDF_MAX_STACK];
        f3 ps[RRTE_SDF_MAX_POINT_STACK];
        uint32_t sp = 0, pp = 0;
        sdf_static_range<S, FIRST, 0u, COUNT, true>(sc, vs, ps, sp, pp, p);
        return vs[0];
    }
};

}  // namespace rrte
