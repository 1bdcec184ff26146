// intersect.hpp — one ray against one object that is no mesh.
//
// The sphere-tracing march of an SDF object inside its bounding sphere (leaves_sphere, sdf_march, with
// the convex secant early miss), its hit attributes (sdf_hit_attributes), the seven analytic
// intersectors in object space (local_ray; sphere, plane, triangle, cube, cylinder, cone, capsule) and
// isect_sdf.  Operation order mirrors the reference (file:line cited per function).
//
// Includes sdf_eval.hpp.  Included by search.hpp.  Embedded for hiprtc (the Makefile's DEVICE_HDR).
#pragma once

#include "sdf_eval.hpp"

namespace rrte {

// Exact "ray leaves the sphere" early-out for any-hit (shadow) rays: origin outside the sphere
// (cc = |oc|^2 - r^2 > 0) not approaching its centre (0 <= hb = oc.d < 2^63), |d|^2 >= 1/4,
// t_min >= 2^-57.  Then the full test finds nothing in [t_min, t_max].  hb < 2^63 keeps RN(hb^2)
// finite, and a cc is a product of two positive numbers, so it is positive, +0 or +inf, never NaN:
// disc = RN(RN(hb^2) - RN(a cc)) is a number, <= RN(hb^2), and -inf (a miss) when a cc overflows.
// Otherwise sq = RN(sqrt(disc)) <= RN(sqrt(RN(hb^2))), which is hb when hb >= 2^-60
// (fl(sqrt(fl(x*x))) = |x| in binary f32 with round-to-nearest while x*x neither overflows nor
// underflows) and <= 2^-60 otherwise (hb = 0 included); hence -hb + sq <= 2^-60, both roots
// (-hb -/+ sq)/a are <= 2^-58 < t_min (a = +inf gives -0), and the sphere / bounding-sphere test
// rejects.  From hb = 2^64 on RN(hb^2) = +inf: with a cc = +inf as well disc is NaN, every comparison
// of the full test fails and the reference reports a hit with t = NaN -- so the early-out stands down
// there and the full test answers.  The range of hb is ONE unsigned compare on its bit pattern,
// bits(hb) < bits(2^63) = 0x5F000000: a negative hb, -0 and NaN all have larger patterns (and go to
// the full test), so the bound costs no instruction over the "hb > 0" it replaces.
// Skips the sqrt and divides of, e.g., every shadow ray's test against the ground sphere.
__device__ __forceinline__ bool leaves_sphere(float hb, float cc, float a, float t_min) {
    return __float_as_uint(hb) < 0x5F000000u && cc > 0.0f && a >= 0.25f && t_min >= 0x1p-57f;
}

// SDFObject::intersect, search part -- sphere tracing inside the object's
// bounding sphere (build-defined).  Only t is produced here;
// the closest-hit search keeps (t, object) and the hit attributes are
// computed once for the winner.  The per-lane trip count diverges; the wave
// leaves the loop when its EXEC mask drains.
//
// CONVEX (marches of objects whose SDF program is a convex, 1-Lipschitz function of p: a convex leaf
// or an intersection of such, no deformers; sdf_convex) adds an exact early miss.  Along
// the ray, f(t) = sdf(o + t d) is convex, so for t >= t_k it lies above the secant through the last
// two march points: f(t) >= f(t_k) + s (t - t_k), s = (f(t_k) - f(t_k-1)) / (t_k - t_k-1).  Every
// computed value d~ is within D of f at the exact point: D = 2^-17 (|o|_1 + tend + |c|_1 + 4 R + K),
// K = sdf_leaf_scale (the largest leaf's |center|_1 + |sizes|).  The rounding of p = o + t d moves
// p by <= 2^-24 (|o|_1 + 2t), which f (1-Lipschitz) passes on unchanged, and each leaf's evaluation
// errs by <= 24 * 2^-24 (|q| + sizes), the cone's being the longest (its clamped projection
// parameter's error times the side length stays <= 8 * 2^-24 (|q| + h)), a smooth max adds
// <= 6 * 2^-24 (|a| + |b| + k) and passes its operands' errors on unscaled; together <= 64 * 2^-24
// (...) against 2^-17 = 128 * 2^-24.  Hence if d~_k - E t_k >= 3D and (d~_k - d~_k-1) - E (t_k - t_k-1) >= 3D with
// E = eps (1 + 2^-20) >= fl(eps t) / t, every later step has d~ >= f - D >= E t >= fl(eps t): no
// later step can hit, and the march's answer is "miss" whether it ends at tend or at max_steps.  A
// NaN anywhere fails both tests.  Shadow rays leaving the object they start on exit after ~3 steps
// instead of marching out of the bound; camera and shadow rays that pass an object exit once they
// recede from it.  (A miss's t is never used, so closest-hit marches take it too.)
template <class EVAL, bool ANY = false, bool CONVEX = false>
__device__ __forceinline__ bool sdf_march(const DPrim& pr, const EVAL& eval, const Ray& r, float t_min, float t_max,
                                          float& t_hit) {
    f3 bc = V(pr.p[0], pr.p[1], pr.p[2]);
    float br = pr.p[3];
    f3 oc = vsub(r.o, bc);
    float b = vdot(oc, r.d);
    float cc = vdot(oc, oc) - br * br;
    // the bound test below has no divide (roots -b -/+ sq): leaves_sphere's argument with a = 1, which
    // leaves tend = mn(t_max, -b + sq) <= 2^-60 < t_min <= t unless t_max is NaN (tend NaN marches on)
    if (ANY && t_max == t_max && leaves_sphere(b, cc, 1.0f, t_min)) return false;
    float disc = b * b - cc;
    if (disc < 0.0f) return false;
    float sq = sqrt_rn(disc);
    float t = mx(t_min, -b - sq);
    float tend = mn(t_max, -b + sq);
    if (t > tend) return false;
    const float eps = pr.sdf_hit_eps, scale = pr.sdf_step_scale;
    const uint32_t steps = pr.sdf_max_steps;
    // One divergent exit per step (hit, or the next t leaves the bound) instead of three: same
    // t sequence and result as "if (d < eps*t) hit; t += d*scale; if (t > tend) miss" (NaN
    // included).  (A fully predicated form with a wave-uniform exit was measured slower.)
    bool hit = false;
    if constexpr (CONVEX) {
        const float E = eps * (1.0f + 0x1p-20f);
        const float K = eval.leaf_scale();
        const float D3 = 3.0f * 0x1p-17f *
                         ((((fabsf(r.o.x) + fabsf(r.o.y)) + fabsf(r.o.z)) + tend) +
                          ((((fabsf(bc.x) + fabsf(bc.y)) + fabsf(bc.z)) + 4.0f * br) + K));
        float dp = __builtin_nanf(""), tp = t;
#pragma unroll 1
        for (uint32_t i = 0; i < steps; ++i) {
            f3 p = ray_at(r, t);
            float d = eval(p);
            hit = d < eps * t;
            const float tn = t + d * scale;
            const bool safe = (d - E * t >= D3) && ((d - dp) - E * (t - tp) >= D3);
            const bool stop = hit || tn > tend || safe;
            dp = d;
            tp = t;
            t = hit ? t : tn;
            if (stop) break;
        }
        t_hit = t;
        return hit;
    }
#pragma unroll 1
    for (uint32_t i = 0; i < steps; ++i) {
        f3 p = ray_at(r, t);
        float d = eval(p);
        hit = d < eps * t;
        const float tn = t + d * scale;
        const bool stop = hit || tn > tend;
        t = hit ? t : tn;
        if (stop) break;
    }
    t_hit = t;
    return hit;
}

// Hit attributes of an SDF hit at t: p = Ray::at(t) and the tetrahedral
// normal n = sum_k k_i f(p + k_i h), h = 1e-3, accumulated in the oracle's
// order: k0=(+,-,-) k1=(-,-,+) k2=(-,+,-) k3=(+,+,+).  One evaluation site.
template <class EVAL>
__device__ __forceinline__ void sdf_hit_attributes(const EVAL& eval, const Ray& r, float t, Hit& out) {
    const float h = 1e-3f;
    const f3 p = ray_at(r, t);
    auto taps = [&] {  // (a lambda of its own: written straight into this function the loop compiles differently)
        f3 n = V(0.0f, 0.0f, 0.0f);
        auto tap = [&](uint32_t k) {
            bool sx = (k == 0) || (k == 3), sy = (k >= 2), sz = (k == 1) || (k == 3);
            f3 q = V(sx ? p.x + h : p.x - h, sy ? p.y + h : p.y - h, sz ? p.z + h : p.z - h);
            float d = eval(q);
            if (k == 0) { n.x = d; n.y = -d; n.z = -d; }
            else if (k == 1) { n.x = n.x - d; n.y = n.y - d; n.z = n.z + d; }
            else if (k == 2) { n.x = n.x - d; n.y = n.y + d; n.z = n.z - d; }
            else { n.x = n.x + d; n.y = n.y + d; n.z = n.z + d; }
        };
        if constexpr (EVAL::kSmall) {
            // short programs (scene-specialised, <= 8 nodes): four straight-line taps, no per-tap selects
            // or loop control (-1.3 % per headline frame; long programs keep the loop for code size)
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) tap(k);
        } else {
#pragma unroll 1
            for (uint32_t k = 0; k < 4; ++k) tap(k);
        }
        return n;
    };
    const f3 n = taps();
    hit_new(out, t, p, vnorm(n), r);
}

// ----------------------------------------------------- analytic intersectors
__device__ __forceinline__ void local_ray(const DPrim& pr, const Ray& r, Ray& lr) {
    // inverse_matrix() applied to the ray, then Ray::new (primitives.rs:303-307)
    lr = ray_new(m_point(pr.inv, r.o), vnorm(m_vector(pr.inv, r.d)));
}

// SceneObject::intersect for the seven primitive kinds (primitives.rs:57-725).
// t is always written to out.t; point/normal only matter when NEED_HIT.
template <bool NEED_HIT, bool ANY = false>
__device__ __forceinline__ bool isect_sphere(const DPrim& pr, const Ray& r, float t_min, float t_max, Hit& out) {  // primitives.rs:57-81
    f3 ctr = V(pr.p[0], pr.p[1], pr.p[2]);
    float rad = pr.p[3];
    f3 oc = vsub(r.o, ctr);
    float a = vlen2(r.d);
    float hb = vdot(oc, r.d);
    float cc = vlen2(oc) - rad * rad;
    if (ANY && leaves_sphere(hb, cc, a, t_min)) return false;
    float disc = hb * hb - a * cc;
    if (disc < 0.0f) return false;
    float sq = sqrt_rn(disc);
    float root = (-hb - sq) / a;
    if (root < t_min || t_max < root) {
        root = (-hb + sq) / a;
        if (root < t_min || t_max < root) return false;
    }
    f3 p = ray_at(r, root);
    hit_new(out, root, p, vdivs(vsub(p, ctr), rad), r);
    return true;
}

// Hit attributes of a sphere hit found by the search at t (= the root isect_sphere returns for the same
// ray with t_max = INFINITY): the point and normal exactly as isect_sphere builds them, without
// solving the quadratic again.
__device__ __forceinline__ void sphere_attributes(const DPrim& pr, const Ray& r, float t, Hit& out) {
    const f3 ctr = V(pr.p[0], pr.p[1], pr.p[2]);
    const f3 p = ray_at(r, t);
    hit_new(out, t, p, vdivs(vsub(p, ctr), pr.p[3]), r);
}

template <bool NEED_HIT>
__device__ __forceinline__ bool isect_plane(const DPrim& pr, const Ray& r, float t_min, float t_max, Hit& out) {  // primitives.rs:133-149
    f3 pt = V(pr.p[0], pr.p[1], pr.p[2]), n = V(pr.p[4], pr.p[5], pr.p[6]);
    float denom = vdot(n, r.d);
    if (fabsf(denom) < 1e-6f) return false;
    float t = vdot(vsub(pt, r.o), n) / denom;
    if (t < t_min || t > t_max) return false;
    f3 p = ray_at(r, t);
    hit_new(out, t, p, denom < 0.0f ? n : vneg(n), r);
    return true;
}

template <bool NEED_HIT>
__device__ __forceinline__ bool isect_triangle(const DPrim& pr, const Ray& r, float t_min, float t_max, Hit& out) {  // primitives.rs:208-244
    f3 v0 = V(pr.p[0], pr.p[1], pr.p[2]), v1 = V(pr.p[3], pr.p[4], pr.p[5]), v2 = V(pr.p[6], pr.p[7], pr.p[8]);
    f3 e1 = vsub(v1, v0), e2 = vsub(v2, v0);
    f3 h = vcross(r.d, e2);
    float a = vdot(e1, h);
    if (a > -1e-6f && a < 1e-6f) return false;
    float f = rcp_rn(a);
    f3 s = vsub(r.o, v0);
    float u = f * vdot(s, h);
    if (u < 0.0f || u > 1.0f) return false;
    f3 q = vcross(s, e1);
    float v = f * vdot(r.d, q);
    if (v < 0.0f || u + v > 1.0f) return false;
    float t = f * vdot(e2, q);
    if (t < t_min || t > t_max) return false;
    f3 p = ray_at(r, t);
    float w = 1.0f - u - v;
    f3 n0 = V(pr.p[9], pr.p[10], pr.p[11]), n1 = V(pr.p[12], pr.p[13], pr.p[14]),
       n2 = V(pr.p[15], pr.p[16], pr.p[17]);
    f3 n = vnorm(vadd(vadd(vmuls(n0, w), vmuls(n1, u)), vmuls(n2, v)));
    hit_new(out, t, p, n, r);
    return true;
}

template <bool NEED_HIT>
__device__ __forceinline__ bool isect_cube(const DPrim& pr, const Ray& r, float t_min, float t_max, Hit& out) {  // primitives.rs:301-364
    Ray lr;
    local_ray(pr, r, lr);
    f3 ctr = V(pr.p[0], pr.p[1], pr.p[2]), size = V(pr.p[4], pr.p[5], pr.p[6]);
    f3 half = vmuls(size, 0.5f);
    f3 mnb = vsub(ctr, half), mxb = vadd(ctr, half);
    float t_near = t_min, t_far = t_max;
    f3 normal = V(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (uint32_t i = 0; i < 3; ++i) {
        f3 axis = setcomp(V(0.0f, 0.0f, 0.0f), i, 1.0f);
        float oc = vdot(lr.o, axis), dc = vdot(lr.d, axis);
        float lo = vdot(mnb, axis), hi = vdot(mxb, axis);
        if (fabsf(dc) < 1e-6f) {
            if (oc < lo || oc > hi) return false;
        } else {
            float t1 = (lo - oc) / dc, t2 = (hi - oc) / dc;
            float tsn = t1 < t2 ? t1 : t2, tsf = t1 < t2 ? t2 : t1;
            if (tsn > t_near) {
                t_near = tsn;
                normal = t1 < t2 ? vneg(axis) : axis;
            }
            if (tsf < t_far) t_far = tsf;
            if (t_near > t_far) return false;
        }
    }
    float t = (t_near >= t_min) ? t_near : t_far;
    if (t < t_min || t > t_max) return false;
    f3 lp = ray_at(lr, t);
    hit_new(out, t, m_point(pr.xf, lp), vnorm(m_vector(pr.xf, normal)), r);
    return true;
}

template <bool NEED_HIT>
__device__ __forceinline__ bool isect_cylinder(const DPrim& pr, const Ray& r, float t_min, float t_max, Hit& out) {  // primitives.rs:419-465
    Ray lr;
    local_ray(pr, r, lr);
    f3 ctr = V(pr.p[0], pr.p[1], pr.p[2]);
    float rad = pr.p[3], hh = pr.p[4] * 0.5f;
    f3 oc = vsub(lr.o, ctr);
    float a = lr.d.x * lr.d.x + lr.d.z * lr.d.z;
    float b = 2.0f * (oc.x * lr.d.x + oc.z * lr.d.z);
    float cc = oc.x * oc.x + oc.z * oc.z - rad * rad;
    float disc = b * b - 4.0f * a * cc;
    if (disc < 0.0f) return false;
    float sq = sqrt_rn(disc);
    float ts0 = (-b - sq) / (2.0f * a), ts1 = (-b + sq) / (2.0f * a);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float t = k == 0 ? ts0 : ts1;
        if (t >= t_min && t <= t_max) {
            f3 p = ray_at(lr, t);
            if (fabsf(p.y - ctr.y) <= hh) {
                f3 ln = V((p.x - ctr.x) / rad, 0.0f, (p.z - ctr.z) / rad);
                hit_new(out, t, m_point(pr.xf, p), vnorm(m_vector(pr.xf, ln)), r);
                return true;
            }
        }
    }
    return false;
}

template <bool NEED_HIT>
__device__ __forceinline__ bool isect_cone(const DPrim& pr, const Ray& r, float t_min, float t_max, Hit& out) {  // primitives.rs:520-571
    Ray lr;
    local_ray(pr, r, lr);
    f3 ctr = V(pr.p[0], pr.p[1], pr.p[2]);
    float rad = pr.p[3], ht = pr.p[4], hh = ht * 0.5f;
    f3 oc = vsub(lr.o, ctr);
    float k = rad / ht, k2 = k * k;
    f3 d = lr.d;
    float a = d.x * d.x + d.z * d.z - k2 * d.y * d.y;
    float b = 2.0f * (oc.x * d.x + oc.z * d.z - k2 * (oc.y - hh) * d.y);
    float cc = oc.x * oc.x + oc.z * oc.z - k2 * (oc.y - hh) * (oc.y - hh);
    float disc = b * b - 4.0f * a * cc;
    if (disc < 0.0f) return false;
    float sq = sqrt_rn(disc);
    float ts0 = (-b - sq) / (2.0f * a), ts1 = (-b + sq) / (2.0f * a);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        float t = kk == 0 ? ts0 : ts1;
        if (t >= t_min && t <= t_max) {
            f3 p = ray_at(lr, t);
            float yl = p.y - ctr.y;
            if (yl >= -hh && yl <= hh) {
                float rr = sqrt_rn(p.x * p.x + p.z * p.z);
                f3 ln = vnorm(V(p.x / rr, k, p.z / rr));
                hit_new(out, t, m_point(pr.xf, p), vnorm(m_vector(pr.xf, ln)), r);
                return true;
            }
        }
    }
    return false;
}

template <bool NEED_HIT>
__device__ __forceinline__ bool isect_capsule(const DPrim& pr, const Ray& r, float t_min, float t_max, Hit& out) {  // primitives.rs:626-725
    Ray lr;
    local_ray(pr, r, lr);
    f3 ctr = V(pr.p[0], pr.p[1], pr.p[2]);
    float rad = pr.p[3], hh = pr.p[4] * 0.5f;
    float closest = kInf;
    bool found = false;
    float a = vlen2(lr.d);
#pragma unroll
    for (int cap = 0; cap < 2; ++cap) {
        f3 cc_ = cap == 0 ? vadd(ctr, V(0.0f, hh, 0.0f)) : vsub(ctr, V(0.0f, hh, 0.0f));
        f3 oc = vsub(lr.o, cc_);
        float hb = vdot(oc, lr.d);
        float cc = vlen2(oc) - rad * rad;
        float disc = hb * hb - a * cc;
        if (disc >= 0.0f) {
            float sq = sqrt_rn(disc);
            float ts0 = (-hb - sq) / a, ts1 = (-hb + sq) / a;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                float t = k == 0 ? ts0 : ts1;
                if (t >= t_min && t <= t_max && t < closest) {
                    f3 p = ray_at(lr, t);
                    bool ok = cap == 0 ? (p.y >= ctr.y) : (p.y <= ctr.y);
                    if (ok) {
                        f3 ln = vnorm(vsub(p, cc_));
                        closest = t;
                        hit_new(out, t, m_point(pr.xf, p), vnorm(m_vector(pr.xf, ln)), r);
                        found = true;
                    }
                }
            }
        }
    }
    f3 oc = vsub(lr.o, ctr);
    float ac = lr.d.x * lr.d.x + lr.d.z * lr.d.z;
    float bc = 2.0f * (oc.x * lr.d.x + oc.z * lr.d.z);
    float ccy = oc.x * oc.x + oc.z * oc.z - rad * rad;
    float disc = bc * bc - 4.0f * ac * ccy;
    if (disc >= 0.0f) {
        float sq = sqrt_rn(disc);
        float ts0 = (-bc - sq) / (2.0f * ac), ts1 = (-bc + sq) / (2.0f * ac);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            float t = k == 0 ? ts0 : ts1;
            if (t >= t_min && t <= t_max && t < closest) {
                f3 p = ray_at(lr, t);
                if (fabsf(p.y - ctr.y) <= hh) {
                    f3 ln = V((p.x - ctr.x) / rad, 0.0f, (p.z - ctr.z) / rad);
                    closest = t;
                    hit_new(out, t, m_point(pr.xf, p), vnorm(m_vector(pr.xf, ln)), r);
                    found = true;
                }
            }
        }
    }
    return found;
}

template <bool NEED_HIT, class EVAL, bool ANY = false, bool CONVEX = false>
__device__ __forceinline__ bool isect_sdf(const DPrim& pr, const EVAL& eval, const Ray& r, float t_min, float t_max,
                                          Hit& out) {
    float t;
    if (!sdf_march<EVAL, ANY, CONVEX>(pr, eval, r, t_min, t_max, t)) return false;
    if (NEED_HIT) sdf_hit_attributes(eval, r, t, out);
    else out.t = t;
    return true;
}

}  // namespace rrte
