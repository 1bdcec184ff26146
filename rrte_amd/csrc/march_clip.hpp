// march_clip.hpp — skip and shorten the sphere-tracing marches of two-sphere CSG objects.
//
// An SDF object marches between the two points where the ray crosses its bounding sphere.  For a program
// of two sphere leaves under one CSG operator that sphere is loose (renderer.py CSGComposite.bound grows
// it by the whole k, and a union's spans both parts), so many rays cross it, graze past the surface with
// ever smaller steps and miss.  Below, the ray is first tested against an enclosure of everything a march
// can report as a hit: a ray that misses it is answered "miss" without marching, and the others stop
// where they leave it.  The start of a march never moves, so the step sequence up to a hit -- and the
// hit's t -- stay bit for bit; frames and shadow counts are what they were.
//
// THE HIT REGION.  sdf_march (intersect.hpp) reports a hit only at a step with d~ < fl(eps t), t <= tend,
// where d~ is the computed value of the program f at the computed point.  As the secant exit's argument
// has it, d~ >= f(o + t d) - D with D = 2^-17 (|o|_1 + tend + |cb|_1 + 4 R + K) ((cb, R) the bounding
// sphere, K = sdf_leaf_scale), and fl(eps t) <= E t with E = eps (1 + 2^-20), for eps >= 0 and t >= 0 (a
// negative t has fl(eps t) <= 0).  So a hit point lies in Hreg = { p : f(p) <= L } for any
// L >= E T + D(T), T >= tend.
//
// ENCLOSURES of Hreg, with a = |p - ca| - ra and b = |p - cb| - rb the leaves and S_x(rho) the ball
// around cx, from the operators as sdf_node_step computes them (real arithmetic: their rounding is in D):
//   union         min(a, b) <= L                        ->  S_a(ra + L) u S_b(rb + L)
//   smooth union  smin(a, b, k) = min(a, b) - k (1 - h')^2 with h' = max(h, 1 - h) in [1/2, 1], so
//                 smin >= min(a, b) - k/4               ->  S_a(ra + k/4 + L) u S_b(rb + k/4 + L)
//   difference    max(a, -b) >= a                       ->  S_a(ra + L)
//   smooth diff.  -smin(-a, b, k) >= -min(-a, b) = max(a, -b) >= a (smin <= min, above)  ->  S_a(ra + L)
//   intersection  max(a, b) <= L                        ->  S_a(ra + L) n S_b(rb + L)
//   smooth int.   -smin(-a, -b, k) >= max(a, b)         ->  the same
//
// SKIP AND END CLIP.  Along the ray the enclosure is an interval, or two for a union.  Let t_exit be the
// last parameter inside it (a union: the larger of the parts' exits, a part the ray's line misses having
// none; an intersection: the smaller).  Every march point with t > t_exit lies outside Hreg: it cannot
// hit, its d~ >= f - D > L - D >= E T >= 0 is positive, and with step_scale > 0 the following t only grow,
// so no later step comes back.  The unclipped march therefore ends in a miss, at tend or at max_steps,
// once it has passed t_exit, and "miss" is what the march clipped to min(tend, t_exit) answers at its
// first step past t_exit; before that the two marches are the same steps.  If the ray's line misses the
// enclosure, or t_exit < t_min (every march point has t >= t_min), no step can hit: miss, without marching.
// The clip is handed to the unchanged sdf_march as its t_max: tend = mn(t_max', -b + sq) is then
// min(tend, t_exit), and there is one march loop, not two.  A convex march (an intersection) thereby runs
// its secant exit on the clipped interval, which is sdf_march's own proof for the arguments it is given:
// it answers what the plain loop on [t, min(tend, t_exit)] answers, which is what the plain loop on
// [t, tend] answers.
//
// THE TEST IS CONSERVATIVE ARITHMETIC, not the reference's: one approximate v_sqrt_f32, no divide.  With
// u = 2^-24, oc = o - c, b~ = fl(oc.d), q~ = fl(oc.oc), and |d|^2 within 2^-20 of 1 (checked: a ray
// whose direction is no unit vector takes the template unchanged):
//   * T = 1.001 |b~| + 2^-8 |o|_1 + Kt bounds tend.  tend <= fl(-bB + sqB) of the bound test, whose disc
//     is <= 1.001 R^2 + 2^-18 |o - cb|^2 (|bB| <= |d| |o - cb| and 40 u of rounding), so sqB <= 1.001 R +
//     2^-9 |o - cb|; |bB| <= |b~| + 1.001 |c - cb| + 5u (|o|_1 + |c|_1); Kt = 1.002 (|c - cb|_1 + R) +
//     2^-8 (|cb|_1 + |c|_1) is a constant of the object.
//   * rho = C0 + C1 |b~| + C2 |o|_1 is the part's radius r (+ k/4) + E T + D(T), every constant grown by
//     1 + 2^-10: that covers the three roundings of rho, those of the constants, and rho^2 >= |d|^2 rho0^2.
//   * the true disc b^2 - |d|^2 (q - rho0^2) is <= dc + 40 u (q + rho^2), dc = fl(b~^2 - fl(q~ - rho^2))
//     (9u q from b~, 21u q from |d|^2 and q~, 4u (q + rho^2) from the three operations), so
//     du = dc + 2^-18 (q~ + rho^2) < 0 proves that the line misses the ball.
//   * the true exit (-b + sqrt(disc)) / |d|^2 is <= fl(s - b~) + 2^-17 (|b~| + s + rho), s = v_sqrt(du)
//     (1 ulp): 4.3u (|b~| + rho) for b~ (|oc| <= |b| + rho once du >= 0), 3u s for the root, 2^-19 (|b| + s)
//     for |d|^2, u (|b~| + s) for the subtraction -- under 2^-18 (|b~| + s + rho) together.
// A ray that starts inside a part (self-shadow, a camera inside the bound) has a negative entry, which
// is never used: only the exit and the miss are.  A light inside the bound is a small t_max, which
// min(t_max, t_exit) keeps.  NaN: every decision below is a compare that NaN fails, so a NaN in the
// origin, the direction, t_min, t_max or the test's own arithmetic skips nothing and leaves t_max as it
// was; clip::info stands down at compile time (cls = 0) for a program that is not exactly "sphere,
// sphere, CSG op" without guards, for a negative or non-finite radius, centre, eps or bound, a step
// scale that is not positive, and a smooth operator whose k is not positive and finite.
//
// Not in the Makefile's DEVICE_HDR, so rrte_hip_build_id stays where it was: the Makefile embeds this file as a string
// of its own (march_clip.inc) and jit.hip's jit_source pastes it into the generated source after the
// definition of rrte_jit::Scene, which the overloads below name; the code-object cache key hashes
// that source.  Only FULL kernels clip: a topology kernel reads radii and centres at run time, where
// these constants would cost registers and scalar loads, and keeps the templates.
// -DRRTE_MARCH_CLIP=0 (RRTE_JIT_EXTRA_OPTS) compiles none of this: the templates' instruction stream.
// The value is a mask of operator classes (A/B): 1 (smooth) difference, 2 (smooth) intersection,
// 4 (smooth) union.
#ifndef RRTE_MARCH_CLIP
#define RRTE_MARCH_CLIP 7
#endif  // RRTE_MARCH_CLIP default
#if RRTE_MARCH_CLIP
namespace rrte {  // (clip constants)
namespace clip {  // the enclosure of one object: constants, host and device (include/rrte_hip_clip.h exports them)

constexpr uint32_t kDifference = 1u, kIntersection = 2u, kUnion = 4u;
// One part sphere: centre, and C0 of rho = C0 + C1 |b~| + C2 |o|_1.
struct Part { float c[3]; float c0; };
struct Info { uint32_t cls; float c1, c2; Part a, b; };  // cls 0: no clip (the template answers)

constexpr bool bounded(float x) { return x > -0x1p40f && x < 0x1p40f; }  // (NaN is not)
constexpr float mag(float x) { return x < 0.0f ? -x : x; }
constexpr float l1(const float* v) { return (mag(v[0]) + mag(v[1])) + mag(v[2]); }

constexpr Info info(const DPrim& pr, const rrte_sdf_node* nodes) {
    const Info none{};
    if (pr.kind != RRTE_PRIM_SDF || pr.sdf_count != 3u) return none;
    const rrte_sdf_node& A = nodes[pr.sdf_first];
    const rrte_sdf_node& B = nodes[pr.sdf_first + 1u];
    const rrte_sdf_node& O = nodes[pr.sdf_first + 2u];
    if (A.op != RRTE_SDF_SPHERE || B.op != RRTE_SDF_SPHERE || O.op < RRTE_SDF_UNION || O.op > RRTE_SDF_SMOOTH_INTERSECTION)
        return none;
    if (A.i[2] != 0u || B.i[2] != 0u || O.i[2] != 0u) return none;  // (a guarded operand: not this shape)
    for (int j = 0; j < 7; ++j)
        if (!bounded(A.f[j]) || !bounded(B.f[j])) return none;
    for (int j = 0; j < 4; ++j)
        if (!bounded(pr.p[j])) return none;
    const bool smooth = O.op >= RRTE_SDF_SMOOTH_UNION;
    const float k = smooth ? O.f[0] : 0.0f;
    if (!bounded(O.f[0]) || (smooth && !(k > 0.0f))) return none;
    const float eps = pr.sdf_hit_eps, R = pr.p[3];
    if (!(A.f[3] >= 0.0f && B.f[3] >= 0.0f && R >= 0.0f && eps >= 0.0f && bounded(eps))) return none;
    if (!(pr.sdf_step_scale > 0.0f && bounded(pr.sdf_step_scale))) return none;
    const bool uni = O.op == RRTE_SDF_UNION || O.op == RRTE_SDF_SMOOTH_UNION;
    const bool dif = O.op == RRTE_SDF_DIFFERENCE || O.op == RRTE_SDF_SMOOTH_DIFFERENCE;
    Info r{};
    r.cls = uni ? kUnion : dif ? kDifference : kIntersection;
    constexpr float grow = 1.0f + 0x1p-10f;
    const float EE = eps * (1.0f + 0x1p-20f) + 0x1p-17f;  // E T + D(T) = EE T + 2^-17 (|o|_1 + |cb|_1 + 4 R + K)
    float sa = 0.0f, sb = 0.0f;                           // K as sdf_leaf_scale has it
    for (int j = 0; j < 7; ++j) {
        sa += mag(A.f[j]);
        sb += mag(B.f[j]);
    }
    const float K = (sa > sb ? sa : sb) + mag(O.f[0]);  // (the op's f[0] counts for a plain op too)
    const float dconst = 0x1p-17f * ((l1(pr.p) + 4.0f * R) + K);
    r.c1 = EE * 1.001f * grow;
    r.c2 = (0x1p-17f + EE * 0x1p-8f) * grow;
    const rrte_sdf_node* leaf[2] = {&A, &B};
    Part* part[2] = {&r.a, &r.b};
    for (int s = 0; s < 2; ++s) {
        const float* f = leaf[s]->f;
        const float off = (mag(f[0] - pr.p[0]) + mag(f[1] - pr.p[1])) + mag(f[2] - pr.p[2]);
        const float kt = 1.002f * (off + R) + 0x1p-8f * (l1(pr.p) + l1(f));
        for (int j = 0; j < 3; ++j) part[s]->c[j] = f[j];
        part[s]->c0 = (((f[3] + (uni ? 0.25f * k : 0.0f)) + EE * kt) + dconst) * grow;
    }
    return r;
}

}  // namespace clip
}  // namespace rrte (clip constants)

#ifndef RRTE_MARCH_CLIP_HOST
namespace rrte {  // (march clip)
namespace clip {  // the device test

template <class S, uint32_t I>
constexpr Info info_of() {
    if constexpr (S::kTopo) return Info{};
    else return info(S::prims[I], S::nodes);
}

// One part's ball against the ray: does the ray's line miss it, and an upper bound of the exit parameter
// (NaN when the arithmetic has none to give).  o1 = |o|_1.
template <class S, uint32_t I, bool SECOND>
__device__ __forceinline__ void part_exit(const Ray& r, float o1, bool& miss, float& exit) {
    constexpr Info ci = info_of<S, I>();
    constexpr Part pt = SECOND ? ci.b : ci.a;
    const f3 oc = vsub(r.o, V(pt.c[0], pt.c[1], pt.c[2]));
    const float b = vdot(oc, r.d);
    const float q = vdot(oc, oc);
    const float rho = (pt.c0 + ci.c1 * fabsf(b)) + ci.c2 * o1;
    const float rr = rho * rho;
    const float du = (b * b - (q - rr)) + 0x1p-18f * (q + rr);
    miss = du < 0.0f;
    const float s = __builtin_amdgcn_sqrtf(du);
    exit = (s - b) + 0x1p-17f * ((fabsf(b) + s) + rho);
}

// false: no step of the march can hit.  Otherwise t_max is the march's end, clipped where that is proven.
template <class S, uint32_t I>
__device__ __forceinline__ bool reach(const Ray& r, float t_min, float& t_max) {
    constexpr Info ci = info_of<S, I>();
    const bool unit = fabsf(vdot(r.d, r.d) - 1.0f) <= 0x1p-20f;
    const float o1 = (fabsf(r.o.x) + fabsf(r.o.y)) + fabsf(r.o.z);
    bool ma, mb = false;
    float ea, eb, ex;
    part_exit<S, I, false>(r, o1, ma, ea);
    if constexpr (ci.cls == kDifference) {
        ex = ea;
    } else {
        part_exit<S, I, true>(r, o1, mb, eb);
        if constexpr (ci.cls == kIntersection) {
            ex = mn(ea, eb);  // (a NaN in either leaves the other or NaN: each part alone encloses)
            ma = ma || mb;
        } else {
            const float both = (eb == eb) ? mx(ea, eb) : eb;  // the later exit; NaN if either is
            ex = ma ? eb : mb ? ea : both;
            ma = ma && mb;
        }
    }
    if (unit && (ma || ex < t_min)) return false;
    t_max = (unit && ex < t_max) ? ex : t_max;
    return true;
}

}  // namespace clip

// intersect_at / any_hit_at of search.hpp for the specialised scene: a clip-able object's march is
// skipped or given its clipped end, everything else is the template's.
template <bool NEED_HIT, uint32_t I, bool ANY = false>
__device__ __forceinline__ bool intersect_at(const rrte_jit::Scene& sc, UC<I> ii, const Ray& r, float t_min, float t_max,
                                             Hit& out) {
    constexpr uint32_t cls = clip::info_of<rrte_jit::Scene, I>().cls;
    if constexpr ((cls & (uint32_t)(RRTE_MARCH_CLIP)) != 0u) {
        if (!clip::reach<rrte_jit::Scene, I>(r, t_min, t_max)) return false;
    }
    return intersect_at<NEED_HIT, rrte_jit::Scene, I, ANY>(sc, ii, r, t_min, t_max, out);
}
template <uint32_t I>
__device__ __forceinline__ bool any_hit_at(const rrte_jit::Scene& sc, UC<I> ii, const Ray& r, float t_min, float t_max,
                                           Hit& h) {
    return intersect_at<false, I, true>(sc, ii, r, t_min, t_max, h);
}

}  // namespace rrte (march clip)
#endif  // RRTE_MARCH_CLIP_HOST
#endif  // RRTE_MARCH_CLIP
