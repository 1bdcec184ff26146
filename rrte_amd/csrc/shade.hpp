// shade.hpp — the colour of a ray.
//
// Lights (Contrib, illuminate), materials (scatter), the camera ray (generate_ray), material_of, the
// REFCOMPAT path loop (PathState, path_begin / path_step, ray_color_ref), the launch traits
// (LaunchAny / LaunchPlain, launch_debug) and the LAMBERT_SHADOW shader (shade_lambert).
//
// Includes search.hpp and cull.hpp.  Included by ray_kernels.hpp and ray_query.hpp (generate_ray).
// Embedded for hiprtc (the Makefile's DEVICE_HDR).
#pragma once

#include "search.hpp"
#include "cull.hpp"

namespace rrte {

// --------------------------------------------------------------- lighting
struct Contrib { float cr, cg, cb, ca; f3 dir; float dist, att; };

// PointLight::calculate_attenuation (light.rs:170-178)
__device__ __forceinline__ float point_att(const DLight& l, float d) {
    if (d > l.range) return 0.0f;
    float a = rcp_rn((1.0f + l.linear * d) + (l.quadratic * d) * d);
    return mx(a, 0.0f);
}

// Light::illuminate (light.rs:87-94, 182-194, 289-304, 365-372)
__device__ __forceinline__ Contrib illuminate(const DLight& l, f3 p) {
    Contrib k;
    k.cr = l.cI[0]; k.cg = l.cI[1]; k.cb = l.cI[2]; k.ca = l.cI[3];
    switch (l.kind) {
    case RRTE_LIGHT_POINT: {
        f3 lv = vsub(V(l.position[0], l.position[1], l.position[2]), p);
        k.dist = vlen(lv);
        k.dir = vnorm(lv);
        k.att = point_att(l, k.dist);
        break;
    }
    case RRTE_LIGHT_DIRECTIONAL:
        k.dir = vneg(V(l.direction[0], l.direction[1], l.direction[2]));
        k.dist = kInf;
        k.att = 1.0f;
        break;
    case RRTE_LIGHT_SPOT: {
        f3 lv = vsub(V(l.position[0], l.position[1], l.position[2]), p);
        k.dist = vlen(lv);
        k.dir = vnorm(lv);
        float da = point_att(l, k.dist);
        float ang = acosf(vdot(V(l.direction[0], l.direction[1], l.direction[2]), vneg(k.dir)));
        float aa;
        if (ang > l.outer_angle) aa = 0.0f;
        else if (ang < l.inner_angle) aa = 1.0f;
        else {
            float fo = (l.outer_angle - ang) / (l.outer_angle - l.inner_angle);
            aa = fo * fo;
        }
        k.att = da * aa;
        break;
    }
    default:
        k.dir = V(0.0f, 0.0f, 0.0f);
        k.dist = 0.0f;
        k.att = 1.0f;
        break;
    }
    return k;
}

__device__ __forceinline__ f3 rand_in_unit_sphere(uint32_t& st) {  // vector.rs:35-46
    for (;;) {
        float x = rng_f32(st) * 2.0f - 1.0f;
        float y = rng_f32(st) * 2.0f - 1.0f;
        float z = rng_f32(st) * 2.0f - 1.0f;
        f3 p = V(x, y, z);
        if (vlen2(p) < 1.0f) return p;
    }
}
__device__ __forceinline__ f3 reflect3(f3 v, f3 n) { return vsub(v, vmuls(n, 2.0f * vdot(v, n))); }

// Material::scatter (material.rs:60-72, 99-110, 147-170, 200-202)
__device__ __forceinline__ bool scatter(const DMaterial& m, const Ray& rin, const Hit& h, uint32_t& st, Ray& out) {
    switch (m.kind) {
    case RRTE_MAT_LAMBERTIAN: {
        f3 sd = vadd(h.n, vnorm(rand_in_unit_sphere(st)));
        f3 dir = vlen2(sd) < 1e-8f ? h.n : sd;
        out = ray_new(h.p, dir);
        return true;
    }
    case RRTE_MAT_METAL: {
        f3 refl = reflect3(vnorm(rin.d), h.n);
        f3 s = vadd(refl, vmuls(rand_in_unit_sphere(st), m.fuzz));
        if (vdot(s, h.n) > 0.0f) { out = ray_new(h.p, s); return true; }
        return false;
    }
    case RRTE_MAT_DIELECTRIC: {
        float ratio = h.front ? rcp_rn(m.ior) : m.ior;
        f3 ud = vnorm(rin.d);
        float cos_t = mn(vdot(vneg(ud), h.n), 1.0f);
        float sin_t = sqrt_rn(1.0f - cos_t * cos_t);
        bool cannot = ratio * sin_t > 1.0f;
        float r0 = (1.0f - ratio) / (1.0f + ratio);
        r0 = r0 * r0;
        float x = 1.0f - cos_t;
        float x2 = x * x;
        float refl = r0 + (1.0f - r0) * (x * (x2 * x2));
        bool do_reflect = cannot;
        if (!do_reflect) do_reflect = refl > rng_f32(st);
        f3 dir;
        if (do_reflect) {
            dir = reflect3(ud, h.n);
        } else {
            float ct = mn(vdot(vneg(ud), h.n), 1.0f);
            f3 perp = vmuls(vadd(ud, vmuls(h.n, ct)), ratio);
            float l2 = vlen2(perp);
            f3 par = vmuls(h.n, -sqrt_rn(fabsf(1.0f - l2)));
            dir = (l2 < 1.0f) ? vadd(perp, par) : reflect3(ud, h.n);
        }
        out = ray_new(h.p, dir);
        return true;
    }
    default:
        return false;
    }
}

// ----------------------------------------------------------------- pixel
struct Col { float r, g, b, a; };

// Camera::generate_ray (camera.rs:98-133)
__device__ __forceinline__ Ray generate_ray(const FrameCam& cm, float u, float v) {
    float ndc_x = 2.0f * u - 1.0f;
    float ndc_y = 1.0f - 2.0f * v;
    if (cm.projection == RRTE_PERSPECTIVE) {
        float half_w = cm.aspect * cm.half_h;
        f3 cd = vnorm(V(ndc_x * half_w, ndc_y * cm.half_h, -1.0f));
        f3 wd = quat_rotate(cm.cam_rot, cd);
        return ray_new_unit(V(cm.cam_pos[0], cm.cam_pos[1], cm.cam_pos[2]), wd);
    }
    float wx = cm.ortho_l + (cm.ortho_r - cm.ortho_l) * u;
    float wy = cm.ortho_b + (cm.ortho_t - cm.ortho_b) * v;
    f3 o = m_point(cm.cam_xf, V(wx, wy, 0.0f));
    f3 wd = quat_rotate(cm.cam_rot, V(0.0f, 0.0f, -1.0f));
    return ray_new_unit(o, wd);
}

// Raytracer::ray_color (raytracer.rs:92-148) for one camera sample.
// REFCOMPAT: ambient + sum(light.color*I*att) + albedo * ray_color(scatter).
// The reference recursion color_d = local_d + albedo_d * color_{d+1} is
// evaluated forward with a running albedo product; that is bit-identical to
// the recursion for max_depth <= 2 (the parity configs use 1) and differs by
// rounding only beyond.
// Material record of a hit (nullptr = no material -> BLACK, raytracer.rs:139-143).
template <class S>
__device__ __forceinline__ const DMaterial* material_of(const S& sc, int idx) {
    const int mi = sc.prims[idx].material;
    return (mi < 0 || (uint32_t)mi >= sc.num_materials) ? nullptr : &sc.mats[mi];
}

// REFCOMPAT: Raytracer::ray_color (raytracer.rs:92-148) for one camera ray:
// ambient + sum(light.color*I*att) + albedo * ray_color(scatter).  The
// reference recursion color_d = local_d + albedo_d * color_{d+1} is evaluated
// forward with a running albedo product: bit-identical to the recursion for
// max_depth <= 2 (the parity configs use 1), rounding-level beyond.  A path is
// advanced one bounce at a time (path_step) so that the kernel can start a
// lane's next sample as soon as its current path ends (see ray_kernel_body).
struct PathState {
    Ray r;
    Col out;
    float tr, tg, tb;  // running albedo product
    uint32_t depth;
};

__device__ __forceinline__ void path_begin(PathState& ps, const Ray& r) {
    ps.r = r;
    ps.out = Col{0.0f, 0.0f, 0.0f, 1.0f};
    ps.tr = ps.tg = ps.tb = 1.0f;
    ps.depth = 0;
}

// One bounce of ray_color (kp.max_depth >= 1); true when the path has ended.  pmask: camera-ray
// tile culling mask (only for the camera ray, ~0u otherwise).
template <class S>
__device__ __forceinline__ bool path_step(const S& sc, const KParams& kp, PathState& ps, uint32_t& st,
                                          uint32_t pmask = ~0u) {
    Hit h;
    const int idx = closest_hit(sc, ps.r, kp.t_min, h, pmask);
    const uint32_t depth = ps.depth;
    if (idx < 0) {
        if (depth == 0) {
            ps.out = Col{kp.bg[0], kp.bg[1], kp.bg[2], kp.bg[3]};
        } else {
            ps.out.r = ps.out.r + ps.tr * kp.bg[0];
            ps.out.g = ps.out.g + ps.tg * kp.bg[1];
            ps.out.b = ps.out.b + ps.tb * kp.bg[2];
        }
        return true;
    }
    const DMaterial* m = material_of(sc, idx);
    if (!m) return true;  // BLACK
    float ar = m->albedo[0], ag = m->albedo[1], ab = m->albedo[2], aa = m->albedo[3];
    // BLACK + ambient_color()*0.1 (raytracer.rs:124, material.rs:10-12)
    float cr = 0.0f + (ar * 0.1f) * 0.1f;
    float cg = 0.0f + (ag * 0.1f) * 0.1f;
    float cb = 0.0f + (ab * 0.1f) * 0.1f;
    float ca = 1.0f + (aa * 0.1f) * 0.1f;
    for_each_light(sc, [&](auto lii) {
        Contrib k = illuminate(light_at(sc, lii), h.p);
        cr = cr + k.cr * k.att;
        cg = cg + k.cg * k.att;
        cb = cb + k.cb * k.att;
        ca = ca + k.ca * k.att;
    });
    if (depth == 0) {
        ps.out = Col{cr, cg, cb, ca};
    } else {
        ps.out.r = ps.out.r + ps.tr * cr;
        ps.out.g = ps.out.g + ps.tg * cg;
        ps.out.b = ps.out.b + ps.tb * cb;
    }
    Ray sc_ray;
    if (!scatter(*m, ps.r, h, st, sc_ray)) return true;
    if (depth == 0) ps.out.a = ps.out.a + 1.0f;  // Color::from(Vec3) has alpha 1 (color.rs:78-82)
    if (depth + 1 >= kp.max_depth) return true;   // ray_color(depth 0) == BLACK: adds 0
    ps.tr = ps.tr * ar;
    ps.tg = ps.tg * ag;
    ps.tb = ps.tb * ab;
    ps.r = sc_ray;
    ps.depth = depth + 1;
    return false;
}

// The whole path of one camera ray.  SINGLE (scene-specialised straight-line kernels): one
// bounce only (max_depth <= 1).
template <class S, bool SINGLE>
__device__ __forceinline__ Col ray_color_ref(const S& sc, const KParams& kp, Ray r, uint32_t& st,
                                             uint32_t pmask = ~0u) {
    PathState ps;
    path_begin(ps, r);
    if (kp.max_depth == 0) return ps.out;
    if constexpr (SINGLE) {
        path_step(sc, kp, ps, st, pmask);
    } else {
#pragma unroll 1
        while (!path_step(sc, kp, ps, st)) {
        }
    }
    return ps.out;
}

// Launch traits of ray_kernel_body: what the kernel may assume about its launch at compile time.
// LaunchAny assumes nothing.  LaunchPlain is the frame an engine renders in a stream (the host checks
// every condition before it picks that entry, rrte_hip.hip plain_launch): one frame per launch
// (nframes 1, the output is the argument pointer), no band map (band_rows, row0, out_image_rows 0),
// debug 0, no f32 output, RGBA8 stores to device memory (no slab, no host-store flag), gamma 2.2, one
// sample per pixel (inv_spp 1).  Those launch values are then constants and the per-wave checks on
// them (a scalar load, a wait and a branch each) fold away.  The tile list and the tile profile
// (KParams::hot, tile_cost) stay run-time values: a stream's frames use the list, and a profiled
// launch then times the entry the list is for.  The values are read
// through accessors, never from a patched copy of KParams: a copy sends the 3.5 KB block to scratch.
struct LaunchAny { static constexpr bool kPlain = false; };
struct LaunchPlain { static constexpr bool kPlain = true; };
template <class LT>
__device__ __forceinline__ uint32_t launch_debug(const KParams& kp) {
    if constexpr (LT::kPlain) return 0u;
    else return kp.debug;
}

// LAMBERT_SHADOW (build-defined) for one camera ray.  Called by
// all 64 lanes of the wave (`live` marks the lanes that own a pixel): with
// CULL the hit-point bound and the per-light shadow culls are wave reductions.
template <class S, bool CULL, class LT = LaunchAny>
__device__ __forceinline__ Col shade_lambert(const S& sc, const KParams& kp, const Cull& cl, const Ray& r, bool live,
                                             uint32_t& nshadow, uint32_t pmask) {
    const uint32_t debug = launch_debug<LT>(kp);
    Col out{0.0f, 0.0f, 0.0f, 1.0f};
    if (kp.max_depth == 0) return out;
    Hit h;
    h.t = 0.0f;  // lanes without a hit keep a benign point and normal
    h.p = V(0.0f, 0.0f, 0.0f);
    h.n = V(0.0f, 1.0f, 0.0f);
    h.front = true;
    h.sub = 0u;
    // RRTE_DEBUG bit 7 (timing diagnostics only, with bit 1): the closest-hit search without hit attributes
    const int idx = closest_hit(sc, r, live ? kp.t_min : kInf, h, pmask, !(debug & 128u));  // idle lanes find nothing
    const DMaterial* m = idx >= 0 ? material_of(sc, idx) : nullptr;
    const bool hit = m != nullptr;
    if (idx < 0) out = Col{kp.bg[0], kp.bg[1], kp.bg[2], kp.bg[3]};
    if (debug & 2u) {  // diagnostics: primary visibility only
        if (idx >= 0) out = Col{h.t * 0.01f, 0.0f, 0.0f, 1.0f};
        return out;
    }
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f, ca = 1.0f;
    if (hit) {
        ar = m->albedo[0]; ag = m->albedo[1]; ab = m->albedo[2];
        // BLACK + ambient_color()*0.1 (raytracer.rs:124, material.rs:10-12)
        cr = 0.0f + (ar * 0.1f) * 0.1f;
        cg = 0.0f + (ag * 0.1f) * 0.1f;
        cb = 0.0f + (ab * 0.1f) * 0.1f;
        ca = 1.0f + (m->albedo[3] * 0.1f) * 0.1f;
    }
    const float bias = kp.bias;
    // contribution of one light to a hit lane (light.rs illuminate + N.L + shadow ray)
    // RRTE_DEBUG bit 8 (timing diagnostics only, wrong images): shadow tests for light (debug >> 9) & 7 only
    auto shade = [&](const DLight& l, uint64_t smask, uint32_t li) {
        Contrib k = illuminate(l, h.p);
        if (l.kind == RRTE_LIGHT_AMBIENT) {
            if (hit) {
                cr = cr + ar * k.cr;
                cg = cg + ag * k.cg;
                cb = cb + ab * k.cb;
            }
            return;
        }
        const float ndl = vdot(h.n, k.dir);
        if (ndl > 0.0f && k.att > 0.0f) {
            ++nshadow;
            Ray sr = ray_new_unit(vadd(h.p, vmuls(h.n, bias)), k.dir);
            // RRTE_DEBUG bit 6 (timing diagnostics only, wrong images): skip the object the ray starts on
            if ((debug & 1u) || ((debug & 256u) && li != ((debug >> 9) & 7u)) ||
                !occluded(sc, sr, bias, k.dist, smask, (debug & 64u) ? idx : -1)) {
                float f = k.att * ndl;
                cr = cr + ar * (k.cr * f);
                cg = cg + ag * (k.cg * f);
                cb = cb + ab * (k.cb * f);
            }
        }
    };
    if constexpr (!CULL) {
        if (hit) for_each_light(sc, [&](auto lii) { shade(light_at(sc, lii), ~0ull, (uint32_t)lii); });
    } else {
        HitBound hb{};
        hb.unsafe = true;  // no bounds table: every mask all-ones
        if (cull_on(cl)) hb = wave_hit_bound(hit, h.p, h.n, bias);
        if constexpr (S::kStatic) {
            // all light masks first, at one converged point, then the shading
            uint64_t smask[S::num_lights ? S::num_lights : 1];
            if constexpr (S::num_lights > 0 && S::num_prims * S::num_lights <= 64u) {
                shadow_cull_lanes<S>(sc, cl, hb, smask);
            } else {
                const float4 bnd = cull_on(cl) ? load_bound(cl) : float4{};
                auto cull_one = [&](auto lii) { smask[(uint32_t)lii] = shadow_cull(cl, hb, light_at(sc, lii), bnd); };
                static_for<0, S::num_lights>(cull_one);
            }
            auto shade_one = [&](auto lii) { if (hit) shade(light_at(sc, lii), smask[(uint32_t)lii], (uint32_t)lii); };
            static_for<0, S::num_lights>(shade_one);
        } else {
            const float4 bnd = cull_on(cl) ? load_bound(cl) : float4{};
#pragma unroll 1
            for (uint32_t li = 0; li < sc.num_lights; ++li) {
                const DLight lt = load_uniform(sc.lights + li);  // (li uniform: scalar loads)
                const uint64_t sm = shadow_cull(cl, hb, lt, bnd);
                if (hit) shade(lt, sm, li);
            }
        }
    }
    if (hit) out = Col{cr, cg, cb, ca};
    return out;
}

}  // namespace rrte
