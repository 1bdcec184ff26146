// mesh_walk.hpp — one ray against a triangle mesh.
//
// Moller-Trumbore on the host's precomputed edges (mt_test, mesh_tri_*), the workgroup geometry
// (kBlockThreads) and the per-lane traversal stack in LDS (mesh_stack), the slab test (box_entry), the
// BVH walk with its original-order scan for rays the culls cannot answer (isect_mesh, kCullReach), and
// the instance path: the same walk through an object's transform (instance_ray, isect_mesh_instance,
// mesh_instance_hit).
//
// Includes scene_view.hpp.  Included by search.hpp and cull.hpp.  Embedded for hiprtc (the Makefile's
// DEVICE_HDR).
#pragma once

#include "scene_view.hpp"

namespace rrte {

// ---------------------------------------------------------------- meshes
// Moller-Trumbore exactly as Triangle::intersect (primitives.rs:208-244), with e1 = v1-v0 and
// e2 = v2-v0 precomputed on the host (the same f32 subtractions).
__device__ __forceinline__ bool mt_test(f3 v0, f3 e1, f3 e2, const Ray& r, float t_min, float t_max, float& t,
                                        float& u, float& v) {
    f3 h = vcross(r.d, e2);
    float a = vdot(e1, h);
    if (a > -1e-6f && a < 1e-6f) return false;
    float f = rcp_rn(a);
    f3 s = vsub(r.o, v0);
    u = f * vdot(s, h);
    if (u < 0.0f || u > 1.0f) return false;
    f3 q = vcross(s, e1);
    v = f * vdot(r.d, q);
    if (v < 0.0f || u + v > 1.0f) return false;
    t = f * vdot(e2, q);
    if (t < t_min || t > t_max) return false;
    return true;
}

__device__ __forceinline__ f3 xyz(float4 a) { return V(a.x, a.y, a.z); }

// Triangle slot k against r: re-run the test for (u, v); t and the barycentric normal
// (primitives.rs:240-243), normalised, not yet flipped towards the ray.
__device__ __forceinline__ bool mesh_tri_local(const MeshView& mv, uint32_t k, const Ray& r, float t_min, float t_max,
                                               float& t, f3& n) {
    float u, v;
    if (!mt_test(xyz(mv.tris[3 * k]), xyz(mv.tris[3 * k + 1]), xyz(mv.tris[3 * k + 2]), r, t_min, t_max, t, u, v))
        return false;
    float w = 1.0f - u - v;
    n = vnorm(vadd(vadd(vmuls(xyz(mv.norms[3 * k]), w), vmuls(xyz(mv.norms[3 * k + 1]), u)),
                   vmuls(xyz(mv.norms[3 * k + 2]), v)));
    return true;
}

// Hit attributes of triangle slot k: mesh_tri_local, then HitInfo::new.
__device__ __forceinline__ bool mesh_tri_hit(const MeshView& mv, uint32_t k, const Ray& r, float t_min, float t_max,
                                             Hit& out) {
    float t;
    f3 n;
    if (!mesh_tri_local(mv, k, r, t_min, t_max, t, n)) return false;
    f3 p = ray_at(r, t);
    hit_new(out, t, p, n, r);
    out.sub = k;
    return true;
}

// Workgroup geometry: one wave per workgroup, one 8x8 pixel tile each (kBlockThreads = 64).  A
// workgroup's waves must start together on one CU and a 4-wave workgroup needs a free slot on every
// SIMD, so with a few long-running (grazing-ray) waves resident, 256-thread workgroups of 16x16 pixels
// left slots idle that single waves fill: -9 % per frame (a switch that restored the
// 256-thread layout for that A/B has been retired).
constexpr uint32_t kBlockThreads = 64u;

constexpr int kMeshStack = 32;  // BVH depth is capped below this at build time

// The magnitude up to which the shortcuts that rest on "a hit the reference reports lies inside the
// object's bound" hold: below it the intersectors' products of up to three coordinates stay finite
// in f32.  Beyond it the reference reports hits with t = NaN or +inf for rays that pass nowhere near
// the object (sphere: hb^2 and a cc both +inf, disc = NaN, every comparison fails), and at such
// distances its rounding alone decides which triangle of a mesh a ray "hits".  There the shadow and
// tile culls stand down (wave_hit_bound; bvh.hip gives such objects the radius +inf) and a mesh is
// scanned in its original order instead of through its BVH (isect_mesh).
constexpr float kCullReach = 0x1p40f;
__device__ __forceinline__ uint32_t* mesh_stack() {
    __shared__ uint32_t stk[kMeshStack * kBlockThreads];  // [depth][lane of the workgroup]
    return stk + threadIdx.x;
}

// Slab test against an (inflated) node box, clipped to [t_min, t_max]: the entry t, or +inf.
__device__ __forceinline__ float box_entry(float4 lo, float4 hi, f3 o, f3 inv, float t_min, float t_max) {
    float tx0 = (lo.x - o.x) * inv.x, tx1 = (hi.x - o.x) * inv.x;
    float ty0 = (lo.y - o.y) * inv.y, ty1 = (hi.y - o.y) * inv.y;
    float tz0 = (lo.z - o.z) * inv.z, tz1 = (hi.z - o.z) * inv.z;
    float tn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), t_min));
    float tf = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fminf(fmaxf(tz0, tz1), t_max));
    return tn <= tf ? tn : kInf;
}

// The mesh as a Vec<Triangle>: closest hit over its triangles in index order (strict '<', the
// lower index wins a tie) or, with ANY, whether any triangle is hit.  The BVH visits the near
// child first and prunes boxes entered beyond the current best; boxes are inflated at build time
// so the pruning never drops a triangle the test would accept (meshes).  Rays with
// a non-finite component take the original-order scan (every test then "hits" with t = NaN, as
// in the reference, and the lowest index wins), and so do rays that start beyond kCullReach, rays
// against a mesh whose root boxes reach beyond it, and rays that start 2^24 or more of the mesh's
// extents away from it (one ulp of such an origin is larger than the mesh): there the triangle
// test's own rounding or overflow, not the geometry, decides what the reference reports, and no box
// bounds that.  A mesh of one leaf (at most four triangles) is always scanned.
// Writes t and the triangle slot (out.sub).
template <bool ANY>
__device__ __forceinline__ bool isect_mesh(const DPrim& pr, const MeshView& mv, const Ray& r, float t_min,
                                           float t_max, Hit& out) {
    const uint32_t count = pr.sdf_count, base = (uint32_t)pr.p[0];
    bool found = false;
    float best = kInf;
    uint32_t best_k = 0u, best_orig = 0u;
    bool scan = !(finite3(r.o) && finite3(r.d)) || !(fmaxf(fmaxf(fabsf(r.o.x), fabsf(r.o.y)), fabsf(r.o.z)) < kCullReach);
    if (count && !(pr.sdf_first & 0x80000000u)) {  // (wave-uniform: the root's two child boxes)
        const float4* rec = mv.nodes + 4u * pr.sdf_first;
        const float4 l0 = rec[0], h0 = rec[1], l1 = rec[2], h1 = rec[3];
        const f3 lo = V(fminf(l0.x, l1.x), fminf(l0.y, l1.y), fminf(l0.z, l1.z));
        const f3 hi = V(fmaxf(h0.x, h1.x), fmaxf(h0.y, h1.y), fmaxf(h0.z, h1.z));
        const float m = fmaxf(fmaxf(fmaxf(fabsf(lo.x), fabsf(lo.y)), fabsf(lo.z)), fmaxf(fmaxf(fabsf(hi.x), fabsf(hi.y)), fabsf(hi.z)));
        // the ray's start is `dist` (largest-coordinate norm) from the root box of extent `ext`: from
        // 2^24 extents on, one ulp of the origin is larger than the whole mesh
        const float ext = fmaxf(fmaxf(hi.x - lo.x, hi.y - lo.y), hi.z - lo.z);
        const float dist = fmaxf(fmaxf(fmaxf(lo.x - r.o.x, r.o.x - hi.x), fmaxf(lo.y - r.o.y, r.o.y - hi.y)),
                                 fmaxf(fmaxf(lo.z - r.o.z, r.o.z - hi.z), 0.0f));
        scan = scan || !(m < kCullReach) || !(dist < 0x1p24f * ext);
    } else {
        scan = true;  // the whole mesh is one leaf: the scan is the same few tests, in the original order
    }
    if (scan) {
        for (uint32_t i = 0; i < count; ++i) {
            const uint32_t k = mv.perm[base + i];
            float t, u, v;
            if (mt_test(xyz(mv.tris[3 * k]), xyz(mv.tris[3 * k + 1]), xyz(mv.tris[3 * k + 2]), r, t_min, t_max, t, u, v)) {
                if (!found || t < best) {
                    best = t;
                    best_k = k;
                    found = true;
                    if (ANY) break;
                }
            }
        }
    } else {
        const f3 inv = V(rcp_rn(r.d.x), rcp_rn(r.d.y), rcp_rn(r.d.z));
        uint32_t* stk = mesh_stack();
        int sp = 0;
        uint32_t link = count ? pr.sdf_first : 0u;
        while (count) {
            if (!(link & 0x80000000u)) {
                // interior: test both children, descend into the nearer, keep the farther
                const float4* rec = mv.nodes + 4u * link;
                const float4 l0 = rec[0], h0 = rec[1], l1 = rec[2], h1 = rec[3];
                const float cap = found ? fminf(best, t_max) : t_max;
                const float t0 = box_entry(l0, h0, r.o, inv, t_min, cap);
                const float t1 = box_entry(l1, h1, r.o, inv, t_min, cap);
                const uint32_t c0 = __float_as_uint(l0.w), c1 = __float_as_uint(l1.w);
                if (t0 != kInf && t1 != kInf) {
                    const bool near0 = t0 <= t1;
                    stk[(sp++) * kBlockThreads] = near0 ? c1 : c0;
                    link = near0 ? c0 : c1;
                    continue;
                }
                if (t0 != kInf) {
                    link = c0;
                    continue;
                }
                if (t1 != kInf) {
                    link = c1;
                    continue;
                }
            } else {
                const uint32_t a = link & 0xFFFFFFu, n = ((link >> 24) & 0x7Fu) + 1u;
                for (uint32_t k = a; k < a + n; ++k) {
                    const float4 A = mv.tris[3 * k];
                    float t, u, v;
                    if (mt_test(xyz(A), xyz(mv.tris[3 * k + 1]), xyz(mv.tris[3 * k + 2]), r, t_min, t_max, t, u, v)) {
                        const uint32_t orig = __float_as_uint(A.w);
                        if (!found || t < best || (t == best && orig < best_orig)) {
                            best = t;
                            best_k = k;
                            best_orig = orig;
                            found = true;
                        }
                        if (ANY) break;
                    }
                }
                if (ANY && found) break;
            }
            if (sp == 0) break;
            link = stk[(--sp) * kBlockThreads];
        }
    }
    out.t = best;
    out.sub = best_k;
    return found;
}

// ------------------------------------------------------- mesh instances
// RRTE_PRIM_MESH_INSTANCE (rrte_hip.h): the object-space ray of local_ray(), the length `len` the
// direction had before it was normalised, and the world interval in local units.  t along the local
// ray is len times t along the world ray, so the hit's t goes back as tl / len: in world units,
// comparable with every other object's.
struct InstanceRay {
    Ray lr;
    float len, t_min, t_max;
};
__device__ __forceinline__ InstanceRay instance_ray(const DPrim& pr, const Ray& r, float t_min, float t_max) {
    InstanceRay ir;
    const f3 v = m_vector(pr.inv, r.d);
    ir.len = sqrt_rn(vlen2(v));
    ir.lr = ray_new(m_point(pr.inv, r.o), vnorm(v));
    ir.t_min = t_min * ir.len;
    ir.t_max = t_max == kInf ? kInf : t_max * ir.len;
    return ir;
}

template <bool ANY>
__device__ __forceinline__ bool isect_mesh_instance(const DPrim& pr, const MeshView& mv, const Ray& r, float t_min,
                                                    float t_max, Hit& out) {
    const InstanceRay ir = instance_ray(pr, r, t_min, t_max);
    if (!isect_mesh<ANY>(pr, mv, ir.lr, ir.t_min, ir.t_max, out)) return false;
    out.t = out.t / ir.len;
    return true;
}

// Hit attributes of an instance's triangle slot k: the slot's test on the local ray over the local
// interval, the point through xf, the normal through the inverse transpose (n_w[j] = column j of
// inv . n_l: right under non-uniform scale and mirroring), HitInfo::new against the world ray.
__device__ __forceinline__ bool mesh_instance_hit(const DPrim& pr, const MeshView& mv, uint32_t k, const Ray& r,
                                                  float t_min, float t_max, Hit& out) {
    const InstanceRay ir = instance_ray(pr, r, t_min, t_max);
    float tl;
    f3 nl;
    if (!mesh_tri_local(mv, k, ir.lr, ir.t_min, ir.t_max, tl, nl)) return false;
    const f3 nw = V(vdot(vld(pr.inv), nl), vdot(vld(pr.inv + 3), nl), vdot(vld(pr.inv + 6), nl));
    hit_new(out, tl / ir.len, m_point(pr.xf, ray_at(ir.lr, tl)), vnorm(nw), r);
    out.sub = k;
    return true;
}

}  // namespace rrte
