// search.hpp — one ray against the scene.
//
// The object dispatch (intersect_at: by kind at run time for the runtime scene, with_leaf_program for
// its one-leaf SDF objects; only the object's own intersector for a compile-time index; prim_convex),
// the closest-hit search and the attributes of each lane's winner (closest_t, attributes_at,
// hit_attributes, closest_hit), and the any-hit search of shadow rays (any_hit_at, occluded).
// accel_kernels.hpp and search_groups.hpp overload closest_t / occluded on their own scene types.
//
// Includes intersect.hpp and mesh_walk.hpp.  Included by shade.hpp.  Embedded for
// hiprtc (the Makefile's DEVICE_HDR).
#pragma once

#include "intersect.hpp"
#include "mesh_walk.hpp"

namespace rrte {

// The one-leaf dispatch of the runtime scene (RRTE_SDF_LEAF_DISPATCH): f(UC<OP>, SdfLeafProgram<OP>) for
// the kind OP of the program's one node, so that what f calls runs that leaf's straight-line distance.
template <class F>
__device__ __forceinline__ void with_leaf_program(const rrte_sdf_node* nd, F&& f) {
    const rrte_sdf_node n = load_uniform(nd);
    auto leaf = [&](auto opc) {
        constexpr uint32_t OP = decltype(opc)::value;
        if (n.op == OP) f(opc, SdfLeafProgram<OP>{load_uniform(reinterpret_cast<const NodeArgs*>(nd->f))});
    };
    static_for_leaves(leaf);
}

// SceneObject::intersect dispatch, runtime object index: switch on the kind
// (wave-uniform -> scalar branches).
template <bool NEED_HIT, class S, bool ANY = false>
__device__ __forceinline__ bool intersect_at(const S& sc, uint32_t i, const Ray& r, float t_min, float t_max,
                                             Hit& out) {
    const DPrim pr = load_uniform(sc.prims + i);  // (i is wave-uniform: scalar loads)
    constexpr uint32_t F = S::kFeat;
    // (a kind outside the variant's features cannot occur: the host picked the variant from the scene)
    if (pr.kind == RRTE_PRIM_SPHERE) return isect_sphere<NEED_HIT, ANY>(pr, r, t_min, t_max, out);
    if constexpr ((F & kFeatSdf) != 0u)
        if (pr.kind == RRTE_PRIM_SDF) {
            const rrte_sdf_node* nd = sc.nodes + pr.sdf_first;
            if (RRTE_SDF_LEAF_DISPATCH && pr.sdf_count == 1u) {
                bool hit = false;
                with_leaf_program(nd, [&](auto opc, const auto& prog) {
                    constexpr uint32_t OP = decltype(opc)::value;
                    hit = isect_sdf<NEED_HIT, SdfLeafProgram<OP>, ANY,
                                    (ANY ? kSecantExit >= 1 : kSecantExit >= 2) && leaf_convex<OP>()>(pr, prog, r, t_min,
                                                                                                      t_max, out);
                });
                return hit;
            }
            return isect_sdf<NEED_HIT, SdfProgramT<F>, ANY>(pr, SdfProgramT<F>{nd, pr.sdf_count}, r, t_min, t_max, out);
        }
    if constexpr ((F & kFeatAnalytic) != 0u) {
        switch (pr.kind) {
        case RRTE_PRIM_PLANE: return isect_plane<NEED_HIT>(pr, r, t_min, t_max, out);
        case RRTE_PRIM_TRIANGLE: return isect_triangle<NEED_HIT>(pr, r, t_min, t_max, out);
        case RRTE_PRIM_CUBE: return isect_cube<NEED_HIT>(pr, r, t_min, t_max, out);
        case RRTE_PRIM_CYLINDER: return isect_cylinder<NEED_HIT>(pr, r, t_min, t_max, out);
        case RRTE_PRIM_CONE: return isect_cone<NEED_HIT>(pr, r, t_min, t_max, out);
        case RRTE_PRIM_CAPSULE: return isect_capsule<NEED_HIT>(pr, r, t_min, t_max, out);
        default: break;
        }
    }
    if constexpr ((F & kFeatMesh) != 0u)
        if (pr.kind == RRTE_PRIM_MESH) return isect_mesh<ANY>(pr, sc.mesh, r, t_min, t_max, out);
    if constexpr ((F & kFeatInstance) != 0u)
        if (pr.kind == RRTE_PRIM_MESH_INSTANCE) return isect_mesh_instance<ANY>(pr, sc.mesh, r, t_min, t_max, out);
    return false;
}

// Compile-time object index (scene-specialised kernel): only the object's
// own intersector is instantiated.
// Convexity of object I's SDF program for the secant early miss (sdf_convex): decided at compile time
// from the constant program for a full scene, by the host for a topology scene (its topology key).
template <class S, uint32_t I>
constexpr bool prim_convex() {
    if constexpr (S::kTopo) return S::topo_prims[I].convex;
    else return sdf_convex(S::nodes + S::prims[I].sdf_first, S::prims[I].sdf_count);
}
template <bool NEED_HIT, class S, uint32_t I, bool ANY = false>
__device__ __forceinline__ bool intersect_at(const S& sc, UC<I> ii, const Ray& r, float t_min, float t_max, Hit& out) {
    const DPrim pr = prim_at(sc, ii);
    constexpr uint32_t kind = prim_kind<S, I>();
    if constexpr (kind == RRTE_PRIM_SPHERE) return isect_sphere<NEED_HIT, ANY>(pr, r, t_min, t_max, out);
    else if constexpr (kind == RRTE_PRIM_PLANE) return isect_plane<NEED_HIT>(pr, r, t_min, t_max, out);
    else if constexpr (kind == RRTE_PRIM_TRIANGLE) return isect_triangle<NEED_HIT>(pr, r, t_min, t_max, out);
    else if constexpr (kind == RRTE_PRIM_CUBE) return isect_cube<NEED_HIT>(pr, r, t_min, t_max, out);
    else if constexpr (kind == RRTE_PRIM_CYLINDER) return isect_cylinder<NEED_HIT>(pr, r, t_min, t_max, out);
    else if constexpr (kind == RRTE_PRIM_CONE) return isect_cone<NEED_HIT>(pr, r, t_min, t_max, out);
    else if constexpr (kind == RRTE_PRIM_CAPSULE) return isect_capsule<NEED_HIT>(pr, r, t_min, t_max, out);
    else if constexpr (kind == RRTE_PRIM_SDF)
        return isect_sdf<NEED_HIT, SdfStaticProgram<S, prim_first<S, I>(), prim_count<S, I>()>, ANY,
                         (ANY ? kSecantExit >= 1 : kSecantExit >= 2) && prim_convex<S, I>()>(
            pr, SdfStaticProgram<S, prim_first<S, I>(), prim_count<S, I>()>{sc}, r, t_min, t_max, out);
    else if constexpr (kind == RRTE_PRIM_MESH) return isect_mesh<ANY>(pr, sc.mesh, r, t_min, t_max, out);
    else if constexpr (kind == RRTE_PRIM_MESH_INSTANCE)
        return isect_mesh_instance<ANY>(pr, sc.mesh, r, t_min, t_max, out);
    else return false;
}

// Closest hit over all objects (raytracer.rs:103-113): strict '<' keeps the
// earlier object on ties; analytic objects get t_max = INFINITY as in the
// reference, SDF objects march only up to the current closest hit.  The
// search carries only (t, object); attributes are produced afterwards.
// `pmask` (camera rays): bit i clear = object i's bounding sphere lies outside this workgroup's
// pixel block (KParams::tile_rect), so no lane can hit it and its test is skipped (exact: the
// skipped test would have missed on every lane).
template <class S>
__device__ __forceinline__ int closest_t(const S& sc, const Ray& r, float t_min, float& best_t, uint32_t& best_sub,
                                         uint32_t pmask = ~0u) {
    int idx = -1;
    best_t = kInf;
    best_sub = 0u;
    for_each_prim(sc, [&](auto ii) {
        const uint32_t i = ii;
        if (i < 32u && !((pmask >> i) & 1u)) return;
        Hit h;
        h.sub = 0u;
        float tmax = (prim_at(sc, ii).kind == RRTE_PRIM_SDF && idx >= 0) ? best_t : kInf;
        if (intersect_at<false>(sc, ii, r, t_min, tmax, h)) {
            if (idx < 0 || h.t < best_t || (h.t == best_t && (int)i < idx)) {
                best_t = h.t;
                best_sub = h.sub;
                idx = (int)i;
            }
        }
    });
    return idx;
}

// Hit attributes for the winning object of each lane: analytic objects are
// re-intersected with the search's exact arguments, SDF objects evaluate
// point + normal at the found t -- bit-identical to computing them during the
// search.  Runtime scene: the wave walks its distinct winners (readfirstlane
// -> uniform object index -> scalar loads).  Static scene: every object is
// visited with a compile-time index and skipped unless some lane won it.
template <class S>
__device__ __forceinline__ void attributes_at(const S& sc, uint32_t i, const Ray& r, float t_min, float t,
                                              uint32_t sub, Hit& out) {
    const DPrim pr = load_uniform(sc.prims + i);  // (i is wave-uniform: scalar loads)
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
            mesh_tri_hit(sc.mesh, sub, r, t_min, kInf, out);
            return;
        }
    }
    if constexpr ((F & kFeatInstance) != 0u) {
        if (pr.kind == RRTE_PRIM_MESH_INSTANCE) {
            mesh_instance_hit(pr, sc.mesh, sub, r, t_min, kInf, out);
            return;
        }
    }
    if constexpr ((F & kFeatAnalytic) != 0u) intersect_at<true>(sc, i, r, t_min, kInf, out);
}
template <class S, uint32_t I>
__device__ __forceinline__ void attributes_at(const S& sc, UC<I> ii, const Ray& r, float t_min, float t, uint32_t sub,
                                              Hit& out) {
    constexpr uint32_t kind = prim_kind<S, I>();
    if constexpr (kind == RRTE_PRIM_SDF)
        sdf_hit_attributes(SdfStaticProgram<S, prim_first<S, I>(), prim_count<S, I>()>{sc}, r, t, out);
    else if constexpr (kind == RRTE_PRIM_MESH)
        mesh_tri_hit(sc.mesh, sub, r, t_min, kInf, out);
    else if constexpr (kind == RRTE_PRIM_MESH_INSTANCE)
        mesh_instance_hit(prim_at(sc, ii), sc.mesh, sub, r, t_min, kInf, out);
    else if constexpr (kind == RRTE_PRIM_SPHERE)
        sphere_attributes(prim_at(sc, ii), r, t, out);
    else
        intersect_at<true>(sc, ii, r, t_min, kInf, out);
}

template <class S>
__device__ __forceinline__ void hit_attributes(const S& sc, const Ray& r, float t_min, int idx, float t, uint32_t sub,
                                               Hit& out) {
    if constexpr (S::kStatic) {
        for_each_prim(sc, [&](auto ii) {
            const uint32_t i = ii;
            if (__any((uint32_t)idx == i)) {
                if ((uint32_t)idx == i) attributes_at(sc, ii, r, t_min, t, sub, out);
            }
        });
    } else {
        bool pending = idx >= 0;
        while (pending) {
            const uint32_t i = __builtin_amdgcn_readfirstlane((uint32_t)idx);
            if ((uint32_t)idx == i) {
                attributes_at(sc, i, r, t_min, t, sub, out);
                pending = false;
            }
        }
    }
}

template <class S>
__device__ __forceinline__ int closest_hit(const S& sc, const Ray& r, float t_min, Hit& best, uint32_t pmask = ~0u,
                                           bool attributes = true) {
    float t;
    uint32_t sub;
    int idx = closest_t(sc, r, t_min, t, sub, pmask);
    if (attributes) hit_attributes(sc, r, t_min, idx, t, sub, best);
    return idx;
}

// Any-hit form of intersect_at (meshes stop at their first triangle hit).
template <class S>
__device__ __forceinline__ bool any_hit_at(const S& sc, uint32_t i, const Ray& r, float t_min, float t_max, Hit& h) {
    return intersect_at<false, S, true>(sc, i, r, t_min, t_max, h);
}
template <class S, uint32_t I>
__device__ __forceinline__ bool any_hit_at(const S& sc, UC<I> ii, const Ray& r, float t_min, float t_max, Hit& h) {
    return intersect_at<false, S, I, true>(sc, ii, r, t_min, t_max, h);
}

// Any hit in [t_min, t_max] (LAMBERT_SHADOW shadow rays).
template <class S>
__device__ __forceinline__ bool occluded(const S& sc, const Ray& r, float t_min, float t_max, uint64_t mask,
                                         int self = -1) {
    bool hit_any = false;
    for_each_prim(sc, [&](auto ii) {
        const uint32_t i = ii;
        // one wave-uniform skip test: culled, or every lane already occluded (mask cleared)
        if (mask == 0 || (i < 64u && !((mask >> i) & 1ull))) return;
        Hit h;
        if (!hit_any && (int)i != self && any_hit_at(sc, ii, r, t_min, t_max, h)) hit_any = true;
        if (__all(hit_any)) mask = 0;
    });
    return hit_any;
}

}  // namespace rrte
