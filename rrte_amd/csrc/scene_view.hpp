// scene_view.hpp — how device code sees a scene (bottom of the device-header stack).
//
// The runtime scene (SceneView: device pointers and counts, with the feature sets kFeat* the generic
// kernel is compiled for), the mesh buffers (MeshView), and what lets the same code run over a
// scene-specialised kernel's compile-time scene: UC / static_for, for_each_prim / for_each_light, the
// topology records (Topo*, SceneValues), load_uniform and the record accessors prim_at / light_at.
//
// Includes device_scene.hpp (records, vector and rounding helpers).  Included by sdf_eval.hpp,
// mesh_walk.hpp and pixel_encode.hpp.  Embedded for hiprtc (the Makefile's DEVICE_HDR).
#pragma once

#include "device_scene.hpp"

namespace rrte {

constexpr float kInf = __builtin_huge_valf();
constexpr uint32_t kCounterShards = 256;  // shadow-ray counter shards (power of two)
constexpr uint32_t kCounterStride = 16;   // u64 per shard: one 128-B line each

// Runtime scene: device pointers + counts (the generic kernel).  A
// scene-specialised kernel (jit.cpp, hiprtc) instead passes a struct whose
// members are static constexpr arrays and counts: the same device code below
// then fully unrolls its object / node / light loops and folds every scene
// constant into the instruction stream.
// Triangle-mesh data (RRTE_PRIM_MESH), built once per scene on the host (bvh.hip).  A link is an
// interior record index (bit 31 clear) or a leaf (bit 31 set, triangle count - 1 in bits 24-30,
// first triangle slot in bits 0-23).  Interior record k = nodes[4k..4k+3]: child 0 box min (w =
// child 0 link), child 0 box max (w = split axis), child 1 box min (w = child 1 link), child 1 box
// max.  Triangle slot k = tris[3k..3k+2]: v0 (w = the triangle's index within its mesh), e1 = v1-v0,
// e2 = v2-v0; norms[3k..3k+2] = vertex normals.  perm maps (mesh's first slot + original index) ->
// slot, for the original-order scan.
struct MeshView {
    const float4* __restrict__ nodes;
    const float4* __restrict__ tris;
    const float4* __restrict__ norms;
    const uint32_t* __restrict__ perm;
};

// Scene features the generic kernel is compiled for (SceneView::kFeat): the host picks the smallest
// precompiled variant whose features cover the scene (rrte_hip.hip generic_kernel), so a scene without
// meshes, deformers or non-sphere analytic objects runs a kernel without their code -- fewer live
// registers, a higher occupancy, no traversal stack in LDS.  Spheres are always compiled in.
constexpr uint32_t kFeatMesh = 1u;      // RRTE_PRIM_MESH objects (BVH traversal, LDS stack)
constexpr uint32_t kFeatDeform = 2u;    // SDF programs with deformers (bend, twist, taper, noise, wave)
constexpr uint32_t kFeatAnalytic = 4u;  // plane, triangle, cube, cylinder, cone, capsule
constexpr uint32_t kFeatSdf = 8u;       // SDF objects
constexpr uint32_t kFeatAll = 15u;
// RRTE_PRIM_MESH_INSTANCE objects (a mesh range placed through xf/inv).  Not part of kFeatAll: only a
// scene that holds an instance runs a variant with the instance path, so every other scene keeps the
// kernels (and their register budgets) it had before instances existed.
constexpr uint32_t kFeatInstance = 16u;
constexpr uint32_t kFeatEvery = kFeatAll | kFeatInstance;

struct SceneView {
    static constexpr bool kStatic = false;
    static constexpr bool kTopo = false;
    static constexpr uint32_t kFeat = kFeatAll;
    const DPrim* __restrict__ prims;
    const DMaterial* __restrict__ mats;
    const DLight* __restrict__ lights;
    const rrte_sdf_node* __restrict__ nodes;
    uint32_t num_prims, num_lights, num_materials;
    MeshView mesh;
};
template <uint32_t F>
struct SceneViewF : SceneView {
    static constexpr uint32_t kFeat = F;
};

// Loop over objects / lights: a plain loop for the runtime scene, compile-time
// recursion (every index a constant) for a static scene, so that the object's
// record, kind and SDF program fold into the code.
template <uint32_t V>
struct UC {
    static constexpr uint32_t value = V;
    __device__ __forceinline__ constexpr operator uint32_t() const { return V; }
};
template <uint32_t I, uint32_t N, class F>
__device__ __forceinline__ void static_for(F& f) {
    if constexpr (I < N) {
        f(UC<I>{});
        static_for<I + 1, N>(f);
    }
}
// The ten SDF leaf kinds (RRTE_SDF_SPHERE .. RRTE_SDF_ELLIPSOID) as compile-time constants.
template <class F>
__device__ __forceinline__ void static_for_leaves(F& f) {
    static_for<RRTE_SDF_SPHERE, RRTE_SDF_ELLIPSOID + 1u>(f);
}
template <class S, class F>
__device__ __forceinline__ void for_each_prim(const S& sc, F&& f) {
    if constexpr (S::kStatic) {
        static_for<0, S::num_prims>(f);
    } else {
        for (uint32_t i = 0; i < sc.num_prims; ++i) f(i);
    }
}
// Scene-specialised kernels come in two kinds (jit.hip).  FULL (S::kTopo false): every scene record
// is a static constexpr array, so all scene constants fold into the code.  TOPOLOGY (S::kTopo true):
// only the scene's structure is compile-time -- object kinds, materials and SDF node ranges, node
// ops, integer arguments and CSG-guard links, light kinds, the convexity and cullability decisions
// (TopoPrim / TopoNode / TopoLight) -- while positions, sizes, matrices, colours and intensities are
// read from the uploaded scene records with wave-uniform (scalar) loads, so moving or recolouring an
// object needs no recompile.  The accessors below give both kinds the same interface.
struct TopoPrim { uint32_t kind; uint32_t sdf_first, sdf_count; bool convex; };
struct TopoNode { uint32_t op; uint32_t i[3]; };
struct TopoLight { uint32_t kind; bool cullable; };
// The uploaded records a topology kernel reads (a kernel argument).
struct SceneValues {
    const DPrim* prims;
    const DMaterial* mats;
    const DLight* lights;
    const rrte_sdf_node* nodes;
};

// A record of the uploaded scene read through the constant address space: a topology kernel's records
// are wave-uniform and read-only, but the compiler cannot prove that for plain global loads in a kernel
// that also stores (it issued them as vector loads: 0.10 -> 0.72 M VMEM reads per 1080p launch against
// the full kernel); loads from address space 4 at a uniform address are scalar loads.  Word-wise, so
// that only the words used are loaded.
template <class T>
__device__ __forceinline__ T load_uniform(const T* p) {
    static_assert(sizeof(T) % 4u == 0u, "records are whole dwords");
    typedef const __attribute__((address_space(4))) uint32_t CWord;
    CWord* w = (CWord*)p;
    T v;
    uint32_t* d = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
    for (uint32_t k = 0; k < sizeof(T) / 4u; ++k) d[k] = w[k];
    return v;
}
struct NodeArgs { float f[12]; };

// Scene record accessors.  For a full static scene the record is copied in a
// constexpr-expression context (constexpr local): device-side copies of
// constexpr globals may be emitted as externally-initialised memory whose
// loads do not fold, while a constexpr copy always does.  For a topology scene
// the record is loaded and its structural fields replaced by their compile-time values.
template <class S>
__device__ __forceinline__ const DPrim& prim_at(const S& sc, uint32_t i) { return sc.prims[i]; }
template <class S, uint32_t I>
constexpr uint32_t prim_kind() {
    if constexpr (S::kTopo) return S::topo_prims[I].kind;
    else return S::prims[I].kind;
}
template <class S, uint32_t I>
constexpr uint32_t prim_first() {
    if constexpr (S::kTopo) return S::topo_prims[I].sdf_first;
    else return S::prims[I].sdf_first;
}
template <class S, uint32_t I>
constexpr uint32_t prim_count() {
    if constexpr (S::kTopo) return S::topo_prims[I].sdf_count;
    else return S::prims[I].sdf_count;
}
template <class S, uint32_t I>
__device__ __forceinline__ DPrim prim_at(const S& sc, UC<I>) {
    if constexpr (S::kTopo) {
        constexpr TopoPrim tp = S::topo_prims[I];
        DPrim v = load_uniform(sc.prims + I);
        v.kind = tp.kind;
        v.sdf_first = tp.sdf_first;
        v.sdf_count = tp.sdf_count;
        return v;
    } else {
        constexpr DPrim v = S::prims[I];
        return v;
    }
}
template <class S>
__device__ __forceinline__ const DLight& light_at(const S& sc, uint32_t i) { return sc.lights[i]; }
template <class S, uint32_t I>
constexpr uint32_t light_kind() {
    if constexpr (S::kTopo) return S::topo_lights[I].kind;
    else return S::lights[I].kind;
}
template <class S, uint32_t I>
__device__ __forceinline__ DLight light_at(const S& sc, UC<I>) {
    if constexpr (S::kTopo) {
        DLight v = load_uniform(sc.lights + I);
        v.kind = light_kind<S, I>();
        return v;
    } else {
        constexpr DLight v = S::lights[I];
        return v;
    }
}

template <class S, class F>
__device__ __forceinline__ void for_each_light(const S& sc, F&& f) {
    if constexpr (S::kStatic) {
        static_for<0, S::num_lights>(f);
    } else {
#pragma unroll 1
        for (uint32_t i = 0; i < sc.num_lights; ++i) f(i);
    }
}

}  // namespace rrte
