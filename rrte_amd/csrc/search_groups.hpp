// search_groups.hpp — the object searches of a scene-specialised kernel, with grouped skip tests
// (DESIGN.md §21).
//
// search.hpp's occluded() and closest_t() visit every object of a static scene with a compile-time
// index and step over the ones the wave's cull removed: one wave-uniform test and branch per object
// -- on the 64-bit shadow mask four scalar instructions, 51 times per ray of the headline (17 objects,
// 3 lights), nearly all of them taken.  The searches below are the same searches -- every object whose
// mask bit is set runs its exact intersector, in index order, with the same arguments, so frames and
// shadow counts are bit for bit what they were -- with less scalar work around them:
//   * a scene of at most 32 objects keeps each light's mask in 32 bits;
//   * the objects are cut into groups of RRTE_SEARCH_GROUPS consecutive indices and a group none of
//     whose bits is set is stepped over with one test (a mask that holds only the ground passes 11 of
//     the headline's 16 SDF objects in two tests);
//   * once every executing lane is occluded the cleared mask fails one test per remaining group, where
//     the template fell through one per remaining object.  (A `return` at that point was tried: the
//     compiler then carries an exit flag through every skip path, three more scalar instructions per
//     stepped-over group -- dearer than the tests it saves in the rare wave that gets there.)
// Objects without a mask bit (index >= 64 for the shadow mask, >= 32 for the camera mask) are never
// skipped, as before; a shadow mask of zero skips every object, as before.
//
// An embedded header like the others (the Makefile's DEVICE_HDR), but included by the generated source,
// not by ray_kernels.hpp: jit.hip's jit_source emits its #include right after the definition of
// rrte_jit::Scene, which the searches below name.  They are non-template overloads on rrte_jit::Scene:
// closest_hit() and shade_lambert() reach them through argument-dependent lookup and prefer them to
// search.hpp's templates, the way accel_kernels.hpp reaches the generic kernel.  Includes nothing (the
// source has included ray_kernels.hpp by then).
// -DRRTE_SEARCH_GROUPS=0 (RRTE_JIT_EXTRA_OPTS) leaves the templates in charge (A/B).
#ifndef RRTE_SEARCH_GROUPS
#define RRTE_SEARCH_GROUPS 6  // objects per group (3, 4, 6, 8 measured on the headline: DESIGN.md §21)
#endif
#if RRTE_SEARCH_GROUPS > 0
namespace rrte {
namespace search {

constexpr uint32_t kGroup = RRTE_SEARCH_GROUPS;

template <bool NARROW> struct MaskOf { typedef uint64_t type; };
template <> struct MaskOf<true> { typedef uint32_t type; };

// The bits of objects [lo, hi) in a mask of type M (an index past the mask's width has no bit).
template <class M>
constexpr M bits_of(uint32_t lo, uint32_t hi) {
    M m = 0;
    for (uint32_t i = lo; i < hi && i < 8u * sizeof(M); ++i) m |= (M)1 << i;
    return m;
}

// Objects [I, E) of one shadow group (SOLO: a group of one, whose group test was the object's test).
// Once every executing lane is occluded the mask is cleared: the rest of this group and every later
// group then fail their tests.
template <uint32_t I, uint32_t E, bool SOLO, class S, class M>
__device__ __forceinline__ void occluded_objects(const S& sc, const Ray& r, float t_min, float t_max, M& mask, int self,
                                                 bool& hit_any) {
    if constexpr (I < E) {
        if (SOLO ? true : I >= 8u * sizeof(M) ? mask != 0 : ((mask >> I) & (M)1) != 0) {
            Hit h;
            if (!hit_any && (int)I != self && any_hit_at(sc, UC<I>{}, r, t_min, t_max, h)) hit_any = true;
            if (__all(hit_any)) mask = 0;
        }
        occluded_objects<I + 1u, E, SOLO>(sc, r, t_min, t_max, mask, self, hit_any);
    }
}
template <uint32_t G, class S, class M>
__device__ __forceinline__ void occluded_groups(const S& sc, const Ray& r, float t_min, float t_max, M& mask, int self,
                                                bool& hit_any) {
    constexpr uint32_t lo = G * kGroup, hi = lo + kGroup < S::num_prims ? lo + kGroup : S::num_prims;
    if constexpr (lo < S::num_prims) {
        constexpr M gbits = bits_of<M>(lo, hi);
        if (hi > 8u * sizeof(M) ? mask != 0 : (mask & gbits) != 0)
            occluded_objects<lo, hi, hi - lo == 1u>(sc, r, t_min, t_max, mask, self, hit_any);
        occluded_groups<G + 1u>(sc, r, t_min, t_max, mask, self, hit_any);
    }
}

struct Best {
    int idx;
    float t;
    uint32_t sub;
};
// closest_t's step for objects [I, E) of one group: the template's body.
template <uint32_t I, uint32_t E, bool SOLO, class S>
__device__ __forceinline__ void closest_objects(const S& sc, const Ray& r, float t_min, uint32_t pmask, Best& b) {
    if constexpr (I < E) {
        if (SOLO || I >= 32u || ((pmask >> I) & 1u) != 0u) {
            Hit h;
            h.sub = 0u;
            float tmax = (prim_at(sc, UC<I>{}).kind == RRTE_PRIM_SDF && b.idx >= 0) ? b.t : kInf;
            if (intersect_at<false>(sc, UC<I>{}, r, t_min, tmax, h)) {
                if (b.idx < 0 || h.t < b.t || (h.t == b.t && (int)I < b.idx)) {
                    b.t = h.t;
                    b.sub = h.sub;
                    b.idx = (int)I;
                }
            }
        }
        closest_objects<I + 1u, E, SOLO>(sc, r, t_min, pmask, b);
    }
}
template <uint32_t G, class S>
__device__ __forceinline__ void closest_groups(const S& sc, const Ray& r, float t_min, uint32_t pmask, Best& b) {
    constexpr uint32_t lo = G * kGroup, hi = lo + kGroup < S::num_prims ? lo + kGroup : S::num_prims;
    if constexpr (lo < S::num_prims) {
        constexpr uint32_t gbits = bits_of<uint32_t>(lo, hi);
        if (hi > 32u || (pmask & gbits) != 0u) closest_objects<lo, hi, hi - lo == 1u>(sc, r, t_min, pmask, b);
        closest_groups<G + 1u>(sc, r, t_min, pmask, b);
    }
}

}  // namespace search

// closest_t of search.hpp for the specialised scene: strict '<', equal t to the lower index.
__device__ __forceinline__ int closest_t(const rrte_jit::Scene& sc, const Ray& r, float t_min, float& best_t,
                                         uint32_t& best_sub, uint32_t pmask = ~0u) {
    search::Best b{-1, kInf, 0u};
    search::closest_groups<0u>(sc, r, t_min, pmask, b);
    best_t = b.t;
    best_sub = b.sub;
    return b.idx;
}

// occluded of search.hpp for the specialised scene.
__device__ __forceinline__ bool occluded(const rrte_jit::Scene& sc, const Ray& r, float t_min, float t_max, uint64_t mask,
                                         int self = -1) {
    typedef search::MaskOf<(rrte_jit::Scene::num_prims <= 32u)>::type M;
    bool hit_any = false;
    M m = (M)mask;
    search::occluded_groups<0u>(sc, r, t_min, t_max, m, self, hit_any);
    return hit_any;
}

}  // namespace rrte
#endif  // RRTE_SEARCH_GROUPS > 0
