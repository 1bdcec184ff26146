// mesh_build.hip — device-side build of the mesh BVHs (include/rrte_hip_build.h).
//
// An LBVH with 4-triangle leaves over every distinct range of the scene at once:
//
//   lbvh_keys       one thread per triangle: its centre's Morton cell in its range's centroid box,
//                   key (range ordinal << 32 | morton), value = its position in index order;
//   (radix sort)    rocprim, stable: a range's slots are its triangles in (morton, index) order;
//   lbvh_slots      one thread per sorted slot: the slot's original index (tris[3k].w), perm, the
//                   slot's three vertex indices, and the key of the leaf a slot starts;
//   lbvh_hierarchy  one thread per record: Karras' radix tree over its range's leaf keys: both
//                   child links, the axis word, and its children's parent codes;
//   lbvh_depths     one thread per record: the parent walk, a per-depth histogram and the maximum;
//   lbvh_order      one thread per record: its place among the records of its depth;
//   (refit kernels) leaves, then records level by level, deepest first (mesh_refit.hip): every
//                   triangle record and every box, by the statements a refit runs.
//
// No kernel reads what another workgroup of the same launch wrote: each stage is a launch, and the
// only shared words are integer atomics (histogram, maximum, per-level cursors) read by later
// launches or by the host.  The host waits twice on the upload stream: for the level counts before
// it can launch the level kernels, and for the read-back.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "mesh_build.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>

#include "mesh_box.hpp"
#include "mesh_refit.hpp"

namespace rrte {
namespace {

constexpr uint32_t kBuildBlock = 64;
constexpr uint32_t kStatsWords = 2u * kLbvhWalkCap + 1u;  // histogram, level cursors, maximum depth

// parts of the scratch allocation
enum : int {
    P_VERTS, P_INDICES, P_RANGES, P_KEYS_IN, P_KEYS_OUT, P_VALS_IN, P_VALS_OUT, P_SORT_TEMP, P_LEAF_KEYS, P_SLOT_VTX,
    P_LEAVES, P_PARENT, P_DEPTH, P_ORDER, P_STATS, P_NODES, P_TRIS, P_NORMS, P_PERM, P_COUNT
};
static_assert(P_COUNT == kBuildParts, "DeviceBuilder::off_ holds one offset per part and the end");

struct BuildDevice {
    const float2* verts;  // rrte_mesh_vertex as 3 x float2
    const uint32_t* indices;
    const BuildRange* ranges;
    uint64_t* keys_in;
    uint64_t* keys_out;
    uint32_t* vals_in;
    uint32_t* vals_out;
    uint64_t* leaf_keys;
    uint32_t* slot_vtx;
    uint2* leaves;
    uint32_t* parent;
    uint32_t* depth;
    uint2* order;
    uint32_t* stats;  // [0, 64) records per depth, [64, 128) level cursors, [128] the maximum depth
    float4* nodes;
    float4* tris;
    uint32_t* perm;
    uint32_t n_ranges, n_verts, n_indices, n_tris, n_leaves, n_recs;
    unsigned long long* check;  // RRTE_DEBUG bit 2: bit 128 a slot, triangle or vertex index out of range, 256 a record
};

struct LevelTable {
    uint32_t off[kLbvhWalkCap + 1];
    uint32_t max_depth;
};

// The last range whose base (slot_base or rec_base) is <= i: empty ranges share their base with the next one.
template <uint32_t BuildRange::*Base>
__device__ inline uint32_t range_of(const BuildRange* ranges, uint32_t n, uint32_t i) {
    uint32_t lo = 0, hi = n;
    for (int it = 0; it < 32; ++it) {
        if (hi - lo <= 1u) break;
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (ranges[mid].*Base <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ inline bool flag(const BuildDevice& d, uint32_t bad) {
    if (bad) atomicOr(d.check, (unsigned long long)bad);
    return bad != 0u;
}

__global__ __launch_bounds__(kBuildBlock) void lbvh_keys(BuildDevice d) {
    const uint32_t g = blockIdx.x * kBuildBlock + threadIdx.x;
    if (g >= d.n_tris) return;
    const uint32_t r = range_of<&BuildRange::slot_base>(d.ranges, d.n_ranges, g);
    const BuildRange R = d.ranges[r];
    const uint32_t k = g - R.slot_base;
    const size_t i0 = ((size_t)R.first + k) * 3u;
    if (d.check) {
        uint32_t bad = (k >= R.count || i0 + 3u > d.n_indices) ? 128u : 0u;
        if (!bad)
            for (int j = 0; j < 3; ++j)
                if (d.indices[i0 + j] >= d.n_verts) bad = 128u;
        if (flag(d, bad)) return;
    }
    Box tb;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float2* v = d.verts + (size_t)d.indices[i0 + j] * 3u;
        const float2 v0 = v[0], v1 = v[1];
        const float p[3] = {v0.x, v0.y, v1.x};
        tb.grow(p);
    }
    uint32_t q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float c = 0.5f * (tb.lo[a] + tb.hi[a]);
        q[a] = lbvh_cell(c, R.cb_lo[a], R.cb_ext[a]);
    }
    d.keys_in[g] = lbvh_tri_key(r, lbvh_morton(q[0], q[1], q[2]));
    d.vals_in[g] = g;
}

__global__ __launch_bounds__(kBuildBlock) void lbvh_slots(BuildDevice d) {
    const uint32_t s = blockIdx.x * kBuildBlock + threadIdx.x;
    if (s >= d.n_tris) return;
    const uint64_t key = d.keys_out[s];
    const uint32_t g = d.vals_out[s], r = (uint32_t)(key >> 32), morton = (uint32_t)key;
    if (d.check && flag(d, (r >= d.n_ranges || g >= d.n_tris) ? 128u : 0u)) return;
    const BuildRange R = d.ranges[r];
    const uint32_t o = g - R.slot_base, sl = s - R.slot_base;
    const size_t i0 = ((size_t)R.first + o) * 3u;
    if (d.check && flag(d, (o >= R.count || sl >= R.count || i0 + 3u > d.n_indices) ? 128u : 0u)) return;
    d.tris[3u * (size_t)s] = make_float4(0.0f, 0.0f, 0.0f, __builtin_bit_cast(float, o));
    d.perm[R.slot_base + o] = s;
#pragma unroll
    for (int j = 0; j < 3; ++j) d.slot_vtx[3u * (size_t)s + j] = d.indices[i0 + j];
    if (sl % kLbvhLeafMax == 0u) {
        const uint32_t j = sl / kLbvhLeafMax;
        d.leaf_keys[R.leaf_base + j] = lbvh_leaf_key(morton, j);
        if (R.leaves == 1u)  // the range's root is this leaf: no record
            d.leaves[R.leaf_base] = make_uint2(kLbvhLeafBit | ((R.count - 1u) << 24) | R.slot_base, kLbvhNoParent);
    }
}

__global__ __launch_bounds__(kBuildBlock) void lbvh_hierarchy(BuildDevice d) {
    const uint32_t i = blockIdx.x * kBuildBlock + threadIdx.x;
    if (i >= d.n_recs) return;
    const uint32_t r = range_of<&BuildRange::rec_base>(d.ranges, d.n_ranges, i);
    const BuildRange R = d.ranges[r];
    const uint32_t li = i - R.rec_base;
    if (d.check && flag(d, (R.leaves < 2u || li >= R.leaves - 1u || (uint64_t)R.leaf_base + R.leaves > d.n_leaves) ? 256u : 0u))
        return;
    const uint64_t* keys = d.leaf_keys + R.leaf_base;
    const LbvhNode nd = lbvh_node(keys, R.leaves, li);
    if (nd.first > nd.split || nd.split >= nd.last || nd.last >= R.leaves) {  // (keys out of order: cannot happen)
        if (d.check) flag(d, 256u);
        return;
    }
    uint32_t link[2];
#pragma unroll
    for (uint32_t side = 0; side < 2u; ++side) {
        const uint32_t a = side ? nd.split + 1u : nd.first, b = side ? nd.last : nd.split;
        const uint32_t code = i * 2u + side;
        if (a == b) {  // leaf a
            const uint32_t left = R.count - kLbvhLeafMax * a;
            const uint32_t cnt = left < kLbvhLeafMax ? left : kLbvhLeafMax;
            link[side] = kLbvhLeafBit | ((cnt - 1u) << 24) | (R.slot_base + kLbvhLeafMax * a);
            d.leaves[R.leaf_base + a] = make_uint2(link[side], code);
        } else {
            const uint32_t child = R.rec_base + (side ? nd.split + 1u : nd.split);
            if (d.check && flag(d, child >= d.n_recs ? 256u : 0u)) return;
            link[side] = child;
            d.parent[child] = code;
        }
    }
    const uint32_t axis = lbvh_axis(keys[nd.split], keys[nd.split + 1u]);
    float4* q = d.nodes + (size_t)i * 4u;
    q[0] = make_float4(0.0f, 0.0f, 0.0f, __builtin_bit_cast(float, link[0]));
    q[1] = make_float4(0.0f, 0.0f, 0.0f, __builtin_bit_cast(float, axis));
    q[2] = make_float4(0.0f, 0.0f, 0.0f, __builtin_bit_cast(float, link[1]));
    q[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (li == 0u) d.parent[i] = kLbvhNoParent;  // record 0 of a range is its root
}

// (every entry of d.parent is a code this build wrote or the no-parent word it was filled with)
__global__ __launch_bounds__(kBuildBlock) void lbvh_depths(BuildDevice d) {
    const uint32_t i = blockIdx.x * kBuildBlock + threadIdx.x;
    if (i >= d.n_recs) return;
    const uint32_t dep = lbvh_depth(d.parent, i);
    d.depth[i] = dep;
    if (dep < kLbvhWalkCap) atomicAdd(d.stats + dep, 1u);
    atomicMax(d.stats + 2u * kLbvhWalkCap, dep);
}

__global__ __launch_bounds__(kBuildBlock) void lbvh_order(BuildDevice d, LevelTable lt) {
    const uint32_t i = blockIdx.x * kBuildBlock + threadIdx.x;
    if (i >= d.n_recs) return;
    const uint32_t dep = d.depth[i];
    if (dep == 0u || dep > lt.max_depth) return;  // (a root has no parent slot to write)
    const uint32_t level = lt.max_depth - dep;    // deepest first
    const uint32_t pos = lt.off[level] + atomicAdd(d.stats + kLbvhWalkCap + level, 1u);
    if (pos >= lt.off[level + 1u]) {
        if (d.check) flag(d, 256u);
        return;
    }
    d.order[pos] = make_uint2(i, d.parent[i]);
}

inline uint32_t blocks(uint32_t n) { return (n + kBuildBlock - 1u) / kBuildBlock; }

inline double us_since(std::chrono::steady_clock::time_point& t) {
    const auto n = std::chrono::steady_clock::now();
    const double us = std::chrono::duration<double, std::micro>(n - t).count();
    t = n;
    return us;
}

}  // namespace

bool DeviceBuilder::plan(const rrte_scene_ir* s) {
    ranges_.clear();
    mesh_ranges_.clear();
    n_tris_ = n_leaves_ = n_recs_ = 0;
    uint64_t slots = 0;
    const std::vector<std::pair<uint32_t, uint32_t>> keys = mesh_ranges_of(s);
    for (const auto& key : keys) {
        if (key.second > (1u << 24)) return false;
        if (((uint64_t)key.first + key.second) * 3u > s->num_mesh_indices) return false;
        slots += key.second;
    }
    if (slots > (1u << 24)) return false;  // (a leaf link names its first slot in 24 bits)
    const rrte_mesh_vertex* vx = s->mesh_vertices;
    for (const auto& key : keys) {
        const uint32_t ntri = key.second;
        const uint32_t* ix = s->mesh_indices + (size_t)key.first * 3;
        // one pass: the finite scan, the box over the named vertices (the culling sphere's, as
        // refit_range_bounds computes it) and the exact centroid box
        Box nb, cb;
        for (uint32_t k = 0; k < ntri; ++k) {
            Box tb;
            for (int j = 0; j < 3; ++j) {
                const float* p = vx[ix[3 * k + j]].position;
                if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) return false;
                tb.grow(p);
                nb.grow(p);
            }
            float c[3];
            for (int a = 0; a < 3; ++a) c[a] = 0.5f * (tb.lo[a] + tb.hi[a]);
            cb.grow(c);
        }
        BuildRange R{};
        R.first = key.first;
        R.count = ntri;
        R.slot_base = n_tris_;
        R.leaf_base = n_leaves_;
        R.leaves = (ntri + kLbvhLeafMax - 1u) / kLbvhLeafMax;
        R.rec_base = n_recs_;
        for (int a = 0; a < 3; ++a) {
            R.cb_lo[a] = ntri ? cb.lo[a] : 0.0f;
            R.cb_ext[a] = ntri ? cb.hi[a] - cb.lo[a] : 0.0f;
        }
        MeshRange mr{};
        mr.first = key.first;
        mr.count = ntri;
        mr.slot_base = n_tris_;
        if (ntri == 0u) mr.root = kLbvhLeafBit;
        else if (R.leaves == 1u) mr.root = kLbvhLeafBit | ((ntri - 1u) << 24) | n_tris_;
        else mr.root = n_recs_;
        if (ntri) nb = inflate(nb);
        for (int a = 0; a < 3; ++a) {
            mr.lo[a] = nb.lo[a];
            mr.hi[a] = nb.hi[a];
        }
        n_tris_ += ntri;
        n_leaves_ += R.leaves;
        n_recs_ += R.leaves > 1u ? R.leaves - 1u : 0u;
        ranges_.push_back(R);
        mesh_ranges_.push_back(mr);
    }
    uint32_t bits = 32u;  // the Morton word, then as many bits as the range ordinals take
    while ((1ull << (bits - 32u)) < ranges_.size()) ++bits;
    if (n_tris_ && (n_tris_ != sort_n_ || bits != sort_bits_)) {  // (the same sort as last time needs the same space)
        sort_temp_ = 0;
        sort_bits_ = bits;
        sort_n_ = n_tris_;
        if (rocprim::radix_sort_pairs(nullptr, sort_temp_, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                      (uint32_t*)nullptr, (size_t)n_tris_, 0u, sort_bits_, (hipStream_t) nullptr) != hipSuccess)
            return sort_n_ = 0, false;
    }
    const size_t T = n_tris_, L = n_leaves_, N = n_recs_;
    const size_t bytes[P_COUNT] = {
        (size_t)s->num_mesh_vertices * sizeof(rrte_mesh_vertex), (size_t)s->num_mesh_indices * sizeof(uint32_t),
        ranges_.size() * sizeof(BuildRange), T * 8, T * 8, T * 4, T * 4, sort_temp_, L * 8, T * 12, L * sizeof(uint2), N * 4,
        N * 4, N * sizeof(uint2), kStatsWords * 4, N * 64, T * 48, T * 48, T * 4};
    total_ = 0;
    for (int i = 0; i < P_COUNT; ++i) {
        off_[i] = total_;
        total_ += (bytes[i] + 255u) & ~(size_t)255u;
    }
    off_[P_COUNT] = total_;
    total_ = std::max<size_t>(total_, 256u);
    return true;
}

BuildResult DeviceBuilder::run(const rrte_scene_ir* s, uint8_t* scratch, hipStream_t st, unsigned long long* check,
                               MeshData& out, uint32_t* depth, hipError_t* err, BuildTimes* times) {
    auto t = std::chrono::steady_clock::now();
    *depth = 0;
    *err = hipSuccess;
#define BUILD_TRY(x)                      \
    do {                                  \
        const hipError_t e_ = (x);        \
        if (e_ != hipSuccess) {           \
            *err = e_;                    \
            (void)hipStreamSynchronize(st); /* copies queued into `out` or `stats` end before they go */ \
            return BuildResult::HipError; \
        }                                 \
    } while (0)
    const uint32_t T = n_tris_, L = n_leaves_, N = n_recs_;
    uint32_t max_depth = 0;
    if (T) {
        BuildDevice d{};
        d.verts = reinterpret_cast<const float2*>(scratch + off_[P_VERTS]);
        d.indices = reinterpret_cast<const uint32_t*>(scratch + off_[P_INDICES]);
        d.ranges = reinterpret_cast<const BuildRange*>(scratch + off_[P_RANGES]);
        d.keys_in = reinterpret_cast<uint64_t*>(scratch + off_[P_KEYS_IN]);
        d.keys_out = reinterpret_cast<uint64_t*>(scratch + off_[P_KEYS_OUT]);
        d.vals_in = reinterpret_cast<uint32_t*>(scratch + off_[P_VALS_IN]);
        d.vals_out = reinterpret_cast<uint32_t*>(scratch + off_[P_VALS_OUT]);
        d.leaf_keys = reinterpret_cast<uint64_t*>(scratch + off_[P_LEAF_KEYS]);
        d.slot_vtx = reinterpret_cast<uint32_t*>(scratch + off_[P_SLOT_VTX]);
        d.leaves = reinterpret_cast<uint2*>(scratch + off_[P_LEAVES]);
        d.parent = reinterpret_cast<uint32_t*>(scratch + off_[P_PARENT]);
        d.depth = reinterpret_cast<uint32_t*>(scratch + off_[P_DEPTH]);
        d.order = reinterpret_cast<uint2*>(scratch + off_[P_ORDER]);
        d.stats = reinterpret_cast<uint32_t*>(scratch + off_[P_STATS]);
        d.nodes = reinterpret_cast<float4*>(scratch + off_[P_NODES]);
        d.tris = reinterpret_cast<float4*>(scratch + off_[P_TRIS]);
        d.perm = reinterpret_cast<uint32_t*>(scratch + off_[P_PERM]);
        d.n_ranges = (uint32_t)ranges_.size();
        d.n_verts = s->num_mesh_vertices;
        d.n_indices = s->num_mesh_indices;
        d.n_tris = T;
        d.n_leaves = L;
        d.n_recs = N;
        d.check = check;
        BUILD_TRY(hipMemcpyAsync(scratch + off_[P_VERTS], s->mesh_vertices, (size_t)s->num_mesh_vertices * sizeof(rrte_mesh_vertex),
                                 hipMemcpyHostToDevice, st));
        BUILD_TRY(hipMemcpyAsync(scratch + off_[P_INDICES], s->mesh_indices, (size_t)s->num_mesh_indices * sizeof(uint32_t),
                                 hipMemcpyHostToDevice, st));
        BUILD_TRY(hipMemcpyAsync(scratch + off_[P_RANGES], ranges_.data(), ranges_.size() * sizeof(BuildRange),
                                 hipMemcpyHostToDevice, st));
        // the no-parent word everywhere (the parent walk then ends whatever happens), zeroed statistics, and
        // zeroed leaf entries (slot 0, record 0: in range wherever a record exists)
        BUILD_TRY(hipMemsetAsync(scratch + off_[P_PARENT], 0xFF, off_[P_DEPTH] - off_[P_PARENT], st));
        BUILD_TRY(hipMemsetAsync(scratch + off_[P_STATS], 0, kStatsWords * 4, st));
        BUILD_TRY(hipMemsetAsync(scratch + off_[P_LEAVES], 0, off_[P_PARENT] - off_[P_LEAVES], st));
        hipLaunchKernelGGL(lbvh_keys, dim3(blocks(T)), dim3(kBuildBlock), 0, st, d);
        BUILD_TRY(hipGetLastError());
        size_t temp = sort_temp_;
        BUILD_TRY(rocprim::radix_sort_pairs(scratch + off_[P_SORT_TEMP], temp, (const uint64_t*)d.keys_in, d.keys_out,
                                            (const uint32_t*)d.vals_in, d.vals_out, (size_t)T, 0u, sort_bits_, st));
        hipLaunchKernelGGL(lbvh_slots, dim3(blocks(T)), dim3(kBuildBlock), 0, st, d);
        BUILD_TRY(hipGetLastError());
        uint32_t stats[kStatsWords] = {};
        if (N) {
            hipLaunchKernelGGL(lbvh_hierarchy, dim3(blocks(N)), dim3(kBuildBlock), 0, st, d);
            BUILD_TRY(hipGetLastError());
            hipLaunchKernelGGL(lbvh_depths, dim3(blocks(N)), dim3(kBuildBlock), 0, st, d);
            BUILD_TRY(hipGetLastError());
            BUILD_TRY(hipMemcpyAsync(stats, d.stats, sizeof stats, hipMemcpyDeviceToHost, st));
            if (times) times->enqueue += us_since(t);
            BUILD_TRY(hipStreamSynchronize(st));
            if (times) times->depth_wait += us_since(t);
            max_depth = stats[2u * kLbvhWalkCap];
            *depth = max_depth + 1u;  // records on the deepest record's path, itself included
            if (*depth > kLbvhMaxRecords) return BuildResult::Fallback;
        } else if (times) {
            times->enqueue += us_since(t);
        }
        LevelTable lt{};
        lt.max_depth = max_depth;
        for (uint32_t l = 0; l < max_depth; ++l) lt.off[l + 1] = lt.off[l] + stats[max_depth - l];
        if (N && lt.off[max_depth] + stats[0] != N) return BuildResult::Fallback;  // (not a forest over the records)
        if (max_depth) {
            hipLaunchKernelGGL(lbvh_order, dim3(blocks(N)), dim3(kBuildBlock), 0, st, d, lt);
            BUILD_TRY(hipGetLastError());
        }
        RefitDevice rd{};
        rd.nodes = d.nodes;
        rd.tris = d.tris;
        rd.norms = reinterpret_cast<float4*>(scratch + off_[P_NORMS]);
        rd.verts = d.verts;
        rd.slot_vtx = d.slot_vtx;
        rd.leaves = d.leaves;
        rd.order = d.order;
        rd.n_verts = d.n_verts;
        rd.n_slots = T;
        rd.n_recs = N;
        rd.check = check;
        BUILD_TRY(launch_refit_levels(L, lt.off, max_depth, rd, st));
        out.nodes.resize((size_t)N * 4);
        out.tris.resize((size_t)T * 3);
        out.norms.resize((size_t)T * 3);
        out.perm.resize(T);
        if (N) BUILD_TRY(hipMemcpyAsync(out.nodes.data(), d.nodes, (size_t)N * 64, hipMemcpyDeviceToHost, st));
        BUILD_TRY(hipMemcpyAsync(out.tris.data(), d.tris, (size_t)T * 48, hipMemcpyDeviceToHost, st));
        BUILD_TRY(hipMemcpyAsync(out.norms.data(), rd.norms, (size_t)T * 48, hipMemcpyDeviceToHost, st));
        BUILD_TRY(hipMemcpyAsync(out.perm.data(), d.perm, (size_t)T * 4, hipMemcpyDeviceToHost, st));
        if (times) times->boxes_enqueue += us_since(t);
        BUILD_TRY(hipStreamSynchronize(st));
        if (times) times->readback += us_since(t);
    }
#undef BUILD_TRY
    out.ranges = mesh_ranges_;
    out.max_depth = *depth;
    out.too_deep = false;
    if (times) ++times->n;
    return BuildResult::Built;
}

}  // namespace rrte
