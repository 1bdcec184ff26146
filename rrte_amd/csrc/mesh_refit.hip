// mesh_refit.hip — device-side refit of the mesh BVHs after a deformation.
//
// A deformation keeps the topology: the indices, the tree shape and every leaf's contents.  What
// changes are the triangle records (v0, e1, e2, normals), the boxes and the culling spheres.  The
// scene version's upload copies the stored (stale) mesh data -- its links and w words are what the
// refit keeps -- and these kernels, on the upload stream behind that copy, overwrite the rest from
// the new vertices, bottom-up:
//
//   refit_leaves  one thread per leaf: rewrites its triangle slots and stores the leaf's inflated
//                 box into its parent record's child slot;
//   refit_level   once per depth, deepest first: one thread per record unions its two child boxes
//                 into its parent's child slot.  Ordering between levels is the kernel boundary.
//
// Same f32 operations as build_mesh_ranges, in the same order (mesh_box.hpp), so a refit of unchanged
// vertices reproduces the built data bit for bit.  Leaf boxes come from the vertex positions.
#include "mesh_refit.hpp"

#include <algorithm>
#include <cstring>

#include "mesh_box.hpp"

namespace rrte {
namespace {

constexpr uint32_t kLeafBit = 0x80000000u;  // bvh.hip: leaf link = bit 31, count - 1 in 24-30, first slot in 0-23
constexpr uint32_t kRefitBlock = 64;

__host__ __device__ inline uint32_t leaf_first(uint32_t link) { return link & 0xFFFFFFu; }
__host__ __device__ inline uint32_t leaf_count(uint32_t link) { return ((link >> 24) & 0x7Fu) + 1u; }

// Stores `b` into the child slot `code` (record * 2 + side) names, keeping the slot's w words (link; axis).
__host__ __device__ inline void store_child(float4* nodes, uint32_t code, const Box& b) {
    float4* q = nodes + (size_t)(code >> 1) * 4u + (code & 1u) * 2u;
    const float w0 = reinterpret_cast<const float*>(q)[3], w1 = reinterpret_cast<const float*>(q + 1)[3];
    q[0] = make_float4(b.lo[0], b.lo[1], b.lo[2], w0);
    q[1] = make_float4(b.hi[0], b.hi[1], b.hi[2], w1);
}

// Leaf i: its triangle slots from the vertices, its inflated box into its parent's child slot.
// (Host-callable so that a CPU driver can run the same statements; the library calls it on the device only.)
__host__ __device__ inline void refit_leaf(const RefitDevice& d, uint32_t i) {
    const uint2 lf = d.leaves[i];
    const uint32_t a = leaf_first(lf.x), n = leaf_count(lf.x);
    Box nb;
    for (uint32_t k = a; k < a + n; ++k) {
        float p[3][3];
        Box tb;
        float4 nr[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float2* v = d.verts + (size_t)d.slot_vtx[3u * k + j] * 3u;
            const float2 v0 = v[0], v1 = v[1], v2 = v[2];  // position xyz, normal xyz
            p[j][0] = v0.x;
            p[j][1] = v0.y;
            p[j][2] = v1.x;
            nr[j] = make_float4(v1.y, v2.x, v2.y, 0.0f);
            tb.grow(p[j]);
        }
        nb.grow(tb);
        const float w = reinterpret_cast<const float*>(d.tris + 3u * (size_t)k)[3];  // the original index
        d.tris[3u * (size_t)k] = make_float4(p[0][0], p[0][1], p[0][2], w);
        d.tris[3u * (size_t)k + 1] = make_float4(p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2], 0.0f);
        d.tris[3u * (size_t)k + 2] = make_float4(p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2], 0.0f);
        d.norms[3u * (size_t)k] = nr[0];
        d.norms[3u * (size_t)k + 1] = nr[1];
        d.norms[3u * (size_t)k + 2] = nr[2];
    }
    if (lf.y != kRefitRoot) store_child(d.nodes, lf.y, inflate(nb));  // (a root leaf has no record)
}

// Record rc.x: the union of its two child boxes into its parent's child slot rc.y.
__host__ __device__ inline void refit_record(const RefitDevice& d, uint2 rc) {
    const float4* q = d.nodes + (size_t)rc.x * 4u;
    const float4 l0 = q[0], h0 = q[1], l1 = q[2], h1 = q[3];
    Box u, r;
    u.lo[0] = l0.x; u.lo[1] = l0.y; u.lo[2] = l0.z;
    u.hi[0] = h0.x; u.hi[1] = h0.y; u.hi[2] = h0.z;
    r.lo[0] = l1.x; r.lo[1] = l1.y; r.lo[2] = l1.z;
    r.hi[0] = h1.x; r.hi[1] = h1.y; r.hi[2] = h1.z;
    u.grow(r);
    store_child(d.nodes, rc.y, u);
}

// RRTE_DEBUG bit 2: every index leaf i's thread is about to use, into the check word.
__device__ bool leaf_indices_ok(const RefitDevice& d, uint32_t i) {
    const uint2 lf = d.leaves[i];
    const uint32_t a = leaf_first(lf.x), n = leaf_count(lf.x);
    uint32_t bad = 0u;
    if (!(lf.x & kLeafBit) || (uint64_t)a + n > d.n_slots) {
        bad |= 128u;
    } else {
        for (uint32_t k = 3u * a; k < 3u * (a + n); ++k)
            if (d.slot_vtx[k] >= d.n_verts) bad |= 128u;
    }
    if (lf.y != kRefitRoot && (lf.y >> 1) >= d.n_recs) bad |= 256u;
    if (bad) atomicOr(d.check, (unsigned long long)bad);
    return !bad;
}

__global__ __launch_bounds__(kRefitBlock) void refit_leaves(RefitDevice d, uint32_t n_leaves) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= n_leaves) return;
    if (d.check && !leaf_indices_ok(d, i)) return;
    refit_leaf(d, i);
}

__global__ __launch_bounds__(kRefitBlock) void refit_level(RefitDevice d, uint32_t begin, uint32_t count) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= count) return;
    const uint2 rc = d.order[begin + i];  // {record, parent code}
    if (d.check && (rc.x >= d.n_recs || (rc.y >> 1) >= d.n_recs)) {
        atomicOr(d.check, 256ull);
        return;
    }
    refit_record(d, rc);
}

inline uint32_t f_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

}  // namespace

bool build_refit_static(const MeshData& md, const uint32_t* indices, uint32_t num_indices, RefitStatic& out) {
    out = RefitStatic{};
    const uint32_t n_slots = (uint32_t)(md.tris.size() / 3), n_recs = (uint32_t)(md.nodes.size() / 4);
    out.slot_vtx.resize((size_t)n_slots * 3);
    out.parent.assign(n_recs, kRefitRoot);
    std::vector<uint32_t> depth(n_recs, 0u);
    std::vector<uint32_t> stack;
    uint32_t max_depth = 0;
    for (const MeshRange& mr : md.ranges) {
        if ((uint64_t)mr.slot_base + mr.count > n_slots || ((uint64_t)mr.first + mr.count) * 3 > num_indices) return false;
        for (uint32_t k = 0; k < mr.count; ++k) {
            const uint32_t o = f_bits(md.tris[3 * (size_t)(mr.slot_base + k)].w);
            if (o >= mr.count) return false;
            for (int j = 0; j < 3; ++j)
                out.slot_vtx[3 * (size_t)(mr.slot_base + k) + j] = indices[((size_t)mr.first + o) * 3 + j];
        }
        if (!mr.count) continue;  // an empty range: nothing to refit
        auto leaf = [&](uint32_t link, uint32_t code) {
            const uint32_t a = link & 0xFFFFFFu, n = ((link >> 24) & 0x7Fu) + 1u;
            if (a < mr.slot_base || (uint64_t)a + n > (uint64_t)mr.slot_base + mr.count) return false;
            out.leaves.push_back(make_uint2(link, code));
            return true;
        };
        if (mr.root & kLeafBit) {
            if (!leaf(mr.root, kRefitRoot)) return false;
            continue;
        }
        if (mr.root >= n_recs) return false;
        stack.assign(1, mr.root);
        size_t visited = 0;
        while (!stack.empty()) {
            const uint32_t rec = stack.back();
            stack.pop_back();
            if (++visited > n_recs) return false;  // (a cycle)
            for (uint32_t side = 0; side < 2; ++side) {
                const uint32_t link = f_bits(md.nodes[(size_t)rec * 4 + side * 2].w), code = rec * 2 + side;
                if (link & kLeafBit) {
                    if (!leaf(link, code)) return false;
                } else {
                    if (link >= n_recs || link == mr.root || out.parent[link] != kRefitRoot) return false;
                    out.parent[link] = code;
                    depth[link] = depth[rec] + 1;
                    max_depth = std::max(max_depth, depth[link]);
                    stack.push_back(link);
                }
            }
        }
    }
    // counting sort by depth, deepest first; depth 0 (the roots) has no parent slot to write
    out.level_off.assign((size_t)max_depth + 1, 0u);
    for (uint32_t r = 0; r < n_recs; ++r)
        if (depth[r]) ++out.level_off[max_depth - depth[r] + 1];
    for (uint32_t l = 0; l < max_depth; ++l) out.level_off[l + 1] += out.level_off[l];
    out.order.resize(out.level_off[max_depth]);
    std::vector<uint32_t> at(out.level_off.begin(), out.level_off.end() - 1);
    for (uint32_t r = 0; r < n_recs; ++r)
        if (depth[r]) out.order[at[max_depth - depth[r]]++] = make_uint2(r, out.parent[r]);
    return true;
}

void refit_range_bounds(const rrte_scene_ir* s, MeshData& md) {
    for (MeshRange& mr : md.ranges) {
        if (!mr.count) continue;
        const uint32_t* ix = s->mesh_indices + (size_t)mr.first * 3;
        Box b;
        for (size_t k = 0; k < (size_t)mr.count * 3; ++k) b.grow(s->mesh_vertices[ix[k]].position);
        b = inflate(b);
        for (int a = 0; a < 3; ++a) {
            mr.lo[a] = b.lo[a];
            mr.hi[a] = b.hi[a];
        }
    }
}

hipError_t launch_refit_levels(uint32_t n_leaves, const uint32_t* level_off, uint32_t levels, const RefitDevice& d,
                               hipStream_t st) {
    if (n_leaves) {
        hipLaunchKernelGGL(refit_leaves, dim3((n_leaves + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, d,
                           n_leaves);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    for (uint32_t l = 0; l < levels; ++l) {
        const uint32_t begin = level_off[l], count = level_off[l + 1] - begin;
        hipLaunchKernelGGL(refit_level, dim3((count + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, d, begin,
                           count);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_refit(const RefitStatic& rs, const RefitDevice& d, hipStream_t st) {
    return launch_refit_levels((uint32_t)rs.leaves.size(), rs.level_off.data(), rs.levels(), d, st);
}

}  // namespace rrte
