// aov.hip — frame AOVs (include/rrte_hip_aov.h): rrte_hip_render_aov / rrte_hip_render_aov_async,
// and the only unit that instantiates the view kernels (aov_kernels.hpp).
//
// Local calls, like the ray queries of rrte_hip.hip: the scene goes through query_scene (the scene
// cache; not a render for JIT AUTO), no collective is issued, no gather batch is closed and rrte_stats
// is untouched.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "context.hpp"
#include "aov_kernels.hpp"

using namespace rrte;

namespace {

constexpr uint32_t kAovPlanes = 7u;
constexpr uint32_t kAovFloat4 = RRTE_AOV_NORMAL | RRTE_AOV_POSITION | RRTE_AOV_ALBEDO;
static_assert(RRTE_AOV_ALL == (1u << kAovPlanes) - 1u, "one bit per plane, in rrte_aov_buffers' order");
static_assert(sizeof(rrte_aov_desc) == 32 && sizeof(rrte_aov_buffers) == 64, "AOV record layout");

constexpr size_t plane_bytes(uint32_t k) { return ((1u << k) & kAovFloat4) ? 16u : 4u; }

// Plane k's pointer of a rrte_aov_buffers (its members in bit order).
void* plane_ptr(const rrte_aov_buffers* b, uint32_t k) {
    void* const p[kAovPlanes] = {b->depth, b->prim, b->material, b->tri, b->normal, b->position, b->albedo};
    return p[k];
}

void set_planes(AovArgs& a, void* const p[kAovPlanes]) {
    a.depth = static_cast<float*>(p[0]);
    a.prim = static_cast<int32_t*>(p[1]);
    a.material = static_cast<int32_t*>(p[2]);
    a.tri = static_cast<uint32_t*>(p[3]);
    a.normal = static_cast<float4*>(p[4]);
    a.position = static_cast<float4*>(p[5]);
    a.albedo = static_cast<float4*>(p[6]);
}

// The argument checks of both forms; on success `a` holds the frame's camera, the rectangle, the plane
// mask and the background (the plane pointers are the caller's to set).
rrte_status aov_args(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, const rrte_aov_desc* d,
                     const rrte_aov_buffers* b, bool device, AovArgs& a) {
    if (!s || !p || !d || !b) return fail(c, RRTE_INVALID_ARG, "null scene, params, AOV description or buffers");
    if (d->planes == 0 || (d->planes & ~RRTE_AOV_ALL))
        return fail(c, RRTE_INVALID_ARG, "AOV planes 0x%x: none, or unknown bits", d->planes);
    if (d->_pad[0] | d->_pad[1] | d->_pad[2] || b->_reserved)
        return fail(c, RRTE_INVALID_ARG, "rrte_aov_desc::_pad / rrte_aov_buffers::_reserved must be zero");
    for (uint32_t k = 0; k < kAovPlanes; ++k) {
        if (!(d->planes & (1u << k))) continue;
        const uintptr_t q = (uintptr_t)plane_ptr(b, k);
        if (!q) return fail(c, RRTE_INVALID_ARG, "AOV plane 0x%x requested with a null buffer", 1u << k);
        if (device && (q & (plane_bytes(k) - 1u)))
            return fail(c, RRTE_INVALID_ARG, "device buffer of AOV plane 0x%x must be %zu-byte aligned", 1u << k,
                        plane_bytes(k));
    }
    if (p->width == 0 || p->height == 0) return fail(c, RRTE_INVALID_ARG, "zero-sized frame %ux%u", p->width, p->height);
    if ((uint64_t)p->width * p->height > (1ull << 30)) return fail(c, RRTE_INVALID_ARG, "frame too large");
    uint32_t x0 = d->x0, y0 = d->y0, w = d->width, h = d->height;
    if (!(x0 | y0 | w | h)) {  // the whole frame
        w = p->width;
        h = p->height;
    }
    // (no sum that could wrap: x0 + w <= width as w <= width - x0)
    if (w == 0 || h == 0 || x0 >= p->width || y0 >= p->height || w > p->width - x0 || h > p->height - y0)
        return fail(c, RRTE_INVALID_ARG, "AOV rectangle %ux%u at (%u, %u) is empty or leaves the %ux%u frame", d->width,
                    d->height, d->x0, d->y0, p->width, p->height);
    // the frame's camera record (make_params), for a frame of this size: rrte_hip_pick's
    rrte_render_params pf{};
    pf.width = p->width;
    pf.height = p->height;
    pf.samples_per_pixel = 1;
    pf.gamma = 2.2f;
    pf.t_min = p->t_min;
    const KParams k = make_params(c, s, &pf, p->height);
    a = AovArgs{};
    a.qc.cam = k.cam[0];
    a.qc.width = p->width;
    a.qc.height = p->height;
    a.qc.t_min = p->t_min;
    a.x0 = x0;
    a.y0 = y0;
    a.w = w;
    a.h = h;
    a.planes = d->planes;
    memcpy(a.bg, p->background, sizeof a.bg);
    return RRTE_OK;
}

// Enqueue one launch of `a` on `st`; the cached scene is `s` (query_scene).
rrte_status aov_launch(rrte_ctx* c, const rrte_scene_ir* s, const AovArgs& a, hipStream_t st, bool fresh_count) {
    const SceneView sv{c->d_prims, c->d_mats, c->d_lights, c->d_nodes, s->num_prims, s->num_lights, s->num_materials,
                       c->mesh_view};
    trace_rec(c, "launch aov", st, nullptr, a.w, a.h);
    if (c->accel_on) {
        AccelView av;
        rrte_status ar = accel_launch_view(c, st, av, fresh_count);
        if (ar != RRTE_OK) return ar;
        launch_aov_accel(st, sv, av, a);
        HIPCHK(c, hipGetLastError());
        return accel_launch_done(c, st);
    }
    const uint32_t need = c->env.generic_all ? (kFeatAll | (c->scene_feat & kFeatInstance)) : c->scene_feat;
    launch_aov(need, st, sv, a);
    HIPCHK(c, hipGetLastError());
    return RRTE_OK;
}

// The blocking form: the rectangle in chunks of whole tile rows (of at most about kQueryChunk pixels:
// a rectangle wider than kQueryChunk / 8 is cut into column blocks of whole tiles as well) staged
// through the context's buffer on the context's stream; each requested plane's block copied back to
// its place in the caller's array; returns after the planes are on the host.
rrte_status aov_blocking(rrte_ctx* c, const rrte_scene_ir* s, const AovArgs& full, const rrte_aov_buffers* out) {
    rrte_status r = query_scene(c, s, c->stream);
    if (r != RRTE_OK) return r;
    const uint32_t cw = std::min(full.w, kQueryChunk / kAovTile);  // (kQueryChunk / 8: a multiple of the tile)
    const uint32_t tile_rows = std::max(1u, kQueryChunk / (cw * kAovTile));
    const uint32_t ch = (uint32_t)std::min<uint64_t>(full.h, (uint64_t)tile_rows * kAovTile);
    // the chunk's planes at 256-B aligned offsets of one allocation
    size_t off[kAovPlanes] = {}, total = 0;
    for (uint32_t k = 0; k < kAovPlanes; ++k) {
        if (!(full.planes & (1u << k))) continue;
        off[k] = total;
        total += ((size_t)cw * ch * plane_bytes(k) + 255u) & ~(size_t)255u;
    }
    if ((r = ensure(c, c->d_aov, total)) != RRTE_OK) return r;
    void* d_plane[kAovPlanes] = {};
    for (uint32_t k = 0; k < kAovPlanes; ++k)
        if (full.planes & (1u << k)) d_plane[k] = c->d_aov.get() + off[k];
    bool first = true;
    for (uint32_t cy = 0; cy < full.h; cy += ch) {
        for (uint32_t cx = 0; cx < full.w; cx += cw) {
            AovArgs a = full;
            a.x0 = full.x0 + cx;
            a.y0 = full.y0 + cy;
            a.w = std::min(cw, full.w - cx);
            a.h = std::min(ch, full.h - cy);
            set_planes(a, d_plane);
            if ((r = aov_launch(c, s, a, c->stream, first)) != RRTE_OK) return r;
            first = false;
            for (uint32_t k = 0; k < kAovPlanes; ++k) {
                if (!(full.planes & (1u << k))) continue;
                const size_t es = plane_bytes(k);
                uint8_t* dst = static_cast<uint8_t*>(plane_ptr(out, k)) + ((size_t)cy * full.w + cx) * es;
                if (a.w == full.w)  // whole rows: one contiguous block
                    HIPCHK(c, hipMemcpyAsync(dst, d_plane[k], (size_t)a.w * a.h * es, hipMemcpyDeviceToHost, c->stream));
                else
                    HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)full.w * es, d_plane[k], (size_t)a.w * es, (size_t)a.w * es,
                                               a.h, hipMemcpyDeviceToHost, c->stream));
            }
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRTE_OK;
}

}  // namespace

extern "C" {

rrte_status rrte_hip_render_aov(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p,
                                const rrte_aov_desc* d, const rrte_aov_buffers* out) {
    if (!c) return RRTE_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    AovArgs a;
    rrte_status r = aov_args(c, s, p, d, out, false, a);
    if (r != RRTE_OK) return r;
    return aov_blocking(c, s, a, out);
}

rrte_status rrte_hip_render_aov_async(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p,
                                      const rrte_aov_desc* d, const rrte_aov_buffers* d_out, void* stream) {
    if (!c) return RRTE_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    AovArgs a;
    rrte_status r = aov_args(c, s, p, d, d_out, true, a);
    if (r != RRTE_OK) return r;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
    if ((r = query_scene(c, s, st)) != RRTE_OK) return r;
    void* planes[kAovPlanes];
    for (uint32_t k = 0; k < kAovPlanes; ++k) planes[k] = (a.planes & (1u << k)) ? plane_ptr(d_out, k) : nullptr;
    set_planes(a, planes);
    return aov_launch(c, s, a, st, true);
}

}  // extern "C"
