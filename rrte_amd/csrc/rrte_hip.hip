// rrte_hip.hip — C-ABI implementation (include/rrte_hip.h) of the MI355X-native
// replacement for rrte-renderer's Raytracer::render
// (Melthizar/RRTE crates/rrte-renderer/src/raytracer.rs:45-148).
//
// This file is the launch itself and the only one that instantiates the ray and query kernels
// (ray_kernel, ray_kernel_accel, ray_query_kernel, ray_query_accel_kernel): the
// launch, the counters, the blocking frame paths, the render entry points and the ray queries.
// The rest of the host side lives beside it, around one private header (context.hpp: rrte_ctx and
// what the units share).  No exception crosses the ABI.
//
// Where a function lives (headers and documents that say "rrte_hip.hip X" mean the unit below):
//   context.hip       rrte_hip_create / destroy / synchronize / stats / check_word, the environment
//                     switches (read_env), the setters and info getters, host_register / unregister,
//                     retire / retired_done / wait_retired (context.hpp: struct Version over them;
//                     resources.hpp: the owning buffer, event and stream types)
//   scene_upload.hip  validate, validate_scene, lower_scene, prim_bound, the mat4 restatement,
//                     scene_key_parts, the mesh cache, topology_of, scene_features,
//                     scene_records_check, upload_scene, rrte_hip_mesh_refit / mesh_nodes / mesh_slots,
//                     rrte_hip_sdf_guards
//   launch_plan.hip   make_params, tile_rects / fill_tile_rects, rows_for_rank, sky_band_count,
//                     band_layout, cull_policy, plan_launch, frame_band_map and their context-free exports
//   jit_select.hip    jit_kernel_for / jit_lookup (jit_pending), jit_wants_topology, jit_key,
//                     jit_uniform_guards, rrte_hip_jit_check / build_id / jit_cache_key
//   tile_order.hip    the tile order of a launch (TileProfile: lpt_slots, fixed_slots, reserve_hot_lists,
//                     upload_hot_list, plan_tile_order, finish_tile_order: issue_launch is their only
//                     caller), rrte_hip_tile_order_plan
//   aov.hip           rrte_hip_render_aov / render_aov_async (include/rrte_hip_aov.h; kernels: aov_kernels.hpp)
//   rrte_hip.hip      launch_generic (the generic kernel variant), plain_launch, issue_launch, launch,
//                     resolve_counters, finish_frame,
//                     render_chunked, render_common, dump_if_asked, rrte_hip_render*, the ray queries
//   gather.hip        rrte_hip_comm_*, slab_rgb24, deinterleave, render_peers, render_batch,
//                     flush_batch, gather_frame, nccl_settle, comm_abort, poll_events, wait_bounded,
//                     rrte_hip_render_gather* / flush / set_gather_batch / gather_info
//   fpcheck.hip       rrte_hip_fpcheck
//   march_clip.hip    rrte_hip_march_clip (the constants of march_clip.hpp, which jit.hip pastes into
//                     every generated source)
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstddef>
#include <cstring>

#include "context.hpp"
#include "ray_query.hpp"

using namespace rrte;

namespace rrte {

// The generic kernel variant for a scene with features `need` (kFeat*): the first of the
// precompiled feature sets F0, F1, F2 that covers it, else every feature (scene_view.hpp SceneView).
template <int MODE, bool CULL, uint32_t F0, uint32_t F1, uint32_t F2>
static void launch_generic(uint32_t need, dim3 grid, dim3 block, hipStream_t st, const KParams& k, const SceneView& sv,
                           const Cull& cl, uint32_t* d_rgba, float4* d_f32, unsigned long long* ctr) {
    // (kFeatInstance is in none of F0..F2: an instance scene takes the last branch)
    if ((need & ~F0) == 0u)
        hipLaunchKernelGGL((ray_kernel<MODE, CULL, F0>), grid, block, 0, st, k, sv, cl, d_rgba, d_f32, ctr);
    else if ((need & ~F1) == 0u)
        hipLaunchKernelGGL((ray_kernel<MODE, CULL, F1>), grid, block, 0, st, k, sv, cl, d_rgba, d_f32, ctr);
    else if ((need & ~F2) == 0u)
        hipLaunchKernelGGL((ray_kernel<MODE, CULL, F2>), grid, block, 0, st, k, sv, cl, d_rgba, d_f32, ctr);
    else if ((need & kFeatInstance) == 0u)
        hipLaunchKernelGGL((ray_kernel<MODE, CULL, kFeatAll>), grid, block, 0, st, k, sv, cl, d_rgba, d_f32, ctr);
    else  // a scene with mesh instances: every feature plus the instance path
        hipLaunchKernelGGL((ray_kernel<MODE, CULL, kFeatEvery>), grid, block, 0, st, k, sv, cl, d_rgba, d_f32, ctr);
}

// Whether a launch of the specialised kernel `jk` meets every assumption of its plain entry
// (shade.hpp LaunchPlain): one frame into the RGBA8 device buffer `d_rgba` alone, rows packed from
// image row 0 with no band map, no debug bit, gamma 2.2 and one sample per pixel (SINGLE kernels only
// have the entry).  Gather slabs, rank shares, multi-frame batches, f32
// frames, zero-copy frames (rrte_ctx::host_out), RRTE_DEBUG and other gammas
// fail one of the tests and take the general entry; RRTE_JIT_PLAIN=0 sends everything there.
static bool plain_launch(const rrte_ctx* c, const JitKernel* jk, const LaunchPlan& L, const uint32_t* d_rgba,
                         const float4* d_f32) {
    const KParams& k = L.k;
    return c->env.jit_plain && jk->fn_plain && L.single && d_rgba && !d_f32 && !c->host_out &&
           k.nframes == 1 && k.band_rows == 0 && k.row0 == 0 && k.out_image_rows == 0 && k.debug == 0 &&
           !(k.flags & (kFlagSlabRgb24 | kFlagHostStore)) && k.inv_gamma == kInvGamma22 && k.inv_spp == 1.0f;
}

// The accelerator's launch argument for a frame or query on `st`.  Under RRTE_ACCEL_COUNT the launch
// counts into two spare words of counter shard 0 (words 2 and 3 of its 128-B line: word 0 is the
// shadow-ray count, word 1 the check word), cleared on `st` ahead of it; `fresh` false continues the
// counts of the launch before (the later chunks of one blocking query).
rrte_status accel_launch_view(rrte_ctx* c, hipStream_t st, AccelView& av, bool fresh) {
    av = c->accel;
    if (!(c->accel_flags & RRTE_ACCEL_COUNT)) return RRTE_OK;
    av.count = c->d_counters + 2;
    HIPCHK(c, c->ev_accel.create());
    if (fresh) HIPCHK(c, hipMemsetAsync(c->d_counters + 2, 0, 2 * sizeof(unsigned long long), st));
    return RRTE_OK;
}

// Behind an accelerated launch on `st`: under RRTE_ACCEL_COUNT the event rrte_hip_accel_info waits for
// (an event, not the stream: the caller may destroy its stream once its work is done).
rrte_status accel_launch_done(rrte_ctx* c, hipStream_t st) {
    if (!(c->accel_flags & RRTE_ACCEL_COUNT)) return RRTE_OK;
    HIPCHK(c, hipEventRecord(c->ev_accel, st));
    c->accel_counted = true;
    return RRTE_OK;
}

// Launch plan `L` (L.k.nframes frames) on `st`; the cached scene is the plan's.
rrte_status issue_launch(rrte_ctx* c, LaunchPlan& L, uint32_t* d_rgba, float4* d_f32, hipStream_t st) {
    if (L.gy == 0) return RRTE_OK;
    HostSection hsa(c);
    Cull cl{L.cull ? c->d_bounds : nullptr, L.num_prims};
    // an accelerated scene runs the accelerated generic kernel, whatever the JIT policy says
    JitKernel* jk = c->accel_on ? nullptr : jit_kernel_for(c, L.mode, L.cull, L.single);
    c->stats.jit_active = jk ? (jk->topology ? 2u : 1u) : 0u;
    // 64-thread workgroups: (tile column, frame, tile row or slot row), KParams::hot
    const bool profile = plan_tile_order(c, L, jk ? (const void*)jk->fn : nullptr, st);
    c->stats.hot_tiles = L.k.hot_n;
    // the launch reads the current scene version: after its upload, tracked until retired
    if (c->sb_cur >= 0) HIPCHK(c, c->sb[c->sb_cur].ver.begin_read(c, st, "wait scene upload"));
    c->launched.use(st);
    if (c->ctr_pending && st != c->stream) HIPCHK(c, c->ctr[c->ctr_slot].wait_upload(c, st, "wait counter snapshot"));
    const dim3 grid(L.gx, L.k.nframes, L.gy), block(kBlockThreads);
    trace_rec(c, profile ? "launch ray (profiled)" : "launch ray", st, nullptr, L.k.nframes, L.k.rows);
    if (jk) {
        unsigned long long* ctr = c->d_counters;
        MeshView mv = c->mesh_view;
        SceneValues vals{c->d_prims, c->d_mats, c->d_lights, c->d_nodes};  // read by topology kernels
        void* args[] = {&L.k, &cl, &mv, &d_rgba, &d_f32, &ctr, &vals};
        if (c->hpa_cur) hsa.lap(13);
        HostSection hs(c);
        const bool plain = plain_launch(c, jk, L, d_rgba, d_f32);
        c->last_entry = plain ? RRTE_ENTRY_PLAIN : RRTE_ENTRY_GENERAL;
        if (plain)
            HIPCHK(c, hipModuleLaunchKernel(jk->fn_plain, grid.x, grid.y, grid.z, kBlockThreads, 1, 1, 0, st, args, nullptr));
        else
            HIPCHK(c, hipModuleLaunchKernel(jk->fn, grid.x, grid.y, grid.z, kBlockThreads, 1, 1, 0, st, args, nullptr));
        hs.lap(c->hpa_cur ? 14 : 8);
        return finish_tile_order(c, L, profile, st);
    }
    c->last_entry = RRTE_ENTRY_GENERIC;
    SceneView sv{c->d_prims, c->d_mats, c->d_lights, c->d_nodes, L.num_prims, L.num_lights, L.num_materials,
                 c->mesh_view};
    const KParams& k = L.k;
    if (c->accel_on) {
        AccelView av;
        rrte_status ar = accel_launch_view(c, st, av);
        if (ar != RRTE_OK) return ar;
        if (L.mode == RRTE_MODE_REFCOMPAT)
            hipLaunchKernelGGL((ray_kernel_accel<RRTE_MODE_REFCOMPAT>), grid, block, 0, st, k, sv, av, d_rgba, d_f32,
                               c->d_counters);
        else
            hipLaunchKernelGGL((ray_kernel_accel<RRTE_MODE_LAMBERT_SHADOW>), grid, block, 0, st, k, sv, av, d_rgba, d_f32,
                               c->d_counters);
        HIPCHK(c, hipGetLastError());
        if ((ar = accel_launch_done(c, st)) != RRTE_OK) return ar;
        return finish_tile_order(c, L, profile, st);
    }
    const uint32_t need = c->env.generic_all ? (kFeatAll | (c->scene_feat & kFeatInstance)) : c->scene_feat;
    if (L.mode == RRTE_MODE_REFCOMPAT)
        launch_generic<RRTE_MODE_REFCOMPAT, false, 0u, kFeatAnalytic, kFeatSdf>(need, grid, block, st, k, sv, cl, d_rgba,
                                                                             d_f32, c->d_counters);
    else if (L.cull)
        launch_generic<RRTE_MODE_LAMBERT_SHADOW, true, kFeatSdf, kFeatSdf | kFeatDeform, kFeatSdf | kFeatAnalytic>(
            need, grid, block, st, k, sv, cl, d_rgba, d_f32, c->d_counters);
    else
        launch_generic<RRTE_MODE_LAMBERT_SHADOW, false, 0u, kFeatAnalytic, kFeatSdf>(need, grid, block, st, k, sv, cl,
                                                                                    d_rgba, d_f32, c->d_counters);
    HIPCHK(c, hipGetLastError());
    return finish_tile_order(c, L, profile, st);
}

rrte_status launch(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, uint32_t rows,
                   uint32_t* d_rgba, float4* d_f32, hipStream_t st, uint32_t internal_flags, uint32_t row0, int prof,
                   const BandMap* bm) {
    if (rows == 0) return RRTE_OK;
    HostSection hs(c);
    LaunchPlan L = plan_launch(c, s, p, rows, internal_flags, row0, bm);
    if (c->hpa_cur) hs.lap(12);
    L.prof = prof;
    return issue_launch(c, L, d_rgba, d_f32, st);
}

// The code object of this file (every generic kernel), loaded at rrte_hip_create and not inside the
// first frame.
hipError_t load_ray_kernels() {
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&ray_kernel_accel<RRTE_MODE_REFCOMPAT>));
}

static unsigned long long* ctr_host(rrte_ctx* c, int slot) { return slot ? c->h_counters2 : c->h_counters; }
static unsigned long long ctr_total(rrte_ctx* c, int slot) {
    const unsigned long long* h = ctr_host(c, slot);
    unsigned long long total = 0;
    for (uint32_t i = 0; i < kCounterShards; ++i) total += h[i * kCounterStride];
    return total;
}

// The last blocking frame's shadow-ray count into rrte_stats (waits for its counter copy).
rrte_status resolve_counters(rrte_ctx* c) {
    if (!c->ctr_pending) return RRTE_OK;
    HIPCHK(c, hipEventSynchronize(c->ctr[c->ctr_slot].ev_up));
    const unsigned long long total = ctr_total(c, c->ctr_slot);
    c->stats.shadow_rays = total - c->shadow_base;
    c->shadow_base = total;
    c->ctr_pending = false;
    return RRTE_OK;
}

// Wait for `ev` by polling (a blocking wait wakes the host several us after the device signals):
// at most ~2 ms of polling, then a blocking wait.
static rrte_status spin_wait(rrte_ctx* c, hipEvent_t ev) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0;; ++spin) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return RRTE_OK;
        if (e != hipErrorNotReady) HIPCHK(c, e);
        if ((spin & 63u) == 63u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
            HIPCHK(c, hipEventSynchronize(ev));
            return RRTE_OK;
        }
    }
}

// Read back the device counters and close the frame's statistics.  `deferred` (the blocking
// single-context frame): return once the frame's work on the context's stream is complete; the
// counter copy queued behind it is folded in by resolve_counters when the statistics are read.
rrte_status finish_frame(rrte_ctx* c, bool deferred) {
    // the slot the pending copy does not use (that copy precedes this one on the stream)
    const int slot = c->ctr_pending ? 1 - c->ctr_slot : 0;
    if (deferred) HIPCHK(c, hipEventRecord(c->ev_done, c->stream));
    HIPCHK(c, hipMemcpyAsync(ctr_host(c, slot), c->d_counters, kCounterBytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, c->ctr[slot].published(c->stream));  // (no stream has waited for this snapshot yet)
    rrte_status r = deferred ? spin_wait(c, c->ev_done) : RRTE_OK;
    if (r != RRTE_OK) return r;
    trace_rec(c, "frame complete (host)", c->stream, nullptr);
    if (!deferred) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->ctr_pending) {
        // (complete: it precedes this frame on the stream) the previous frame's counts, never read,
        // become the base of this one's
        c->shadow_base = ctr_total(c, c->ctr_slot);
        c->ctr_pending = false;
    }
    c->ctr_slot = slot;
    c->ctr_pending = true;
    if (!deferred && (r = resolve_counters(c)) != RRTE_OK) return r;
    if (c->pending_kernel_timing) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) c->stats.kernel_ms = ms;
        c->pending_kernel_timing = false;
    }
    c->stats.primary_rays = c->pending_primary;
    return RRTE_OK;
}

// The blocking drop-in path into a host RGBA8 buffer (Raytracer::render, raytracer.rs:45-89): the
// frame renders as `n` row chunks (multiples of 16 rows, so camera-culling tiles never straddle two
// chunks), each launched on a stream of its own so they run together as one frame would, each in its
// own measured-cost tile order (tile-profile slot 1 + i).  Each chunk's D2H copy starts on the copy
// stream as soon as that chunk's kernel has completed -- the kernel boundary orders its stores, no
// fences -- so the 8.3 MB PCIe copy (~150 us at ~55 GB/s) overlaps the rest of the render instead of
// following all of it.  Copies run top to bottom.
static rrte_status render_chunked(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, uint8_t* out8,
                                  uint32_t n) {
    const uint32_t W = p->width, H = p->height;
    const uint32_t rows = (((H + n - 1) / n) + 15u) & ~15u;
    n = (H + rows - 1) / rows;
    for (uint32_t i = 0; i < n; ++i) {
        HIPCHK(c, c->bnd_stream[i].create());
        HIPCHK(c, c->ev_bchunk[i].create());
    }
    HIPCHK(c, c->bnd_copy.create());
    HIPCHK(c, c->ev_bcopy.create());
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));  // after the work already queued on the context's stream
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t r0 = i * rows, nr = std::min(rows, H - r0);
        HIPCHK(c, hipStreamWaitEvent(c->bnd_stream[i], c->ev0, 0));
        rrte_status r = launch(c, s, p, nr, c->d_rgba + (size_t)r0 * W, nullptr, c->bnd_stream[i], 0u, r0, 1 + (int)i);
        if (r != RRTE_OK) return r;
        HIPCHK(c, hipEventRecord(c->ev_bchunk[i], c->bnd_stream[i]));
    }
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t r0 = i * rows, nr = std::min(rows, H - r0);
        HIPCHK(c, hipStreamWaitEvent(c->bnd_copy, c->ev_bchunk[i], 0));
        HIPCHK(c, hipMemcpyAsync(out8 + (size_t)r0 * W * 4, c->d_rgba + (size_t)r0 * W, (size_t)nr * W * 4,
                                 hipMemcpyDeviceToHost, c->bnd_copy));
    }
    HIPCHK(c, hipEventRecord(c->ev_bcopy, c->bnd_copy));
    // the context's stream: every chunk (ev1: the render's end, rrte_stats.kernel_ms), then the copies
    for (uint32_t i = 0; i < n; ++i) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_bchunk[i], 0));
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_bcopy, 0));
    return RRTE_OK;
}

// The device address of pinned host memory [host, host + bytes) -- hipHostMalloc'd, or registered
// (rrte_hip_host_register, hipHostRegister) -- or nullptr for pageable memory.  The whole range must
// lie in one pinned allocation.
static uint32_t* pinned_device_ptr(void* host, size_t bytes) {
    hipPointerAttribute_t a{}, b{};
    if (hipPointerGetAttributes(&a, host) != hipSuccess) {
        (void)hipGetLastError();  // (pageable memory: not an error of this call)
        return nullptr;
    }
    if (a.type != hipMemoryTypeHost || !a.devicePointer) return nullptr;
    uint8_t* last = static_cast<uint8_t*>(host) + bytes - 1;
    if (hipPointerGetAttributes(&b, last) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (b.type != hipMemoryTypeHost || static_cast<uint8_t*>(b.devicePointer) != static_cast<uint8_t*>(a.devicePointer) + bytes - 1)
        return nullptr;
    return static_cast<uint32_t*>(a.devicePointer);
}

// RRTE_DUMP_SCENE (diagnostics): the frame's scene and parameters, as given, into the dump file
// before anything else happens to them (rrte_hip_scene_dump; replayable on the oracle or the device).
void dump_if_asked(const rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p) {
    if (!c->env.dump_path.empty() && s && p) (void)rrte_hip_scene_dump(s, p, c->env.dump_path.c_str());
}

static rrte_status render_common(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, uint8_t* out8,
                                 float* outf) {
    dump_if_asked(c, s, p);
    rrte_status r = validate(c, s, p);
    if (r != RRTE_OK) return r;
    HIPCHK(c, hipSetDevice(c->device));
    double up = 0.0;
    if ((r = upload_scene(c, s, c->stream, &up)) != RRTE_OK) return r;
    const size_t npix = (size_t)p->width * p->height;
    if ((r = ensure(c, c->d_rgba, npix)) != RRTE_OK) return r;
    if (outf && (r = ensure(c, c->d_f32, npix)) != RRTE_OK) return r;
    // single-context render: all rows, no band mapping
    const int nr = c->nranks, rk = c->rank;
    c->nranks = 1;
    c->rank = 0;
    c->jit_stream = false;  // (one blocking frame: the latency flavour of the specialised kernel)
    // pinned caller buffer: the kernel writes the frame into it directly (no D2H copy afterwards)
    uint32_t* zc = out8 && !outf && c->env.bnd_zerocopy ? pinned_device_ptr(out8, npix * 4) : nullptr;
    const bool chunked = !zc && out8 && !outf && c->env.bnd_chunks > 1 && p->height >= 32u && !(c->env.debug & ~4u);  // (bit 2, the index check, keeps every path)
    if (chunked) {
        r = render_chunked(c, s, p, out8, (uint32_t)c->env.bnd_chunks);
    } else {
        HIPCHK(c, hipEventRecord(c->ev0, c->stream));
        if (zc) c->tile_shift = c->env.zc_tile_shift;  // whole 128-B lines per wave across PCIe
        c->host_out = zc != nullptr;
        r = launch(c, s, p, p->height, zc ? zc : c->d_rgba, outf ? c->d_f32 : nullptr, c->stream,
                   zc && c->env.zc_system_store ? kFlagHostStore : 0u, 0u, zc ? rrte_ctx::kZcProf : 0);
        c->tile_shift = 3;
        c->host_out = false;
        if (r == RRTE_OK) r = hipEventRecord(c->ev1, c->stream) == hipSuccess ? RRTE_OK : RRTE_HIP_ERROR;
    }
    c->nranks = nr;
    c->rank = rk;
    c->jit_stream = true;
    if (r != RRTE_OK) return r;
    c->pending_kernel_timing = true;
    c->pending_primary = (uint64_t)npix * p->samples_per_pixel;
    c->stats.upload_ms = up;
    c->stats.gather_ms = 0.0;
    if (out8 && !chunked && !zc) HIPCHK(c, hipMemcpyAsync(out8, c->d_rgba, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (outf) HIPCHK(c, hipMemcpyAsync(outf, c->d_f32, npix * 16, hipMemcpyDeviceToHost, c->stream));
    if ((r = finish_frame(c, true)) != RRTE_OK) return r;
    c->stats.frames++;
    return RRTE_OK;
}

}  // namespace rrte

extern "C" {

rrte_status rrte_hip_render(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, uint8_t* out) {
    if (!c) return RRTE_INVALID_ARG;
    if (!out) return fail(c, RRTE_INVALID_ARG, "null output buffer");
    trace_rec(c, "render: enter", nullptr, nullptr);
    return render_common(c, s, p, out, nullptr);
}

rrte_status rrte_hip_render_f32(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, uint8_t* out8,
                                float* outf) {
    if (!c) return RRTE_INVALID_ARG;
    return render_common(c, s, p, out8, outf);
}

rrte_status rrte_hip_render_async(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, void* d_rgba,
                                  void* d_f32, void* stream) {
    if (!c) return RRTE_INVALID_ARG;
    dump_if_asked(c, s, p);
    HostSection hs(c);
    rrte_status r = validate(c, s, p);
    if (r != RRTE_OK) return r;
    hs.lap(10);
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
    double up = 0.0;
    if ((r = upload_scene(c, s, st, &up)) != RRTE_OK) return r;
    hs.lap(11);
    c->hpa_cur = true;
    const int nr = c->nranks, rk = c->rank;
    uint32_t rows = p->height;
    rrte_render_params pe = *p;
    BandMap bm{0u, 1u, 0u, 1u, 1u};
    if (c->env.emu_nranks > 1) {  // diagnostic: exactly one rank's share of a multi-GPU frame, packed
        c->nranks = c->env.emu_nranks;
        c->rank = c->env.emu_rank;
        pe.band_rows = p->band_rows ? p->band_rows : 16;
        bm = frame_band_map(c, s, &pe, 0, &rows);
    } else {
        c->nranks = 1;
        c->rank = 0;
    }
    r = launch(c, s, &pe, rows, static_cast<uint32_t*>(d_rgba), static_cast<float4*>(d_f32), st, 0u, 0u, 0, &bm);
    c->hpa_cur = false;
    c->nranks = nr;
    c->rank = rk;
    if (r != RRTE_OK) return r;
    c->hpa_frames += c->env.host_prof;
    c->pending_primary = (uint64_t)p->width * rows * p->samples_per_pixel;
    c->stats.upload_ms = up;
    c->stats.frames++;
    return RRTE_OK;
}

}  // extern "C"

// ------------------------------------------------- ray queries (include/rrte_hip_query.h)
// Closest hit, any hit and pixel picking over the cached scene (kernel: ray_query.hpp).  Local
// calls: no collective, no gather-batch close, rrte_stats untouched.
// (kQueryChunk rays per launch of the blocking forms: 128 MiB of rays, 192 MiB of hits)
namespace rrte {

// The scene of a query, cached and readable on `st`: validated, uploaded through the context's scene
// cache if it differs from the cached one, `st` ordered after the version's upload and registered with
// its retire tracking (as issue_launch does for a frame).
rrte_status query_scene(rrte_ctx* c, const rrte_scene_ir* s, hipStream_t st) {
    rrte_status r = validate_scene(c, s);
    if (r != RRTE_OK) return r;
    const uint64_t renders = c->same_scene_renders;
    double up = 0.0;
    if ((r = upload_scene(c, s, st, &up)) != RRTE_OK) return r;
    // a query of the cached scene is not a render of it (JIT AUTO counts consecutive renders)
    if (c->same_scene_renders == renders + 1) c->same_scene_renders = renders;
    if (c->sb_cur >= 0) HIPCHK(c, c->sb[c->sb_cur].ver.begin_read(c, st, "wait scene upload"));
    c->launched.use(st);
    return RRTE_OK;
}

}  // namespace rrte

namespace {

// Enqueue one query launch of n rays (or n pixel pairs with `qc`) on `st`.
rrte_status query_launch(rrte_ctx* c, const rrte_scene_ir* s, const void* d_in, uint32_t n, uint32_t flags,
                         const QueryCam* qc, void* d_hits, hipStream_t st, bool fresh_count = true) {
    const SceneView sv{c->d_prims, c->d_mats, c->d_lights, c->d_nodes, s->num_prims, s->num_lights, s->num_materials,
                       c->mesh_view};
    const uint32_t need = c->env.generic_all ? (kFeatAll | (c->scene_feat & kFeatInstance)) : c->scene_feat;
    static const QueryCam no_cam{};
    trace_rec(c, "launch query", st, nullptr, n, flags);
    if (c->accel_on) {
        AccelView av;
        rrte_status ar = accel_launch_view(c, st, av, fresh_count);
        if (ar != RRTE_OK) return ar;
        if (qc)
            launch_query_accel<false, true>(n, st, sv, av, d_in, *qc, d_hits);
        else if (flags & RRTE_QUERY_ANY)
            launch_query_accel<true, false>(n, st, sv, av, d_in, no_cam, d_hits);
        else
            launch_query_accel<false, false>(n, st, sv, av, d_in, no_cam, d_hits);
        HIPCHK(c, hipGetLastError());
        return accel_launch_done(c, st);
    }
    if (qc)
        launch_query<false, true>(need, n, st, sv, d_in, *qc, d_hits);
    else if (flags & RRTE_QUERY_ANY)
        launch_query<true, false>(need, n, st, sv, d_in, no_cam, d_hits);
    else
        launch_query<false, false>(need, n, st, sv, d_in, no_cam, d_hits);
    HIPCHK(c, hipGetLastError());
    return RRTE_OK;
}

// The blocking forms: `in_stride` bytes per ray (or pixel pair) staged through the context's buffers
// in chunks on the context's stream; returns after the hits are on the host.
rrte_status query_blocking(rrte_ctx* c, const rrte_scene_ir* s, const void* in, size_t in_stride, uint32_t n,
                           uint32_t flags, const QueryCam* qc, rrte_ray_hit* hits) {
    rrte_status r = query_scene(c, s, c->stream);
    if (r != RRTE_OK) return r;
    const uint32_t chunk = std::min(n, kQueryChunk);
    if ((r = ensure(c, c->d_qin, (size_t)chunk * in_stride)) != RRTE_OK) return r;
    if ((r = ensure(c, c->d_qout, (size_t)chunk * sizeof(rrte_ray_hit))) != RRTE_OK) return r;
    for (uint32_t done = 0; done < n; done += chunk) {
        const uint32_t m = std::min(chunk, n - done);
        HIPCHK(c, hipMemcpyAsync(c->d_qin, static_cast<const uint8_t*>(in) + (size_t)done * in_stride,
                                 (size_t)m * in_stride, hipMemcpyHostToDevice, c->stream));
        if ((r = query_launch(c, s, c->d_qin, m, flags, qc, c->d_qout, c->stream, done == 0)) != RRTE_OK) return r;
        HIPCHK(c, hipMemcpyAsync(hits + done, c->d_qout, (size_t)m * sizeof(rrte_ray_hit), hipMemcpyDeviceToHost,
                                 c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRTE_OK;
}

rrte_status query_args(rrte_ctx* c, const rrte_scene_ir* s, const void* in, uint32_t n, uint32_t flags,
                       const void* out) {
    if (!s || !in || !out) return fail(c, RRTE_INVALID_ARG, "null scene, ray or hit buffer");
    if (n == 0 || n > RRTE_QUERY_MAX_RAYS) return fail(c, RRTE_INVALID_ARG, "ray count %u outside [1, 2^24]", n);
    if (flags & ~RRTE_QUERY_ANY) return fail(c, RRTE_INVALID_ARG, "unknown query flags 0x%x", flags);
    return RRTE_OK;
}

}  // namespace

extern "C" {

rrte_status rrte_hip_raycast(rrte_ctx* c, const rrte_scene_ir* s, const rrte_ray* rays, uint32_t n, uint32_t flags,
                             rrte_ray_hit* hits_out) {
    if (!c) return RRTE_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    rrte_status r = query_args(c, s, rays, n, flags, hits_out);
    if (r != RRTE_OK) return r;
    return query_blocking(c, s, rays, sizeof(rrte_ray), n, flags, nullptr, hits_out);
}

rrte_status rrte_hip_raycast_async(rrte_ctx* c, const rrte_scene_ir* s, const void* d_rays, uint32_t n, uint32_t flags,
                                   void* d_hits, void* stream) {
    if (!c) return RRTE_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    rrte_status r = query_args(c, s, d_rays, n, flags, d_hits);
    if (r != RRTE_OK) return r;
    if (((uintptr_t)d_rays | (uintptr_t)d_hits) & 15u)
        return fail(c, RRTE_INVALID_ARG, "device ray and hit buffers must be 16-byte aligned");
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
    if ((r = query_scene(c, s, st)) != RRTE_OK) return r;
    return query_launch(c, s, d_rays, n, flags, nullptr, d_hits, st);
}

rrte_status rrte_hip_pick(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, const uint32_t* xy,
                          uint32_t n, rrte_ray_hit* hits_out) {
    if (!c) return RRTE_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (!p) return fail(c, RRTE_INVALID_ARG, "null params");
    rrte_status r = query_args(c, s, xy, n, RRTE_QUERY_CLOSEST, hits_out);
    if (r != RRTE_OK) return r;
    if (p->width == 0 || p->height == 0) return fail(c, RRTE_INVALID_ARG, "zero-sized frame %ux%u", p->width, p->height);
    if ((uint64_t)p->width * p->height > (1ull << 30)) return fail(c, RRTE_INVALID_ARG, "frame too large");
    for (uint32_t i = 0; i < n; ++i)
        if (xy[2 * (size_t)i] >= p->width || xy[2 * (size_t)i + 1] >= p->height)
            return fail(c, RRTE_INVALID_ARG, "pixel %u (%u, %u) outside the %ux%u frame", i, xy[2 * (size_t)i],
                        xy[2 * (size_t)i + 1], p->width, p->height);
    // the frame's camera record (make_params), for a frame of this size
    rrte_render_params pf{};
    pf.width = p->width;
    pf.height = p->height;
    pf.samples_per_pixel = 1;
    pf.gamma = 2.2f;
    pf.t_min = p->t_min;
    const KParams k = make_params(c, s, &pf, p->height);
    QueryCam qc{};
    qc.cam = k.cam[0];
    qc.width = p->width;
    qc.height = p->height;
    qc.t_min = p->t_min;
    return query_blocking(c, s, xy, 2 * sizeof(uint32_t), n, RRTE_QUERY_CLOSEST, &qc, hits_out);
}

}  // extern "C"
