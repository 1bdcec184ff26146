// gather.hip — the multi-GPU side: the RCCL communicator, a frame's row bands rendered per rank and
// gathered to the root over RCCL/xGMI (per frame or batched), the root's expansion of the gathered
// slabs, emulated peers, and the bounded waits that turn a stalled or dead peer into RRTE_RCCL_ERROR.
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstring>
#include <thread>

#include "context.hpp"

using namespace rrte;

extern "C" {  // (the two kernels keep the C names they had inside rrte_hip.hip)

// One empty kernel: a new stream's first dispatch (gather_frame).
__global__ void noop_kernel() {}

// The stalled-peer stand-in of RRTE_FAULT_STALL_GATHER: spins on a host-written flag (vector atomic
// loads at system scope) with its own 5 s deadline on the 100 MHz wall clock, so it always ends.
__global__ void stall_kernel(const uint32_t* flag) {
    const uint64_t t0 = wall_clock64();
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u &&
           wall_clock64() - t0 < 500000000ull) {
        __builtin_amdgcn_s_sleep(10);
    }
}

}  // extern "C"

namespace rrte {

// Root-side de-interleave after the RCCL gather: the gathered buffer holds, per rank (rank_stride
// bytes each; rank `skip_rank`'s rows -- the root's, rendered in place -- are skipped, ~0u for none),
// that rank's packed rows of `gridDim.z` frames back to back (frame_stride bytes each,
// `rows_cap` rows of RGBA8 or RGB24 per frame); frame z goes to full[z] (one frame per launch for
// per-frame gathers, a batch's frames for rrte_hip_set_gather_batch).  RGB24 slabs are expanded
// with alpha 255 (the host proved every alpha byte is 255).  VEC4: each lane moves 4 pixels (three
// dword loads for RGB24 or one dwordx4, one dwordx4 store) instead of 4 byte-wise pixels -- the
// host picks it when the width is a multiple of 4 and every target is 16-byte aligned (the slab
// strides are 256-byte aligned).  One workgroup row per image row, blockIdx.x strides the row.
struct DeinterleaveTargets {
    uint32_t* full[16];
};
template <bool RGB24, bool VEC4>
__global__ __launch_bounds__(256) void deinterleave_batch_kernel(const uint8_t* __restrict__ gathered,
                                                                 DeinterleaveTargets t, uint32_t width,
                                                                 BandMap bm, size_t rank_stride, size_t frame_stride,
                                                                 uint32_t skip_rank) {
    const uint32_t y = blockIdx.y;
    const uint32_t band_rows = bm.band_rows;
    const uint32_t band = y / band_rows, w = y - band * band_rows;
    uint32_t local_band = 0;
    const uint32_t rank = band_owner(bm, band, local_band);
    if (rank == skip_rank) return;  // the root's own bands: rendered into the frame in place
    const uint32_t lr = local_band * band_rows + w;
    constexpr uint32_t bpp = RGB24 ? 3u : 4u;
    const uint8_t* src = gathered + (size_t)rank * rank_stride + (size_t)blockIdx.z * frame_stride +
                         (size_t)lr * width * bpp;
    uint32_t* dst = t.full[blockIdx.z] + (size_t)y * width;
    const uint32_t step = gridDim.x * blockDim.x;
    if constexpr (VEC4) {
        const uint32_t n4 = width >> 2;
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += step) {
            uint4 o;
            if constexpr (RGB24) {
                // pixels 4i..4i+3 = bytes 12i..12i+11 = dwords 3i..3i+2 (little endian)
                const uint32_t* q = reinterpret_cast<const uint32_t*>(src) + 3u * i;
                const uint32_t d0 = __builtin_nontemporal_load(q), d1 = __builtin_nontemporal_load(q + 1),
                               d2 = __builtin_nontemporal_load(q + 2);
                o.x = d0 | 0xFF000000u;
                o.y = (d0 >> 24) | (d1 << 8) | 0xFF000000u;
                o.z = (d1 >> 16) | (d2 << 16) | 0xFF000000u;
                o.w = (d2 >> 8) | 0xFF000000u;
            } else {
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src) + i);
                o = make_uint4(v.x, v.y, v.z, v.w);
            }
            reinterpret_cast<uint4*>(dst)[i] = o;
        }
    } else {
        for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < width; x += step) {
            if constexpr (RGB24) {
                const uint8_t* q = src + 3u * x;
                dst[x] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | 0xFF000000u;
            } else {
                dst[x] = reinterpret_cast<const uint32_t*>(src)[x];
            }
        }
    }
}
static_assert(rrte_ctx::kMaxBatch == sizeof(DeinterleaveTargets::full) / sizeof(uint32_t*), "batch targets");

// Gather slabs carry RGB24 (3 B/pixel, 25 % fewer bytes over xGMI) when every pixel's alpha byte
// is provably 255.  LAMBERT_SHADOW never lets a light touch alpha (shade.hpp, shade_lambert):
// a sample's alpha is the background's (miss), 1 (no material, max_depth 0) or 1 + (a*0.1)*0.1 for
// the material's albedo alpha a, and the pixel's is rclamp((1 + sum of sample alphas) * inv_spp)
// (the sum starts from BLACK, alpha 1).  With every sample alpha >= 0 (spp 1) or >= 1 (spp n > 1:
// the sum is then >= n + 1 and (n + 1) * RN(1/n) >= 1), the clamp gives 1.0 and to_u8 255.  The
// test is on signs only (no host arithmetic to mirror); NaN fails it.  Every rank decides from the
// same scene and parameters, so all agree on the slab format.  RRTE_GATHER_RGB24=0 forces RGBA8.
static bool slab_rgb24(const rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p) {
    if (c->env.gather_rgba || (c->env.debug & ~4u) || p->mode != RRTE_MODE_LAMBERT_SHADOW) return false;
    const float thr = p->samples_per_pixel == 1 ? 0.0f : 1.0f;
    if (!(p->background[3] >= thr)) return false;
    for (uint32_t i = 0; i < s->num_materials; ++i)
        if (!(s->materials[i].albedo[3] >= 0.0f)) return false;
    return true;
}

// Issue the open batch (batched gather): the comm stream waits for its frames' renders, gathers all
// of them to the root in one ncclGather (each rank sends its frames' slices back to back) and
// de-interleaves every frame into its caller buffer.  Every rank holds the same open batch (same
// frames in the same order), so the collective matches.
// De-interleave `n` gathered frames (deinterleave_batch_kernel, above) on `st`.
static rrte_status deinterleave(rrte_ctx* c, hipStream_t st, const uint8_t* gathered, const DeinterleaveTargets& t,
                                uint32_t n, uint32_t width, uint32_t height, const BandMap& bm, bool rgb24,
                                size_t rank_stride, size_t frame_stride, uint32_t skip_rank = ~0u) {
    trace_rec(c, "launch expansion", st, nullptr, n, height);
    bool vec4 = width % 4u == 0;
    for (uint32_t j = 0; j < n; ++j) vec4 = vec4 && reinterpret_cast<uintptr_t>(t.full[j]) % 16u == 0;
    const uint32_t per = vec4 ? 1024u : 256u;  // pixels one workgroup moves per pass
    const dim3 dg(std::min((width + per - 1) / per, 8u), height, n), db(256);
    if (rgb24 && vec4)
        hipLaunchKernelGGL((deinterleave_batch_kernel<true, true>), dg, db, 0, st, gathered, t, width, bm, rank_stride, frame_stride, skip_rank);
    else if (rgb24)
        hipLaunchKernelGGL((deinterleave_batch_kernel<true, false>), dg, db, 0, st, gathered, t, width, bm, rank_stride, frame_stride, skip_rank);
    else if (vec4)
        hipLaunchKernelGGL((deinterleave_batch_kernel<false, true>), dg, db, 0, st, gathered, t, width, bm, rank_stride, frame_stride, skip_rank);
    else
        hipLaunchKernelGGL((deinterleave_batch_kernel<false, false>), dg, db, 0, st, gathered, t, width, bm, rank_stride, frame_stride, skip_rank);
    HIPCHK(c, hipGetLastError());
    return RRTE_OK;
}

// RRTE_EMULATE_PEERS (tests): render every peer's share of `n` frames -- peer q's bands under the plan's
// band partition, packed, in the plan's slab format (RGB24 or RGBA8) -- into its receive slot
// slab + q * rank_stride (frame j at + j * frame_stride), on `st`: the bytes a real peer would have
// sent with ncclSend for the same frames.  `base` is the root's plan of these frames.
static rrte_status render_peers(rrte_ctx* c, const LaunchPlan& base, const FrameCam* cams, uint32_t n, uint8_t* slab,
                                size_t rank_stride, size_t frame_stride, int root, hipStream_t st) {
    const BandMap bm{base.k.band_rows, (uint32_t)c->nranks, base.k.sky_bands, base.k.root_bands, base.k.peer_bands};
    for (int q = 0; q < c->nranks; ++q) {
        if (q == root) continue;
        LaunchPlan L = base;
        L.k.rank = (uint32_t)q;
        L.k.rows = rows_for_rank(base.k.height, bm.band_rows, c->nranks, q, bm.sky, bm.root_bands, bm.peer_bands);
        L.gy = tile_grid_rows(L.k, L.k.rows);
        L.k.out_image_rows = 0u;
        L.k.frame_stride = frame_stride;
        L.prof = 1 + (q - 1) % rrte_ctx::kBndChunksMax;  // (a tile profile per peer shape)
        for (uint32_t j0 = 0; j0 < n; j0 += kMaxLaunchFrames) {
            const uint32_t nf = std::min<uint32_t>(n - j0, kMaxLaunchFrames);
            memcpy(L.k.cam, cams + j0, nf * sizeof(FrameCam));
            L.k.nframes = nf;
            uint8_t* dst = slab + (size_t)q * rank_stride + (size_t)j0 * frame_stride;
            rrte_status r = issue_launch(c, L, reinterpret_cast<uint32_t*>(dst), nullptr, st);
            if (r != RRTE_OK) return r;
        }
    }
    return RRTE_OK;
}

// Launch the open batch's frames that have not been rendered yet ([rendered, n)) into its send slab on
// the slab's render stream, after the work queued on the frames' caller streams.  Local: no
// collective, so a rank may call it on its own (a scene change through a non-gather entry point,
// rrte_hip_synchronize) without desynchronising the ranks' gathers.
rrte_status render_batch(rrte_ctx* c, bool at_flush) {
    rrte_ctx::Batch& b = c->batch;
    if (b.rendered >= b.n) return RRTE_OK;
    HostSection hs(c);
    const int k = c->bslot;
    (void)at_flush;
    // The root renders its own bands straight into each frame's caller buffer at their image rows
    // (RGBA8; FrameCam::out): nothing of the root's share is copied, gathered or expanded.  Peers
    // render into the send slab (packed rows, RGB24 when alpha is provably 255).
    uint8_t* base = b.in_place ? nullptr : c->d_bsend[k];
    hipStream_t rs = c->render_stream[k];
    // the renders follow the frames' caller streams (scene uploads, the callers' own prior work) and
    // the slab's previous batch (its gather reads the send slab)
    if (!(c->env.diag_skip & 4u))
        for (uint32_t i = 0; i < b.nsrc; ++i) {
            HIPCHK(c, ev_record(c, b.ev_src[i], b.src[i], "record src (render)"));
            HIPCHK(c, ev_wait(c, rs, b.ev_src[i], "render waits src"));
        }
    if (b.rendered == 0) HIPCHK(c, ev_wait(c, rs, c->ev_batch[k], "render waits slab's last exchange"));
    hs.lap(2);
    // a copy of the batch's plan: b.plan's fields before KParams::nframes are the batch-compatibility
    // key gather_frame compares every new frame with, identically on every rank, so they stay as
    // planned (the in-place root's RGBA8 flag is this launch's business only)
    LaunchPlan L = b.plan;
    if (b.in_place) L.k.flags &= ~kFlagSlabRgb24;
    for (uint32_t j0 = b.rendered; j0 < b.n; j0 += kMaxLaunchFrames) {
        const uint32_t nf = std::min<uint32_t>(b.n - j0, kMaxLaunchFrames);
        memcpy(L.k.cam, b.cam + j0, nf * sizeof(FrameCam));
        L.k.nframes = nf;
        L.k.frame_stride = b.slice;
        L.k.out_image_rows = b.in_place ? 1u : 0u;
        uint8_t* dst = b.in_place ? nullptr : base + (size_t)j0 * b.slice;
        rrte_status r = issue_launch(c, L, reinterpret_cast<uint32_t*>(dst), nullptr, rs);
        if (r != RRTE_OK) return r;
    }
    b.rendered = b.n;
    HIPCHK(c, ev_record(c, c->ev_render[k], rs, "record render done"));
    hs.lap(3);
    return RRTE_OK;
}

// Before a collective on `st`: count it, and enqueue the injected stall if this is the one.
static rrte_status before_collective(rrte_ctx* c, hipStream_t st) {
    ++c->gathers_issued;
    if (c->env.fault_stall_at && !c->stall_fired && c->gathers_issued == c->env.fault_stall_at && c->h_stall) {
        __hip_atomic_store(c->h_stall.get(), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        uint32_t* dflag = nullptr;
        HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&dflag), c->h_stall.get(), 0));
        hipLaunchKernelGGL(stall_kernel, dim3(1), dim3(64), 0, st, dflag);
        HIPCHK(c, hipGetLastError());
        c->stall_armed = true;
        c->stall_fired = true;  // one-shot
    }
    return RRTE_OK;
}

// A call on the non-blocking communicator returned `r`: ncclInProgress means RCCL is still setting the
// operation up (connections, the communicator itself), and the next call may only follow once the
// communicator's state has left ncclInProgress -- polled under comm_timeout_ms.
rrte_status nccl_settle(rrte_ctx* c, ncclResult_t r, const char* what) {
    if (r == ncclSuccess) return RRTE_OK;
    if (r != ncclInProgress) return fail(c, RRTE_RCCL_ERROR, "%s failed: %s", what, ncclGetErrorString(r));
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0;; ++spin) {
        ncclResult_t st = ncclInProgress;
        if (ncclCommGetAsyncError(c->comm, &st) != ncclSuccess)
            return fail(c, RRTE_RCCL_ERROR, "%s: ncclCommGetAsyncError failed", what);
        if (st == ncclSuccess) return RRTE_OK;
        if (st != ncclInProgress) return fail(c, RRTE_RCCL_ERROR, "%s failed: %s", what, ncclGetErrorString(st));
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(c->comm_timeout_ms))
            return fail(c, RRTE_RCCL_ERROR, "%s did not complete within %u ms (a peer never joined?)", what,
                        c->comm_timeout_ms);
        if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

// A gather failed or did not finish in time: release any injected stall, give the queued work a short
// bounded chance to drain (so nothing of this communicator is still running when it is torn down),
// abort the communicator and fail every later gather call until rrte_hip_comm_init.
static rrte_status comm_abort(rrte_ctx* c, const char* why) {
    if (c->stall_armed && c->h_stall) __hip_atomic_store(c->h_stall.get(), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    c->stall_armed = false;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        bool busy = false;
        for (const Event& e : c->ev_poll)
            if (e && hipEventQuery(e) == hipErrorNotReady) busy = true;
        if (!busy || std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2000)) break;
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    if (c->comm) (void)ncclCommAbort(c->comm);
    c->comm = nullptr;
    c->comm_failed = true;
    c->comm_fail_msg = why;
    rrte_ctx::Batch& b = c->batch;
    b.n = b.nsrc = b.rendered = 0;
    c->last_gather_stream = nullptr;
    c->last_gather_ev = nullptr;
    return fail(c, RRTE_RCCL_ERROR, "%s; communicator aborted (call rrte_hip_comm_init again)", why);
}

// Bounded wait for events: polls them (and, while a communicator exists, ncclCommGetAsyncError)
// instead of blocking, so work that sits behind a gather that never completes -- a dead or stalled
// peer -- surfaces as RRTE_RCCL_ERROR after comm_timeout_ms (the communicator aborted) instead of a
// hang.  Without a communicator no gather can stall a frame (an aborted one's kernels are being torn
// down), so the wait lasts as long as the device needs up to RRTE_NOCOMM_WAIT_MS (default 10 minutes,
// far above any queue of frames; RRTE_HIP_ERROR after it so a hung or faulted kernel still returns;
// 0 = no limit).
rrte_status poll_events(rrte_ctx* c, const Event* ev, size_t n) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t limit_ms = c->comm ? c->comm_timeout_ms : c->env.nocomm_wait_ms;
    for (uint32_t spin = 0;; ++spin) {
        bool busy = false;
        for (size_t i = 0; i < n; ++i) {
            const hipError_t e = hipEventQuery(ev[i]);
            if (e == hipErrorNotReady) {
                busy = true;
                break;
            }
            HIPCHK(c, e);
        }
        if (!busy) return RRTE_OK;
        const bool late = std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(limit_ms);
        if (c->comm) {
            ncclResult_t ae = ncclSuccess;
            if (ncclCommGetAsyncError(c->comm, &ae) == ncclSuccess && ae != ncclSuccess && ae != ncclInProgress) {
                char why[256];
                snprintf(why, sizeof why, "RCCL asynchronous error: %s", ncclGetErrorString(ae));
                return comm_abort(c, why);
            }
            if (late) {
                char why[256];
                snprintf(why, sizeof why, "gather did not complete within %u ms (stalled or dead peer?)", c->comm_timeout_ms);
                return comm_abort(c, why);
            }
        } else if (late && limit_ms) {
            return fail(c, RRTE_HIP_ERROR, "device work did not complete within %u ms", limit_ms);
        }
        if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

// Bounded wait for the context's own streams and its last gather (poll_events).
rrte_status wait_bounded(rrte_ctx* c) {
    constexpr int kPoll = 3 + rrte_ctx::kBatchSlabs;
    static_assert(sizeof(c->ev_poll) / sizeof(c->ev_poll[0]) == kPoll, "poll events");
    hipStream_t ss[kPoll] = {c->stream, c->comm_stream, c->last_gather_stream};
    for (int i = 0; i < rrte_ctx::kBatchSlabs; ++i) ss[3 + i] = c->render_stream[i];
    size_t n = 0;
    for (int i = 0; i < kPoll; ++i) {
        if (!ss[i]) continue;
        HIPCHK(c, c->ev_poll[n].create());
        HIPCHK(c, hipEventRecord(c->ev_poll[n], ss[i]));
        ++n;
    }
    return poll_events(c, c->ev_poll, n);
}

// Close the open batch (collective: every rank holds the same open batch -- same frames in the same
// order -- so the ncclGather matches): render what is not rendered yet, then ONE ncclGather on the
// comm stream moves every frame's slices to the root, which de-interleaves each into its caller
// buffer.  Any failure resets the batch and aborts the communicator: a half-issued batch would leave
// the ranks' collectives out of step.
static rrte_status flush_batch(rrte_ctx* c) {
    rrte_ctx::Batch& b = c->batch;
    if (b.n == 0) return RRTE_OK;
    if (c->comm_failed || !c->comm) {
        b.n = b.nsrc = b.rendered = 0;
        return fail(c, RRTE_RCCL_ERROR, "gather batch dropped: %s", c->comm_failed ? c->comm_fail_msg.c_str() : "no communicator");
    }
    const bool launched_per_frame = b.per_frame;
    rrte_status r = launched_per_frame ? RRTE_OK : render_batch(c, true);
    if (r != RRTE_OK) return comm_abort(c, ("batch render failed: " + c->err).c_str());
    HostSection hs(c);
    const int k = c->bslot;
    const size_t count = (size_t)b.n * b.slice;  // bytes per rank
    auto issue = [&]() -> rrte_status {
        if (launched_per_frame) {
            // the frames rendered on their callers' streams: the exchange follows each of them
            for (uint32_t i = 0; i < b.nsrc; ++i) {
                HIPCHK(c, ev_record(c, b.ev_src[i], b.src[i], "record src (exchange)"));
                HIPCHK(c, ev_wait(c, c->comm_stream, b.ev_src[i], "comm waits src"));
            }
        } else {
            HIPCHK(c, ev_wait(c, c->comm_stream, c->ev_render[k], "comm waits render"));
        }
        if (c->last_gather_stream && c->last_gather_stream != c->comm_stream)
            HIPCHK(c, ev_wait(c, c->comm_stream, c->last_gather_ev, "comm waits last gather"));
        hs.lap(4);
        if ((r = before_collective(c, c->comm_stream)) != RRTE_OK) return r;
        // every peer's slab to the root: grouped point-to-point (the root's own bands never move); with
        // a 1-rank communicator (emulated ranks, RRTE_EMULATE_RANK) there is no peer, RRTE_GATHER_SELF
        // routes the root's bands through RCCL to itself
        const bool self_only = c->comm_size == 1;  // (no real peer: only the root's RRTE_GATHER_SELF round trip)
        if (!(c->env.diag_skip & 1u) && (!self_only || (!b.in_place && c->rank == b.root))) {
            // (a failing call inside the group still closes it before the error is returned, so the
            // thread's group depth is balanced when comm_abort tears the communicator down)
            NCCLCHK(c, ncclGroupStart());
            ncclResult_t gr = ncclSuccess;
            const char* what = "ncclRecv";
            if (c->rank == b.root) {
                for (int q = 0; q < c->comm_size && (gr == ncclSuccess || gr == ncclInProgress); ++q)
                    if (q != b.root || !b.in_place)
                        gr = ncclRecv(c->d_brecv[k] + (size_t)q * count, count, ncclUint8, q, c->comm, c->comm_stream);
            }
            if ((gr == ncclSuccess || gr == ncclInProgress) && (c->rank != b.root || !b.in_place)) {
                what = "ncclSend";
                gr = ncclSend(c->d_bsend[k], count, ncclUint8, b.root, c->comm, c->comm_stream);
            }
            const ncclResult_t er = ncclGroupEnd();
            if (gr != ncclSuccess && gr != ncclInProgress)
                return fail(c, RRTE_RCCL_ERROR, "%s failed: %s", what, ncclGetErrorString(gr));
            NCCLCHK(c, er);
        }
        if (self_only && c->env.emu_peers > 1 && c->rank == b.root &&
            (r = render_peers(c, b.plan, b.cam, b.n, c->d_brecv[k], count, b.slice, b.root, c->comm_stream)) != RRTE_OK)
            return r;
        hs.lap(5);
        if (c->rank == b.root && !(c->env.diag_skip & 2u) && (c->nranks > 1 || !b.in_place)) {
            DeinterleaveTargets t{};
            for (uint32_t j = 0; j < b.n; ++j) t.full[j] = b.full[j];
            if ((r = deinterleave(c, c->comm_stream, c->d_brecv[k], t, b.n, b.width, b.height, b.bm, b.rgb24, count,
                                  b.slice, b.in_place ? (uint32_t)b.root : ~0u)) != RRTE_OK)
                return r;
        }
        hs.lap(6);
        HIPCHK(c, ev_record(c, c->ev_batch[k], c->comm_stream, "record exchange done"));
        return RRTE_OK;
    };
    if ((r = issue()) != RRTE_OK) return comm_abort(c, ("batch gather failed: " + c->err).c_str());
    c->last_gather_stream = c->comm_stream;
    c->last_gather_ev = c->ev_batch[k];
    c->bslot = (k + 1) % c->env.batch_slabs;
    b.n = b.nsrc = b.rendered = 0;
    hs.lap(7);
    return RRTE_OK;
}

// One multi-GPU frame on `st`: render this rank's bands into its slice of a gather slab, gather it to
// the root and de-interleave there -- per frame (gather batch 1: everything on `st`, in place, the
// frames' gathers chained across streams in issue order), or batched (the gather happens when the
// open batch is full or flushed, on the comm stream).  `timing` (the blocking entry point): ev1 marks
// the end of the render for rrte_stats.
static rrte_status gather_frame(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, int root,
                                void* d_full, hipStream_t st, bool timing) {
    HostSection hs(c);
    rrte_status r = validate(c, s, p);
    if (r != RRTE_OK) return r;
    if (root < 0 || root >= c->nranks) return fail(c, RRTE_INVALID_ARG, "root %d out of range", root);
    if (c->rank == root && !d_full) return fail(c, RRTE_INVALID_ARG, "root needs an output buffer");
    double up = 0.0;
    hs.lap(0);
    if ((r = upload_scene(c, s, st, &up)) != RRTE_OK) return r;
    hs.lap(1);
    const uint32_t band = p->band_rows ? p->band_rows : 16;
    rrte_render_params pp = *p;
    pp.band_rows = band;
    uint32_t rows = p->height, cap = p->height;  // this rank's rows; slab rows (the most any rank owns)
    const bool rgb24 = slab_rgb24(c, s, p);
    // A frame joining an open batch of the same frame geometry keeps the batch's band partition: which
    // rank renders a band is a work-balance choice, never a pixel, and every rank makes the same one
    // from the same calls -- so a moving camera neither recomputes the partition every frame nor
    // closes the batch whenever its sky-band count changes
    const rrte_ctx::Batch& ob = c->batch;
    const bool join = c->nranks > 1 && c->gather_batch > 1 && !timing && ob.n && ob.width == p->width &&
                      ob.height == p->height && ob.band == band && ob.root == root && ob.rgb24 == rgb24;
    BandMap bm{band, 1u, 0u, 1u, 1u};
    if (join) {
        bm = ob.bm;
        rows = ob.plan.k.rows;
    } else if (c->nranks > 1) {
        bm = frame_band_map(c, s, &pp, root, &rows, &cap);
    }
    // bytes per rank slot, 256-B aligned so every rank's send buffer starts aligned
    const size_t slice = join ? ob.slice : ((size_t)cap * p->width * (rgb24 ? 3u : 4u) + 255u) & ~(size_t)255u;
    const uint32_t kflags = rgb24 ? kFlagSlabRgb24 : 0u;
    if (c->comm_failed)
        return fail(c, RRTE_RCCL_ERROR, "communicator aborted earlier (%s); call rrte_hip_comm_init", c->comm_fail_msg.c_str());
    // one rank: no exchange (RRTE_FORCE_GATHER=1 still takes the gather path: tests on one GPU)
    if (c->nranks == 1 && !(c->env.force_gather && c->comm)) {
        r = launch(c, s, p, p->height, static_cast<uint32_t*>(d_full), nullptr, st);
        if (r == RRTE_OK) c->pending_primary = (uint64_t)p->width * p->height * p->samples_per_pixel;
        if (timing) HIPCHK(c, hipEventRecord(c->ev1, st));
        return r;
    }
    if (!c->comm) return fail(c, RRTE_INVALID_ARG, "rrte_hip_comm_init has not been called");
    if (c->gather_batch > 1 && !timing) {
        rrte_ctx::Batch& b = c->batch;
        if (!c->comm_stream) {
            // the comm stream's gathers and de-interleaves at the highest priority: its kernels are
            // dispatched ahead of the next batches' render workgroups instead of queueing behind them
            // (RRTE_COMM_PRIORITY=0: default priority, A/B)
            int lo = 0, hi = 0;
            HIPCHK(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
            HIPCHK(c, c->comm_stream.create(c->env.comm_priority ? hi : lo));
            for (int i = 0; i < c->env.batch_slabs; ++i) {  // (only the slots of the ring in use)
                HIPCHK(c, c->render_stream[i].create());
                HIPCHK(c, c->ev_batch[i].create());
                HIPCHK(c, c->ev_render[i].create());
            }
            // one empty kernel on each new stream now: the runtime binds a stream to a hardware queue at
            // its first dispatch, which must not happen inside a later frame's critical path
            for (int i = 0; i < c->env.batch_slabs; ++i) {
                hipLaunchKernelGGL(noop_kernel, dim3(1), dim3(64), 0, c->render_stream[i]);
                HIPCHK(c, hipGetLastError());
            }
            hipLaunchKernelGGL(noop_kernel, dim3(1), dim3(64), 0, c->comm_stream);
            HIPCHK(c, hipGetLastError());
            for (int i = 0; i < rrte_ctx::kMaxBatch; ++i)
                HIPCHK(c, b.ev_src[i].create());
        }
        LaunchPlan L = plan_launch(c, s, &pp, rows, kflags, 0u, &bm);
        // a frame of another size, band, root, slab format or render setup closes the open batch
        // (the cameras and tile rectangles are per frame; everything before KParams::nframes is not)
        if (b.n && (b.width != p->width || b.height != p->height || b.band != band || b.root != root ||
                    b.rgb24 != rgb24 || b.slice != slice || b.plan.mode != L.mode || b.plan.cull != L.cull ||
                    b.plan.single != L.single || memcmp(&b.plan.k, &L.k, offsetof(KParams, nframes))))
            if ((r = flush_batch(c)) != RRTE_OK) return r;
        const int k = c->bslot;
        if (b.n == 0) {
            b.cap = c->gather_batch;
            b.width = p->width;
            b.height = p->height;
            b.band = band;
            b.root = root;
            b.rgb24 = rgb24;
            b.slice = slice;
            b.bm = bm;
            b.plan = L;
            b.in_place = c->rank == root && !c->env.gather_self;
            b.per_frame = !c->env.batch_launch;
            // every rank holds a receive slab too (the root's is the only one written)
            const size_t send = (size_t)b.cap * slice, recv = send * (size_t)c->nranks;
            if (c->d_bsend[k].cap() < send || c->d_brecv[k].cap() < recv) {
                // every slab of the ring in use at once (at the first batch: none is allocated inside a
                // later timed batch); a smaller slab an in-flight gather may still use goes to the
                // graveyard (freed when the context is next idle), so nothing waits for the device here
                for (int q = 0; q < c->env.batch_slabs; ++q) {
                    if ((r = ensure(c, c->d_bsend[q], send)) != RRTE_OK) return r;
                    if ((r = ensure(c, c->d_brecv[q], recv)) != RRTE_OK) return r;
                }
            }
        }
        hs.lap(2);
        b.cam[b.n] = L.k.cam[0];
        b.cam[b.n].out = static_cast<uint32_t*>(d_full);
        b.full[b.n] = static_cast<uint32_t*>(d_full);
        uint32_t i = 0;
        while (i < b.nsrc && b.src[i] != st) ++i;
        const bool new_src = i == b.nsrc;
        if (new_src) b.src[b.nsrc++] = st;
        if (b.per_frame) {
            // render now, on the caller's stream: the root straight into the frame at its image rows
            // (RGBA8), a peer into its slot of the send slab -- after that slab's previous exchange
            // (once per stream and batch)
            if (b.in_place) {
                L.k.flags &= ~kFlagSlabRgb24;
                L.k.out_image_rows = 1u;
                L.k.cam[0].out = static_cast<uint32_t*>(d_full);
                if ((r = issue_launch(c, L, nullptr, nullptr, st)) != RRTE_OK) return r;
            } else {
                if (new_src) HIPCHK(c, hipStreamWaitEvent(st, c->ev_batch[k], 0));
                uint8_t* dst = c->d_bsend[k] + (size_t)b.n * b.slice;
                if ((r = issue_launch(c, L, reinterpret_cast<uint32_t*>(dst), nullptr, st)) != RRTE_OK) return r;
            }
            b.rendered = b.n + 1;
        }
        ++b.n;
        hs.lap(3);
        if (b.n == b.cap && (r = flush_batch(c)) != RRTE_OK) return r;
    } else {
        if ((r = flush_batch(c)) != RRTE_OK) return r;  // keep every rank's collectives in issue order
        if (!c->ev_gath[0])
            for (int i = 0; i < rrte_ctx::kSlabs; ++i)
                HIPCHK(c, c->ev_gath[i].create());
        // slabs are a ring shared by every frame in flight: a frame on another stream than the slab's
        // previous user waits until that frame has been gathered (same stream: stream order suffices)
        const int slot = (int)(c->gather_frames % rrte_ctx::kSlabs);
        const size_t slab_words = slice * (size_t)c->nranks / 4u;
        if (c->d_slab[slot].cap() < slab_words) {
            // (re)size the whole ring at once; smaller slabs in-flight gathers may still use go to the
            // graveyard (freed when the context is next idle): no device synchronisation
            for (int i = 0; i < rrte_ctx::kSlabs; ++i)
                if ((r = ensure(c, c->d_slab[i], slab_words)) != RRTE_OK) return r;
        }
        uint8_t* slab = reinterpret_cast<uint8_t*>(c->d_slab[slot].get());
        uint8_t* mine = slab + (size_t)c->rank * slice;  // in-place send slot
        if (c->slab_stream[slot] && c->slab_stream[slot] != st)
            HIPCHK(c, hipStreamWaitEvent(st, c->ev_gath[slot], 0));
        hs.lap(2);
        if ((r = launch(c, s, &pp, rows, reinterpret_cast<uint32_t*>(mine), nullptr, st, kflags, 0u, 0, &bm)) != RRTE_OK)
            return r;
        if (c->comm_size == 1 && c->env.emu_peers > 1 && c->rank == root) {  // RRTE_EMULATE_PEERS (tests)
            const LaunchPlan L = plan_launch(c, s, &pp, rows, kflags, 0u, &bm);
            if ((r = render_peers(c, L, L.k.cam, 1, slab, slice, 0, root, st)) != RRTE_OK) return r;
        }
        hs.lap(3);
        if (timing) HIPCHK(c, hipEventRecord(c->ev1, st));
        // gathers on one communicator must run in the same order on every rank: a frame on another
        // stream than the previous gather waits for it
        if (c->last_gather_stream && c->last_gather_stream != st)
            HIPCHK(c, hipStreamWaitEvent(st, c->last_gather_ev, 0));
        hs.lap(4);
        if ((r = before_collective(c, st)) != RRTE_OK) return comm_abort(c, ("gather setup failed: " + c->err).c_str());
        {
            const ncclResult_t nr = ncclGather(mine, slab, slice, ncclUint8, root, c->comm, st);
            if (nr != ncclSuccess && nccl_settle(c, nr, "ncclGather") != RRTE_OK) return comm_abort(c, c->err.c_str());
        }
        hs.lap(5);
        if (c->rank == root) {
            DeinterleaveTargets t{};
            t.full[0] = static_cast<uint32_t*>(d_full);
            if ((r = deinterleave(c, st, slab, t, 1, p->width, p->height, bm, rgb24, slice, 0)) != RRTE_OK)
                return comm_abort(c, ("de-interleave failed: " + c->err).c_str());
        }
        hs.lap(6);
        HIPCHK(c, hipEventRecord(c->ev_gath[slot], st));
        c->slab_stream[slot] = st;
        c->last_gather_stream = st;
        c->last_gather_ev = c->ev_gath[slot];
        hs.lap(7);
        ++c->gather_frames;
    }
    ++c->hp_frames;
    c->pending_primary = (uint64_t)p->width * rows * p->samples_per_pixel;
    c->stats.upload_ms = up;
    c->stats.frames++;
    return RRTE_OK;
}

// The code object of this file (the expansion kernels), loaded at rrte_hip_create and not inside the
// first gathered frame.
hipError_t load_gather_kernels() {
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&noop_kernel));
}

}  // namespace rrte

extern "C" {

rrte_status rrte_hip_comm_unique_id(uint8_t out_id[RRTE_UNIQUE_ID_BYTES]) {
    if (!out_id) return RRTE_INVALID_ARG;
    static_assert(sizeof(ncclUniqueId) == RRTE_UNIQUE_ID_BYTES, "unique id size");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return RRTE_RCCL_ERROR;
    memcpy(out_id, &id, sizeof id);
    return RRTE_OK;
}

rrte_status rrte_hip_comm_init(rrte_ctx* c, int nranks, int rank, const uint8_t id_bytes[RRTE_UNIQUE_ID_BYTES]) {
    if (!c || !id_bytes || nranks < 1 || rank < 0 || rank >= nranks) return fail(c, RRTE_INVALID_ARG, "bad comm args");
    HIPCHK(c, hipSetDevice(c->device));
    // frames already accepted into an open batch are gathered on the old communicator first (every rank
    // re-initialises together, so this collective matches); then nothing of the old one may still run
    rrte_status fr = c->comm ? flush_batch(c) : RRTE_OK;
    c->batch.n = c->batch.nsrc = c->batch.rendered = 0;
    if (fr == RRTE_OK && c->comm) fr = wait_bounded(c);
    if (fr == RRTE_OK) {  // the frames on caller streams too (bounded)
        if ((fr = retire(c, c->launched)) == RRTE_OK) fr = wait_retired(c, c->launched);
    }
    if (c->comm) ncclCommDestroy(c->comm);
    c->comm = nullptr;
    c->last_gather_stream = nullptr;
    c->last_gather_ev = nullptr;
    c->comm_failed = false;
    c->comm_fail_msg.clear();
    c->gathers_issued = 0;
    if (fr != RRTE_OK) return fr;
    ncclUniqueId id;
    memcpy(&id, id_bytes, sizeof id);
    // Non-blocking initialisation, polled under the same timeout as every gather wait: a peer that
    // never joins surfaces as RRTE_RCCL_ERROR instead of a hang in ncclCommInitRank.  (Every later call
    // on the communicator may then return ncclInProgress: nccl_settle.)
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 0;
    const ncclResult_t ir = ncclCommInitRankConfig(&c->comm, nranks, id, rank, &cfg);
    if (ir != ncclSuccess && ir != ncclInProgress) {
        if (c->comm) (void)ncclCommAbort(c->comm);
        c->comm = nullptr;
        return fail(c, RRTE_RCCL_ERROR, "ncclCommInitRankConfig failed: %s", ncclGetErrorString(ir));
    }
    if (rrte_status r = nccl_settle(c, ir, "ncclCommInitRankConfig"); r != RRTE_OK) {
        if (c->comm) (void)ncclCommAbort(c->comm);
        c->comm = nullptr;
        c->comm_failed = false;  // (no communicator: a later comm_init starts clean)
        return r;
    }
    c->nranks = nranks;
    c->rank = rank;
    c->comm_size = nranks;
    if (nranks == 1 && c->env.emu_peers > 1) {
        // RRTE_EMULATE_PEERS=N: the root of N ranks whose peers' shares it renders itself (render_peers)
        c->nranks = c->env.emu_peers;
        c->rank = 0;
    } else if (nranks == 1 && c->env.emu_nranks > 1) {
        // RRTE_EMULATE_RANK=N:R with a 1-rank communicator (diagnostic, one GPU): the gather path lays
        // frames out as rank R of N -- R's bands rendered into its slab slice, the 1-rank gather moving
        // that slice, and on rank 0 the de-interleave of all N slices (the other N-1 hold whatever the
        // receive buffer held) -- i.e. one rank's whole per-frame cost except the xGMI transfers.
        c->nranks = c->env.emu_nranks;
        c->rank = c->env.emu_rank;
    }
    return RRTE_OK;
}

rrte_status rrte_hip_render_gather_async(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, int root,
                                         void* d_full, void* stream) {
    if (!c) return RRTE_INVALID_ARG;
    dump_if_asked(c, s, p);
    return gather_frame(c, s, p, root, d_full, stream ? static_cast<hipStream_t>(stream) : c->stream, false);
}

rrte_status rrte_hip_set_gather_batch(rrte_ctx* c, uint32_t frames) {
    if (!c) return RRTE_INVALID_ARG;
    if (frames < 1 || frames > (uint32_t)rrte_ctx::kMaxBatch)
        return fail(c, RRTE_INVALID_ARG, "gather batch %u outside [1, %d]", frames, rrte_ctx::kMaxBatch);
    rrte_status r = flush_batch(c);
    if (r != RRTE_OK) return r;
    c->gather_batch = frames;
    return RRTE_OK;
}

rrte_status rrte_hip_flush(rrte_ctx* c) {
    if (!c) return RRTE_INVALID_ARG;
    return flush_batch(c);
}

rrte_status rrte_hip_gather_info(rrte_ctx* c, uint64_t* collectives, uint32_t* open_frames) {
    if (!c || !collectives || !open_frames) return RRTE_INVALID_ARG;
    *collectives = c->gathers_issued;
    *open_frames = c->batch.n;
    return RRTE_OK;
}

rrte_status rrte_hip_render_gather(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, int root,
                                   uint8_t* out) {
    if (!c) return RRTE_INVALID_ARG;
    dump_if_asked(c, s, p);
    rrte_status r = validate(c, s, p);
    if (r != RRTE_OK) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t npix = (size_t)p->width * p->height;
    uint32_t* full = nullptr;
    if (c->rank == root) {
        if ((r = ensure(c, c->d_full, npix)) != RRTE_OK) return r;
        full = c->d_full;
    }
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if ((r = gather_frame(c, s, p, root, full, c->stream, true)) != RRTE_OK) return r;
    HIPCHK(c, hipEventRecord(c->ev2, c->stream));
    if (c->rank == root && out) HIPCHK(c, hipMemcpyAsync(out, full, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if ((r = wait_bounded(c)) != RRTE_OK) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float k_ms = 0.0f, all_ms = 0.0f;
    if (c->nranks > 1) {
        (void)hipEventElapsedTime(&k_ms, c->ev0, c->ev1);
        (void)hipEventElapsedTime(&all_ms, c->ev0, c->ev2);
        c->stats.kernel_ms = k_ms;
        c->stats.gather_ms = all_ms - k_ms;
    }
    return finish_frame(c);
}

}  // extern "C"
