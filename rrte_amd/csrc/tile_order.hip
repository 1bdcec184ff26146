// tile_order.hip — the measured-cost tile order of a launch (rrte_ctx::TileProfile, KParams::hot):
// profiling a launch shape, composing the order off the render thread, and the pool of device list
// versions.  issue_launch calls plan_tile_order before the launch and finish_tile_order after it.
// Host only: no kernel is instantiated here.
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <future>

#include "context.hpp"

using namespace rrte;

namespace rrte {

// Measured-cost tile order (rrte_ctx::TileProfile, KParams::hot).
constexpr uint64_t kTileReprofile = 256;  // launches of one shape between two profiles (each costs a list upload)
constexpr uint64_t kTileReprofileMoving = 32;  // ... when the camera has moved since the last profile

static uint64_t fnv1a(const void* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
    return h;
}

// Every tile of a profile (costs[0 .. n), tiles_x per row), slowest first (longest-processing-time
// order), as packed slots: a counting sort on 65536 cost buckets (ties in tile order), O(tiles) on the
// host.
static std::vector<uint32_t> lpt_slots(const uint32_t* costs, uint32_t n, uint32_t tiles_x) {
    std::vector<uint32_t> slots;
    if (n == 0 || tiles_x == 0) return slots;
    uint32_t mx = 0;
    for (uint32_t i = 0; i < n; ++i) mx = std::max(mx, costs[i]);
    constexpr uint32_t B = 65536;
    std::vector<uint32_t> cnt(B + 1, 0u);
    auto bucket = [&](uint32_t c) { return B - 1 - (mx ? (uint32_t)((uint64_t)c * (B - 1) / mx) : 0u); };
    for (uint32_t i = 0; i < n; ++i) ++cnt[bucket(costs[i])];
    uint32_t acc = 0;
    for (uint32_t b = 0; b <= B; ++b) {
        const uint32_t c = cnt[b];
        cnt[b] = acc;
        acc += c;
    }
    slots.resize(n);
    for (uint32_t i = 0; i < n; ++i) slots[cnt[bucket(costs[i])]++] = hot_pack(i % tiles_x, i / tiles_x);
    return slots;
}

// RRTE_TILE_ORDER=2 (tests): every tile once in a fixed scrambled order -- slot k takes tile
// (k * stride) mod n for a stride near 0.618 n coprime with n -- so the list path runs on every launch
// without a profile.
static std::vector<uint32_t> fixed_slots(uint32_t n, uint32_t tiles_x) {
    std::vector<uint32_t> slots(n);
    uint64_t stride = std::max<uint64_t>(1, (uint64_t)(0.618034 * n));
    auto gcd = [](uint64_t a, uint64_t b) { while (b) { const uint64_t t = a % b; a = b; b = t; } return a; };
    while (n > 1 && gcd(stride, n) != 1) ++stride;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t i = (uint32_t)((k * stride) % n);
        slots[k] = hot_pack(i % tiles_x, i / tiles_x);
    }
    return slots;
}

// Words per XCD of a tile list of n slots stored XCD-major (KParams::hot_stride).
static uint32_t hot_stride(uint32_t n) { return (n + 7u) / 8u; }

// Allocates what an upload of up to `words` list words needs -- the pinned staging arena and the device
// versions not yet allocated -- at profile time, so the first upload (inside a later render call)
// allocates nothing.  The copies run on the context's upload stream, created with the context: a
// stream's first use sets up its hardware queue (~8 ms measured, profiles/r06_engine_loop_trace.log),
// which must not land in a frame.  false = not now (a copy out of the arena is still pending).
static bool reserve_hot_lists(rrte_ctx::TileProfile& tp, size_t words) {
    constexpr int K = rrte_ctx::TileProfile::kVersions;
    if (tp.arena_words < words) {
        for (int i = 0; i < K; ++i)
            if (tp.ver[i].ev_up && hipEventQuery(tp.ver[i].ev_up) != hipSuccess) return false;
        tp.arena_words = 0;
        if (tp.h_arena.grow(K * words) != hipSuccess) return false;
        tp.arena_words = words;
    }
    for (int i = 0; i < K; ++i)
        if (!tp.d_list[i] && tp.d_list[i].alloc(words) != hipSuccess) return false;
    return true;
}

// Uploads the composed slots into a free version of the device list; false leaves the launch on the
// current list (or in image order) -- it never waits for the device.  The current version is retired
// first; a version is free once every launch that read it has completed (struct Retire).  The copy
// runs on the list's own upload stream; its event orders every stream's first launch that reads the
// version after it (plan_tile_order), so every launch sees a whole list and no render call waits.
static bool upload_hot_list(rrte_ctx* c, rrte_ctx::TileProfile& tp) {
    constexpr int K = rrte_ctx::TileProfile::kVersions;
    int pick = -1;
    for (int k = 1; k <= K && pick < 0; ++k) {  // the oldest retired version first
        const int v = (int)((tp.uploads + (uint64_t)k) % K);
        if (v != tp.cur && tp.ver[v].retired_done()) pick = v;
    }
    if (pick < 0) return false;
    trace_rec(c, "hot-list upload: begin", nullptr, nullptr, (uint32_t)pick);
    tp.ver[pick].ret.nev = 0;
    const size_t n = tp.slots.size(), stride = hot_stride((uint32_t)n);
    const size_t words = 8u * stride;  // XCD-major (KParams::hot_stride)
    const size_t bytes = words * sizeof(uint32_t);
    // (a larger frame: its launches have completed, the old buffer is idle)
    if (ensure(c, tp.d_list[pick], words) != RRTE_OK) return false;
    trace_rec(c, "hot-list upload: device buffer", nullptr, nullptr, (uint32_t)pick);
    if (!reserve_hot_lists(tp, words)) return false;
    trace_rec(c, "hot-list upload: reserved", nullptr, nullptr, (uint32_t)pick);
    uint32_t* stage = tp.h_arena + (size_t)pick * tp.arena_words;
    for (size_t k = 0; k < n; ++k) stage[(k & 7u) * stride + (k >> 3)] = tp.slots[k];
    // fault injection for the device index check (tests): only where the check stops the wave first
    if (c->env.fault_bad_slot == 1 && (c->env.debug & 4u) && n) stage[0] = hot_pack(0u, 0xfff0u);
    if (tp.ver[pick].ev_up.create() != hipSuccess) return false;
    trace_rec(c, "hot-list upload: staged", nullptr, nullptr, (uint32_t)pick);
    if (hipMemcpyAsync(tp.d_list[pick], stage, bytes, hipMemcpyHostToDevice, c->upload_stream) != hipSuccess)
        return false;
    trace_rec(c, "hot-list upload: copy queued", c->upload_stream, nullptr, (uint32_t)bytes);
    if (tp.ver[pick].published(c->upload_stream) != hipSuccess) return false;
    if (tp.cur >= 0 && tp.ver[tp.cur].retire(c) != RRTE_OK) return false;
    tp.cur = pick;
    ++tp.uploads;
    return true;
}

// Sets the plan's tile order (slot list, tile profile) for a launch of kernel `kern`; true when this
// launch is profiled (the caller copies the durations back after it).
bool plan_tile_order(rrte_ctx* c, LaunchPlan& L, const void* kern, hipStream_t st) {
    KParams& k = L.k;
    k.tiles_x = L.gx;
    k.hot = nullptr;
    k.hot_n = 0;
    k.hot_stride = 0;
    k.tile_cost = nullptr;
    // (RRTE_DEBUG bit 5 runs one workgroup in image-order numbering: no tile order; bit 4's per-wave
    // stamps work with it)
    if (!c->env.tile_order || L.gx > 0xffffu || L.gy > 0xffffu || (k.debug & 32u)) return false;
    auto& tp = c->tprof[L.prof];
    std::string key(reinterpret_cast<const char*>(&kern), sizeof kern);
    const uint32_t shape[] = {k.width, k.height, k.rows, k.row0, k.band_rows, k.nranks, k.rank, k.spp, k.max_depth,
                              (uint32_t)L.mode, (uint32_t)L.cull, (uint32_t)L.single, k.tile_shift};
    key.append(reinterpret_cast<const char*>(shape), sizeof shape);
    const uint32_t tiles = L.gx * L.gy;
    if (tp.pending && hipEventQuery(tp.ev) == hipSuccess) {
        trace_rec(c, "tile plan: profile landed", st, nullptr);
        tp.pending = false;
        if (tp.pending_key == key) {
            // the order is composed on a worker thread from a copy of the durations: a whole frame's
            // counting sort takes ~0.5 ms of host time that a render call must not stall for
            std::vector<uint32_t> costs(tp.h_cost.get(), tp.h_cost.get() + tp.tiles);
            const uint32_t tx = tp.tiles_x;
            tp.work = std::async(std::launch::async, [key, costs = std::move(costs), tx]() {
                return TilePlanResult{key, lpt_slots(costs.data(), (uint32_t)costs.size(), tx)};
            });
            tp.working = true;
            tp.launches = 0;
            ++tp.profiles;
        }
    }
    if (tp.working && tp.work.wait_for(std::chrono::seconds(0)) == std::future_status::ready) {
        trace_rec(c, "tile plan: worker result", st, nullptr);
        TilePlanResult r = tp.work.get();
        tp.working = false;
        if (r.key == key && r.slots.size() == tiles) {  // (a result for another shape is dropped)
            tp.key = key;
            tp.slots = std::move(r.slots);
            tp.fixed = false;
            if (tp.cur >= 0 && tp.ver[tp.cur].retire(c) != RRTE_OK) return false;
            tp.cur = -1;
        }
    }
    if (tp.key != key) {  // another shape: drop the list, profile as soon as the copy buffer is free
        tp.key = key;
        tp.slots.clear();
        tp.fixed = c->env.tile_order_fixed;
        if (tp.fixed) tp.slots = fixed_slots(tiles, L.gx);
        if (tp.cur >= 0 && tp.ver[tp.cur].retire(c) != RRTE_OK) return false;
        tp.cur = -1;
        tp.launches = kTileReprofile;
    }
    if (tp.fixed) tp.launches = 0;  // RRTE_TILE_ORDER=2: the fixed list, never profiled
    // a moving camera moves the expensive tiles: re-profile after kTileReprofileMoving launches instead
    const uint64_t cam = fnv1a(&k.cam[0], offsetof(FrameCam, tile_cull));
    const bool moved = cam != tp.cam_sig;
    const uint64_t every = c->env.test_recycle ? 1 : kTileReprofile, moving = c->env.test_recycle ? 1 : kTileReprofileMoving;
    const bool profile = !tp.pending && (tp.launches >= every || (moved && tp.launches >= moving));
    ++tp.launches;
    // RRTE_TEST_RECYCLE=1: a new list version every launch (the fixed list re-uploaded), so the
    // version pool wraps within kVersions launches
    // (into a free version, retiring the current one; with none free the launch keeps the current list)
    if (c->env.test_recycle && tp.fixed && tp.cur >= 0) (void)upload_hot_list(c, tp);
    if (!tp.slots.empty() && tp.slots.size() == tiles && (tp.cur >= 0 || upload_hot_list(c, tp))) {
        // (first launch of this stream on the version: after its upload)
        if (tp.ver[tp.cur].begin_read(c, st, "wait tile-list upload") != hipSuccess) return false;
        k.hot = tp.d_list[tp.cur];
        k.hot_n = (uint32_t)tp.slots.size();
        k.hot_stride = hot_stride(k.hot_n);
    }
    if (!profile) return false;
    if (ensure(c, tp.d_cost, tiles) != RRTE_OK) return false;
    if (tp.h_cost.grow(tiles) != hipSuccess) return false;  // (no copy into it is pending: !tp.pending)
    if (tp.ev.create() != hipSuccess) return false;
    trace_rec(c, "tile profile: reserve lists", st, nullptr, tiles);
    if (!reserve_hot_lists(tp, 8u * (size_t)hot_stride(tiles))) return false;
    trace_rec(c, "tile profile: reserved", st, nullptr, tiles);
    k.tile_cost = tp.d_cost;  // every tile of frame 0 stores its duration (no clearing needed)
    tp.cam_sig = cam;
    tp.pending_key = key;
    tp.tiles = tiles;
    tp.tiles_x = L.gx;
    return true;
}

// Queues the profiled launch's copy-back on its stream (plan_tile_order returned true).
rrte_status finish_tile_order(rrte_ctx* c, const LaunchPlan& L, bool profile, hipStream_t st) {
    auto& tp = c->tprof[L.prof];
    if (!profile) return RRTE_OK;
    HIPCHK(c, hipMemcpyAsync(tp.h_cost, tp.d_cost, (size_t)tp.tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, ev_record(c, tp.ev, st, "record tile-profile copy"));
    tp.pending = true;
    return RRTE_OK;
}

}  // namespace rrte

extern "C" {

rrte_status rrte_hip_tile_order_plan(const uint32_t* costs, uint32_t tiles, uint32_t tiles_x, uint32_t* slots,
                                     uint32_t cap, uint32_t* n_slots) {
    if (!costs || !slots || !n_slots || tiles == 0 || tiles_x == 0 || tiles_x > 0xffffu || tiles / tiles_x > 0xffffu)
        return RRTE_INVALID_ARG;
    const std::vector<uint32_t> v = lpt_slots(costs, tiles, tiles_x);
    *n_slots = (uint32_t)v.size();
    if (v.size() > cap) return RRTE_INVALID_ARG;
    std::copy(v.begin(), v.end(), slots);
    return RRTE_OK;
}

}  // extern "C"
