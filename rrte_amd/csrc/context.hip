// context.hip — the life of a render context (rrte_ctx, context.hpp): creation with its environment
// switches, destruction, synchronisation, the retire bookkeeping, and the small setters and info
// getters of the C ABI.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>

#include "context.hpp"

using namespace rrte;

namespace rrte {

// Retire a resource (struct Retire): an event on every stream that read it since it became current.
// Events of an earlier retirement that have not completed yet are kept.
rrte_status retire(rrte_ctx* c, Retire& r) {
    size_t keep = 0;
    for (size_t i = 0; i < r.nev; ++i)
        if (hipEventQuery(r.events[i]) != hipSuccess) std::swap(r.events[keep++], r.events[i]);
    r.nev = keep;
    for (hipStream_t s : r.streams) {
        if (r.events.size() <= r.nev) {
            Event e;
            HIPCHK(c, e.create());
            r.events.push_back(std::move(e));
        }
        HIPCHK(c, hipEventRecord(r.events[r.nev], s));
        ++r.nev;
    }
    r.streams.clear();
    return RRTE_OK;
}

// True when every launch that read a retired resource has completed (no wait).
bool retired_done(const Retire& r) {
    for (size_t i = 0; i < r.nev; ++i)
        if (hipEventQuery(r.events[i]) != hipSuccess) return false;
    return true;
}

// Bounded wait for a retired resource (poll_events: RRTE_RCCL_ERROR if a gather it sits behind stalls).
rrte_status wait_retired(rrte_ctx* c, Retire& r) {
    if (retired_done(r)) {
        r.nev = 0;
        return RRTE_OK;
    }
    rrte_status st = poll_events(c, r.events.data(), r.nev);
    if (st == RRTE_OK) r.nev = 0;
    return st;
}

// RRTE_CSG_GUARDS: unset = 2 (guard operands of >= 2 leaves), 0 = off, N = smallest guarded operand
uint32_t env_guard_setting() {
    const char* g = getenv("RRTE_CSG_GUARDS");
    return g ? (uint32_t)strtoul(g, nullptr, 0) : 2u;
}

int env_cull_setting() {
    const char* ce = getenv("RRTE_CULL");
    return ce ? (ce[0] != '0' ? 1 : 0) : -1;
}

// The environment switches of a new context (struct Env): every getenv of context creation.
Env read_env() {
    Env e;
    if (const char* j = getenv("RRTE_JIT")) e.jit_mode = (int)strtol(j, nullptr, 0);
    if (const char* d = getenv("RRTE_DEBUG")) e.debug = (uint32_t)strtoul(d, nullptr, 0);
    e.cull = env_cull_setting();
    if (const char* t = getenv("RRTE_TILE_CULL")) e.tile_cull = t[0] != '0';
    if (const char* t = getenv("RRTE_JIT_PLAIN")) e.jit_plain = t[0] != '0';
    if (const char* g = getenv("RRTE_FORCE_GATHER")) e.force_gather = g[0] == '1';
    if (const char* g = getenv("RRTE_HOST_PROFILE")) e.host_prof = g[0] == '1';
    if (const char* g = getenv("RRTE_MESH_BUILD")) {
        if (!strcmp(g, "device")) e.mesh_build = RRTE_MESH_BUILD_DEVICE;
        else if (!strcmp(g, "host")) e.mesh_build = RRTE_MESH_BUILD_HOST;
    }
    if (const char* g = getenv("RRTE_SCENE_ACCEL")) {
        if (!strcmp(g, "on")) e.accel_policy = RRTE_SCENE_ACCEL_ON;
        else if (!strcmp(g, "off")) e.accel_policy = RRTE_SCENE_ACCEL_OFF;
    }
    if (const char* g = getenv("RRTE_SCENE_ACCEL_MIN"); g && *g)
        if (const uint32_t m = (uint32_t)strtoul(g, nullptr, 0)) e.accel_min = m;
    if (const char* g = getenv("RRTE_TRACE")) e.trace = g[0] == '1';
    if (const char* g = getenv("RRTE_DIAG_SKIP")) e.diag_skip = (uint32_t)strtoul(g, nullptr, 0);
    if (const char* g = getenv("RRTE_GATHER_RGB24")) e.gather_rgba = g[0] == '0';
    e.guard_leaves = env_guard_setting();
    if (const char* g = getenv("RRTE_COMM_TIMEOUT_MS")) e.comm_timeout_ms = std::max<uint32_t>(1u, (uint32_t)strtoul(g, nullptr, 0));
    if (const char* g = getenv("RRTE_FAULT_STALL_GATHER")) e.fault_stall_at = strtoull(g, nullptr, 0);
    if (const char* g = getenv("RRTE_BATCH_SLABS"); g && *g)
        e.batch_slabs = std::max(1, std::min(rrte_ctx::kBatchSlabs, (int)strtol(g, nullptr, 0)));
    if (const char* g = getenv("RRTE_GATHER_SELF")) e.gather_self = g[0] == '1';
    if (const char* g = getenv("RRTE_BAND_SKY")) e.band_sky = g[0] != '0';
    if (const char* g = getenv("RRTE_COMM_PRIORITY")) e.comm_priority = g[0] != '0';
    if (const char* g = getenv("RRTE_GENERIC_ALL")) e.generic_all = g[0] == '1';
    if (const char* g = getenv("RRTE_GUARD_POLICY"); g && *g) e.guard_policy = std::min(2, std::max(0, atoi(g)));
    if (const char* g = getenv("RRTE_BATCH_LAUNCH")) e.batch_launch = g[0] != '0';
    if (const char* g = getenv("RRTE_BND_ZEROCOPY")) e.bnd_zerocopy = g[0] != '0';
    if (const char* g = getenv("RRTE_ZC_TILE_SHIFT"))
        e.zc_tile_shift = std::max(3u, std::min(6u, (uint32_t)strtoul(g, nullptr, 0)));
    if (const char* g = getenv("RRTE_ZC_SYSTEM_STORE")) e.zc_system_store = g[0] != '0';
    if (const char* g = getenv("RRTE_NOCOMM_WAIT_MS")) e.nocomm_wait_ms = (uint32_t)strtoul(g, nullptr, 0);
    if (const char* g = getenv("RRTE_TILE_ORDER")) {
        e.tile_order = g[0] != '0';
        e.tile_order_fixed = g[0] == '2';  // 0 image order, 2 fixed permutation (tests), else measured (default)
    }
    if (const char* g = getenv("RRTE_TEST_RECYCLE")) e.test_recycle = g[0] == '1';
    if (const char* g = getenv("RRTE_FAULT_BAD_SLOT")) e.fault_bad_slot = (g[0] == '1' || g[0] == '2') ? g[0] - '0' : 0;
    if (const char* g = getenv("RRTE_DUMP_SCENE"); g && *g) e.dump_path = g;
    if (const char* g = getenv("RRTE_BND_CHUNKS"); g && *g)
        e.bnd_chunks = std::max(1, std::min(rrte_ctx::kBndChunksMax, (int)strtol(g, nullptr, 0)));
    if (const char* t = getenv("RRTE_JIT_TOPO"); t && *t) e.jit_topo = (int)strtol(t, nullptr, 0);
    if (const char* g = getenv("RRTE_EMULATE_PEERS")) {
        const int n = (int)strtol(g, nullptr, 0);
        if (n > 1) e.emu_peers = n;
    }
    if (const char* g = getenv("RRTE_EMULATE_RANK")) {
        int n = 0, r = 0;
        if (sscanf(g, "%d:%d", &n, &r) == 2 && n > 1 && r >= 0 && r < n) {
            e.emu_nranks = n;
            e.emu_rank = r;
        }
    }
    if (const char* g = getenv("RRTE_HOST_REGISTER_FLAGS")) e.host_register_flags = (unsigned)strtoul(g, nullptr, 0);  // (A/B)
    return e;
}

}  // namespace rrte

extern "C" {

uint32_t rrte_hip_abi_version(void) { return RRTE_ABI_VERSION; }

rrte_status rrte_hip_create(int device, rrte_ctx** out) {
    if (!out) return RRTE_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return RRTE_NO_DEVICE;
    if (device < 0 || device >= n) return RRTE_NO_DEVICE;
    rrte_ctx* c = new (std::nothrow) rrte_ctx(read_env());
    if (!c) return RRTE_HIP_ERROR;
    c->device = device;
    auto bail = [&](hipError_t e) {
        (void)e;
        rrte_hip_destroy(c);
        return RRTE_HIP_ERROR;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return bail(e);
    if ((e = c->stream.create()) != hipSuccess) return bail(e);
    if ((e = c->ev0.create(true)) != hipSuccess) return bail(e);
    if ((e = c->ev1.create(true)) != hipSuccess) return bail(e);
    if ((e = c->ev2.create(true)) != hipSuccess) return bail(e);
    if ((e = c->d_counters.alloc(kCounterShards * kCounterStride)) != hipSuccess) return bail(e);
    // (on the context's stream: its first operation sets up its hardware queue, here and not in a frame)
    if ((e = hipMemsetAsync(c->d_counters, 0, kCounterBytes, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return bail(e);
    if ((e = c->h_counters.alloc(kCounterShards * kCounterStride)) != hipSuccess) return bail(e);
    memset(c->h_counters, 0, kCounterBytes);
    if ((e = c->h_counters2.alloc(kCounterShards * kCounterStride)) != hipSuccess) return bail(e);
    memset(c->h_counters2, 0, kCounterBytes);
    for (Version& v : c->ctr)
        if ((e = v.ev_up.create()) != hipSuccess) return bail(e);
    if ((e = c->ev_done.create()) != hipSuccess) return bail(e);
    // the upload stream, and a first copy of a tile list's size class through it: the runtime sets up
    // what such a copy needs at its first use (7-8 ms measured, inside the first frame of a new launch
    // shape: profiles/r06_engine_loop_trace.log) -- here rather than in a frame
    if ((e = c->upload_stream.create()) != hipSuccess) return bail(e);
    {
        // the library's code objects of the frame paths (every generic kernel; the gather's expansion):
        // the runtime loads one at the first use of a kernel in it -- ~20 ms inside the first frame
        // otherwise (profiles/r06_engine_loop_trace_after.log).  One code object per unit: each is
        // asked for by the unit that holds it
        if ((e = load_ray_kernels()) != hipSuccess || (e = load_gather_kernels()) != hipSuccess) return bail(e);
    }
    {
        constexpr size_t kWarm = 129600;  // a 1080p frame's list (32400 slots)
        // (the buffers are freed with the context: a free here could wait for other contexts' frames)
        if ((e = c->h_warm.alloc(kWarm)) != hipSuccess) return bail(e);
        memset(c->h_warm, 0, kWarm);
        // (and the way back on the context's stream: a frame's tile-profile copy is a D2H of that size)
        if ((e = c->d_warm.alloc(kWarm)) != hipSuccess ||
            (e = hipMemcpyAsync(c->d_warm, c->h_warm, kWarm, hipMemcpyHostToDevice, c->upload_stream)) != hipSuccess ||
            (e = hipStreamSynchronize(c->upload_stream)) != hipSuccess ||
            (e = hipMemcpyAsync(c->h_warm, c->d_warm, kWarm, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(c->stream)) != hipSuccess)
            return bail(e);
    }
    if (c->env.fault_stall_at) {
        if ((e = c->h_stall.alloc(16, hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess)
            return bail(e);
        *c->h_stall.get() = 1u;
    }
    *out = c;
    return RRTE_OK;
}

void rrte_hip_destroy(rrte_ctx* c) {
    if (!c) return;
    if (c->env.host_prof && c->hp_frames) {
        static const char* names[9] = {"validate", "upload_check", "slab_setup", "render_launch", "event_chain",
                                       "ncclGather", "deinterleave", "event_record", "(of render_launch: the launch call)"};
        fprintf(stderr, "rrte host profile (%llu gather frames, us/frame):", (unsigned long long)c->hp_frames);
        for (int i = 0; i < 9; ++i) fprintf(stderr, " %s %.2f", names[i], c->hp[i] / (double)c->hp_frames);
        fprintf(stderr, "\n");
    }
    if (c->env.host_prof && c->hpa_frames) {
        static const char* names[5] = {"validate", "scene_check", "plan", "tile_order+jit", "launch_call"};
        fprintf(stderr, "rrte host profile (%llu async frames, us/frame):", (unsigned long long)c->hpa_frames);
        for (int i = 0; i < 5; ++i) fprintf(stderr, " %s %.2f", names[i], c->hp[10 + i] / (double)c->hpa_frames);
        fprintf(stderr, "\n");
    }
    if (c->env.host_prof && c->hpu_n) {
        static const char* names[9] = {"lower", "mesh_bvh", "csg_guards", "topology", "version_wait", "staging",
                                       "copy_call", "event_record", "bookkeeping"};
        fprintf(stderr, "rrte host profile (%llu scene uploads, us/upload):", (unsigned long long)c->hpu_n);
        for (int i = 0; i < 9; ++i) fprintf(stderr, " %s %.2f", names[i], c->hpu[i] / (double)c->hpu_n);
        fprintf(stderr, "\n");
    }
    if (c->env.host_prof && c->build_times.n) {
        const BuildTimes& bt = c->build_times;
        const double n = (double)bt.n;
        fprintf(stderr, "rrte host profile (%llu device mesh builds, us/build): host_scan %.2f enqueue %.2f depth_wait %.2f "
                        "boxes_enqueue %.2f readback %.2f\n",
                (unsigned long long)bt.n, bt.host_scan / n, bt.enqueue / n, bt.depth_wait / n, bt.boxes_enqueue / n, bt.readback / n);
    }
    if (c->env.trace) {
        for (const auto& t : c->trace_log)
            fprintf(stderr, "rrte trace %12.1f us  %-34s stream %p event %p  %u %u\n", t.us, t.what, t.st, t.ev, t.a, t.b);
    }
    (void)hipSetDevice(c->device);
    if (c->h_stall) __hip_atomic_store(c->h_stall.get(), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // injected stall
    // gathers first, bounded (a dead peer aborts the communicator instead of hanging here); then the
    // frames that may still run on caller streams
    if (c->comm && wait_bounded(c) != RRTE_OK) c->comm = nullptr;  // (comm_abort has aborted it)
    (void)hipDeviceSynchronize();
    if (c->comm) ncclCommDestroy(c->comm);
    for (const auto& hr : c->host_regs) (void)hipHostUnregister(hr.p);
    c->jit_pending.clear();  // joins background compiles
    for (auto& tp : c->tprof)
        if (tp.working) tp.work.wait();  // the tile-order workers
    for (auto& kv : c->jit_cache) jit_release(kv.second);
    delete c;  // every buffer, event and stream: the members' destructors (resources.hpp)
}

const char* rrte_hip_last_error(const rrte_ctx* c) { return c ? c->err.c_str() : "null context"; }

rrte_status rrte_hip_synchronize(rrte_ctx* c) {
    if (!c) return RRTE_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    // local: an open gather batch is rendered but stays open (its gather is collective: rrte_hip_flush)
    rrte_status r = render_batch(c, false);
    if (r != RRTE_OK) return r;
    if ((r = wait_bounded(c)) != RRTE_OK) return r;
    // every stream that launched a frame (bounded: a frame may sit behind a gather), then the device
    if ((r = retire(c, c->launched)) != RRTE_OK || (r = wait_retired(c, c->launched)) != RRTE_OK) return r;
    HIPCHK(c, hipDeviceSynchronize());
    // idle: buffers replaced while frames were in flight can go, and every retired version is free
    c->graveyard.clear();
    return finish_frame(c);
}

rrte_status rrte_hip_check_word(rrte_ctx* c, uint64_t* word) {
    if (!c || !word) return RRTE_INVALID_ARG;
    rrte_status r = rrte_hip_synchronize(c);
    if (r != RRTE_OK) return r;
    unsigned long long w = 0;  // counters[1]: an unused word of shard 0 (ray_kernels.hpp launch_indices_ok)
    HIPCHK(c, hipMemcpy(&w, c->d_counters + 1, sizeof w, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemset(c->d_counters + 1, 0, sizeof w));
    *word = w;
    return RRTE_OK;
}

// include/rrte_hip_jit.h
rrte_status rrte_hip_jit_entry(rrte_ctx* c, uint32_t* entry) {
    if (!c || !entry) return RRTE_INVALID_ARG;
    *entry = c->last_entry;
    return RRTE_OK;
}

// include/rrte_hip_mesh.h
rrte_status rrte_hip_mesh_info(rrte_ctx* c, rrte_mesh_info* out) {
    if (!c || !out) return RRTE_INVALID_ARG;
    memset(out, 0, sizeof *out);
    out->bvh_builds = c->bvh_builds;
    if (c->sb_cur >= 0 && c->mesh_cache_valid) {  // (the current scene version holds a copy of the cache)
        out->ranges = (uint32_t)c->mesh_cache.ranges.size();
        out->tri_slots = (uint32_t)(c->mesh_cache.tris.size() / 3);
        out->bvh_nodes = (uint32_t)(c->mesh_cache.nodes.size() / 4);
    }
    return RRTE_OK;
}

// include/rrte_hip_build.h
rrte_status rrte_hip_set_mesh_build(rrte_ctx* c, uint32_t policy) {
    if (!c) return RRTE_INVALID_ARG;
    if (policy != RRTE_MESH_BUILD_HOST && policy != RRTE_MESH_BUILD_DEVICE)
        return fail(c, RRTE_INVALID_ARG, "mesh build policy %u (0 host, 1 device)", policy);
    c->mesh_build = policy;
    return RRTE_OK;
}

rrte_status rrte_hip_build_info(rrte_ctx* c, rrte_build_info* out) {
    if (!c || !out) return RRTE_INVALID_ARG;
    out->device_builds = c->device_builds;
    out->host_fallbacks = c->host_fallbacks;
    out->policy = c->mesh_build;
    out->depth = c->build_depth;
    return RRTE_OK;
}

// include/rrte_hip_accel.h
rrte_status rrte_hip_set_scene_accel(rrte_ctx* c, uint32_t policy, uint32_t min_prims, uint32_t flags) {
    if (!c) return RRTE_INVALID_ARG;
    if (policy != RRTE_SCENE_ACCEL_OFF && policy != RRTE_SCENE_ACCEL_ON)
        return fail(c, RRTE_INVALID_ARG, "scene accelerator policy %u (0 off, 1 on)", policy);
    if (flags & ~RRTE_ACCEL_COUNT) return fail(c, RRTE_INVALID_ARG, "unknown scene accelerator flags 0x%x", flags);
    if (min_prims == 0u) min_prims = RRTE_ACCEL_DEFAULT_MIN_PRIMS;
    // whether the cached scene has a tree was decided at its upload: a change of what decides it makes
    // the next frame or query upload the scene again (the mesh cache has its own key: no BVH build).
    // The scene key itself stays: it also names the cached scene's specialised kernels
    if (policy != c->accel_policy || min_prims != c->accel_min) c->accel_dirty = true;
    c->accel_policy = policy;
    c->accel_min = min_prims;
    c->accel_flags = flags;
    if (!(flags & RRTE_ACCEL_COUNT)) c->accel_counted = false;
    return RRTE_OK;
}

rrte_status rrte_hip_accel_info(rrte_ctx* c, rrte_accel_info* out) {
    if (!c || !out) return RRTE_INVALID_ARG;
    memset(out, 0, sizeof *out);
    out->builds = c->accel_builds;
    out->fallbacks = c->accel_fallbacks;
    out->policy = c->accel_policy;
    out->min_prims = c->accel_min;
    out->flags = c->accel_flags;
    if (c->accel_on) {
        out->nodes = c->accel_nodes;
        out->depth = c->accel_depth;
        out->bounded = c->accel_bounded;
        out->unbounded = c->accel_unbounded;
    }
    if ((c->accel_flags & RRTE_ACCEL_COUNT) && c->accel_counted) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipEventSynchronize(c->ev_accel));
        unsigned long long w[2] = {0ull, 0ull};
        HIPCHK(c, hipMemcpy(w, c->d_counters + 2, sizeof w, hipMemcpyDeviceToHost));
        out->searches = w[0];
        out->candidates = w[1];
    }
    return RRTE_OK;
}

rrte_status rrte_hip_refit_info(rrte_ctx* c, rrte_refit_info* out) {
    if (!c || !out) return RRTE_INVALID_ARG;
    memset(out, 0, sizeof *out);
    out->refits = c->refits;
    out->device_refits = c->device_refits;
    out->levels = c->refit_static_valid ? c->refit_static.levels() : 0u;
    out->deformed = (c->mesh_cache_valid && c->mesh_deformed) ? 1u : 0u;
    return RRTE_OK;
}

rrte_status rrte_hip_set_comm_timeout(rrte_ctx* c, uint32_t ms) {
    if (!c) return RRTE_INVALID_ARG;
    if (ms == 0) return fail(c, RRTE_INVALID_ARG, "comm timeout must be > 0 ms");
    c->comm_timeout_ms = ms;
    return RRTE_OK;
}

rrte_status rrte_hip_query(rrte_ctx* c, uint32_t* busy) {
    if (!c || !busy) return RRTE_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t ss[2 + rrte_ctx::kBatchSlabs] = {c->stream, c->comm_stream};
    for (int i = 0; i < rrte_ctx::kBatchSlabs; ++i) ss[2 + i] = c->render_stream[i];
    *busy = 0;
    for (hipStream_t s : ss) {
        if (!s) continue;
        const hipError_t e = hipStreamQuery(s);
        if (e == hipErrorNotReady) {
            *busy = 1;
            return RRTE_OK;
        }
        HIPCHK(c, e);
    }
    return RRTE_OK;
}

rrte_status rrte_hip_set_jit(rrte_ctx* c, int mode) {
    if (!c) return RRTE_INVALID_ARG;
    if (mode < RRTE_JIT_OFF || mode > RRTE_JIT_AUTO) return fail(c, RRTE_INVALID_ARG, "unknown JIT mode %d", mode);
    c->jit_mode = mode;
    return RRTE_OK;
}

rrte_status rrte_hip_stats(rrte_ctx* c, rrte_stats* out) {
    if (!c || !out) return RRTE_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    rrte_status r = resolve_counters(c);
    if (r != RRTE_OK) return r;
    *out = c->stats;
    return RRTE_OK;
}

rrte_status rrte_hip_host_register(rrte_ctx* c, void* host, size_t bytes) {
    if (!c || !host || bytes == 0) return fail(c, RRTE_INVALID_ARG, "null or empty host range");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipHostRegister(host, bytes, c->env.host_register_flags));
    c->host_regs.push_back({host, bytes});
    return RRTE_OK;
}

rrte_status rrte_hip_host_unregister(rrte_ctx* c, void* host) {
    if (!c || !host) return RRTE_INVALID_ARG;
    for (size_t i = 0; i < c->host_regs.size(); ++i)
        if (c->host_regs[i].p == host) {
            HIPCHK(c, hipSetDevice(c->device));
            rrte_status r = rrte_hip_synchronize(c);  // (no frame may still write into it)
            if (r != RRTE_OK) return r;
            HIPCHK(c, hipHostUnregister(host));
            c->host_regs.erase(c->host_regs.begin() + (long)i);
            return RRTE_OK;
        }
    return fail(c, RRTE_INVALID_ARG, "host range %p was not registered with this context", host);
}

}  // extern "C"
