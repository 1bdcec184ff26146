// context.hpp — the render context (struct rrte_ctx) and what the library's host units share: the
// launch plan, the retire bookkeeping, error and trace helpers, and the functions that cross files
// (rrte_hip.hip opens with the map from function to file).  Private to csrc/: not installed.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <future>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/rrte_hip_accel.h"
#include "../../include/rrte_hip_build.h"
#include "../../include/rrte_hip_jit.h"
#include "../../include/rrte_hip_mesh.h"
#include "../../include/rrte_hip_refit.h"
#include "bvh.hpp"
#include "mesh_build.hpp"
#include "mesh_refit.hpp"
#include "jit.hpp"
#include "ray_kernels.hpp"
#include "accel_kernels.hpp"
#include "resources.hpp"

namespace rrte {

// Everything one launch of the ray kernel needs, decided on the host from the scene and parameters.
// A multi-frame launch (batched gather) is one plan whose KParams carry up to kMaxLaunchFrames
// cameras: blockIdx.y picks the frame (KParams::hot: grid (tile columns, frames, hot rows + tile rows)).
struct LaunchPlan {
    KParams k;
    int mode;
    bool cull, single;
    uint32_t num_prims, num_lights, num_materials;
    uint32_t gx, gy;
    int prof = 0;  // tile-profile slot (rrte_ctx::tprof): 0 whole frames / rank shares, 1 + i chunk i of a blocking frame
};

// A tile order composed off the render thread (plan_tile_order): the profile's shape key and the
// slot list (every tile, slowest first).
struct TilePlanResult {
    std::string key;
    std::vector<uint32_t> slots;
};

// A device resource that launches read asynchronously (a scene version, a tile-list version): the
// streams that launched work reading it since it became current, and -- once it is retired -- one
// event per such stream recorded at retirement, after that stream's last launch that read it.  The
// resource may be overwritten or freed once every event has completed.  No event is recorded per
// launch (an event after every launch put a gap between one stream's launches).
// Streams handed to the async entry points must therefore stay valid until the context has been
// synchronised (include/rrte_hip.h).
struct Retire {
    std::vector<hipStream_t> streams;
    std::vector<Event> events;
    size_t nev = 0;
    void use(hipStream_t st) {
        for (hipStream_t s : streams)
            if (s == st) return;
        streams.push_back(st);
    }
};

// One version of a device resource that launches read asynchronously (a scene version, a tile-list
// version, a counter snapshot): the event of the copy that filled it, the streams already made to
// wait for that event, and the Retire set of the streams that read it.  DESIGN.md §25 states the
// rules; the operations are defined below, after the trace helpers they go through.
struct Version {
    Event ev_up;                       // the version's upload copy done
    std::vector<hipStream_t> ordered;  // streams already made to wait for ev_up
    Retire ret;
    // The copy that fills the version has been queued on `upload`: launches order themselves behind it.
    inline hipError_t published(hipStream_t upload);
    // `st` waits for the upload (once per stream and publication; traced as `tag`).
    inline hipError_t wait_upload(rrte_ctx* c, hipStream_t st, const char* tag);
    // A launch on `st` reads the version: after its upload, and tracked until the version is retired.
    inline hipError_t begin_read(rrte_ctx* c, hipStream_t st, const char* tag);
    inline rrte_status retire(rrte_ctx* c);
    inline bool retired_done() const;
    inline rrte_status wait_retired(rrte_ctx* c);
};

// The environment switches (diagnostics / A-B runs / tests), read once by read_env (context.hip) when
// a context is created and never written afterwards.
struct Env {
    uint32_t debug = 0;       // RRTE_DEBUG ablation bits
    int cull = -1;            // RRTE_CULL: -1 unset, 0 off, 1 on
    bool tile_cull = true;    // RRTE_TILE_CULL=0: no camera-ray tile culling (A/B, tests)
    bool jit_plain = true;    // RRTE_JIT_PLAIN=0: specialised kernels always through the general entry (A/B, tests)
    bool force_gather = false;  // RRTE_FORCE_GATHER=1
    bool gather_rgba = false;   // RRTE_GATHER_RGB24=0: gather slabs always RGBA8
    bool band_sky = true;       // RRTE_BAND_SKY=0: the plain band interleave (band_layout)
    bool gather_self = false;   // RRTE_GATHER_SELF=1 (tests): the root sends its own bands to itself
                                // through RCCL and expands them like a peer's (the 1-GPU check of the
                                // send / recv / expand path)
    uint32_t guard_leaves = 2;  // RRTE_CSG_GUARDS: 0 = off, N = smallest guarded operand (leaves)
    int emu_nranks = 0, emu_rank = 0;  // RRTE_EMULATE_RANK=N:R: render_async renders rank R's bands of N (diagnostic)
    // RRTE_EMULATE_PEERS=N (tests, one GPU): a 1-rank communicator acts as the root of N ranks, and the
    // root renders every peer's packed share (exactly what RRTE_EMULATE_RANK=N:q renders, RGB24 slab
    // included) into peer q's receive slot where ncclRecv would have put it; the real expansion
    // (deinterleave_batch_kernel, skip_rank = root) then composes the frames -- the q >= 1 side of the
    // multi-GPU product path without the link
    int emu_peers = 0;
    bool comm_priority = true;  // RRTE_COMM_PRIORITY=0: comm stream at default priority (A/B)
    int batch_slabs = 3;        // slabs in the ring (RRTE_BATCH_SLABS, A/B: 1..kBatchSlabs; 3 measured
                                // best against 4 and 6, tools/runs/r03_call16.sh)
    // RRTE_FAULT_STALL_GATHER=N (fault injection, tests only): the N-th collective on this context is
    // preceded on its stream by a kernel that spins until the host releases it (or 5 s pass) -- a
    // stalled peer as seen from this rank.
    uint64_t fault_stall_at = 0;
    bool generic_all = false;   // RRTE_GENERIC_ALL=1: the all-features generic kernel for every scene (A/B, tests)
    // Batched gathers render the batch's frames in multi-frame launches at its close (default), or with
    // RRTE_BATCH_LAUNCH=0 each frame at its call (its own launch on the caller's stream: the root in
    // place, a peer into its slot of the send slab) with only the exchange batched -- measured slower
    // for rank shares (a launch of 1/N of a frame lasts as long as its slowest tile, so
    // per-frame launches are tail-bound; 8 frames per launch overlap their tails)
    bool batch_launch = true;
    // Blocking drop-in path into PINNED host memory (hipHostMalloc'd by the caller, or registered with
    // rrte_hip_host_register): the kernel stores the frame straight into the caller's buffer over PCIe
    // while it renders, instead of a render followed by one 8.3 MB D2H copy.  RRTE_BND_ZEROCOPY=0 turns
    // it off (A/B).  Pageable buffers keep the copy.
    bool bnd_zerocopy = true;
    bool zc_system_store = true;  // ... their pixel stores at system scope (RRTE_ZC_SYSTEM_STORE=0: plain, A/B)
    uint32_t zc_tile_shift = 5;   // ... their tile shape (RRTE_ZC_TILE_SHIFT: 3 / 4 / 5 / 6)
    unsigned host_register_flags = hipHostRegisterMapped;  // RRTE_HOST_REGISTER_FLAGS (A/B): rrte_hip_host_register
    // Guard flavour of the scene-specialised kernel (device_scene.hpp RRTE_GUARD_UNIFORM): the correctly
    // rounded sequences' rare fallbacks as wave-uniform branches on a ballot (fewer scalar-unit
    // instructions, a longer dependent chain) or as divergent branches (measured, DESIGN.md §13: frame
    // streams -1.8 %, a lone frame +12 %).  RRTE_GUARD_POLICY: 0 divergent everywhere (default), 1
    // uniform everywhere, 2 uniform for the streaming entry points (async, gather) and divergent for
    // the blocking frame.
    int guard_policy = 0;
    int jit_topo = 2;           // RRTE_JIT_TOPO: 0 full only, 1 topology only, 2 adaptive
    // RRTE_HOST_PROFILE=1 (diagnostics): host time per section of rrte_hip_render_gather_async,
    // printed to stderr by rrte_hip_destroy
    bool host_prof = false;
    uint32_t diag_skip = 0;  // RRTE_DIAG_SKIP (1-rank timing diagnostics only): 1 no ncclGather, 2 no
                             // de-interleave, 4 no comm-stream waits -- results are wrong
    // RRTE_TRACE=1 (diagnostics): every event record / stream wait / launch of the frame paths with its
    // stream and event, host-timestamped, printed to stderr by rrte_hip_destroy (matched against a
    // rocprofv3 kernel trace by launch order)
    bool trace = false;
    // Blocking drop-in path (rrte_hip_render into a host buffer): the frame renders as row chunks on
    // streams of their own, and each chunk's D2H starts as soon as that chunk is done (render_chunked)
    // RRTE_BND_CHUNKS (default 1: one launch, then one copy).  Measured slower so far:
    // every chunk holding object rows is bound by its own slowest tile (~100 us), and the chunks'
    // launches start 7-17 us apart, so the copies cannot start before ~140 us
    int bnd_chunks = 1;
    bool tile_order = true;         // RRTE_TILE_ORDER=0: image order (A/B, tests)
    bool tile_order_fixed = false;  // RRTE_TILE_ORDER=2: a fixed scrambled permutation of the tiles (tests)
    // RRTE_NOCOMM_WAIT_MS: limit of device waits without a communicator (0 = none).  Nothing can stall
    // a frame without one, so the default is far above any frame (10 minutes): a hung or faulted kernel
    // still ends rrte_hip_synchronize / host_unregister / destroy with RRTE_HIP_ERROR
    uint32_t nocomm_wait_ms = 600000;
    // Retire sets / re-profile intervals shortened for tests (RRTE_TEST_RECYCLE=1: a tile-list version
    // per launch, so the version pool wraps within a few frames)
    bool test_recycle = false;
    int fault_bad_slot = 0;  // RRTE_FAULT_BAD_SLOT: 1 a tile-list slot, 2 an object kind (with RRTE_DEBUG bit 2)
    std::string dump_path;   // RRTE_DUMP_SCENE: every render call's scene + params into this file (scene_io.hip)
    // The environment's defaults of switches that have a setter in the C ABI: rrte_ctx copies them into
    // its own members of the same names, which the setters write
    int jit_mode = RRTE_JIT_AUTO;                       // RRTE_JIT (rrte_hip_set_jit)
    uint32_t mesh_build = RRTE_MESH_BUILD_HOST;         // RRTE_MESH_BUILD (rrte_hip_set_mesh_build)
    uint32_t accel_policy = RRTE_SCENE_ACCEL_OFF;       // RRTE_SCENE_ACCEL (rrte_hip_set_scene_accel)
    uint32_t accel_min = RRTE_ACCEL_DEFAULT_MIN_PRIMS;  // RRTE_SCENE_ACCEL_MIN
    uint32_t comm_timeout_ms = 30000;                   // RRTE_COMM_TIMEOUT_MS (rrte_hip_set_comm_timeout)
};

}  // namespace rrte

struct rrte_ctx {
    explicit rrte_ctx(const rrte::Env& e)
        : env(e), comm_timeout_ms(e.comm_timeout_ms), jit_mode(e.jit_mode), mesh_build(e.mesh_build),
          accel_policy(e.accel_policy), accel_min(e.accel_min) {}
    const rrte::Env env;  // what a render call can never change; everything below is state
    int device = 0;
    rrte::Stream stream;
    rrte::Event ev0, ev1, ev2;  // (with timing: rrte_stats.kernel_ms, gather_ms)
    std::string err;
    // scene cache (device copy + the host bytes it was made from).  The device copy is versioned: a
    // ring of kSceneVersions buffer sets, so a scene change uploads into a version no frame in flight
    // reads (Retire) instead of draining the device; d_prims ... mesh_view alias the current version.
    std::vector<unsigned char> scene_key;
    // One scene version = ONE device allocation holding every array (objects, materials, lights, SDF
    // nodes, culling spheres, mesh BVH / triangles / normals / permutation at 256-B aligned offsets),
    // filled by ONE copy from a pinned staging buffer on the upload stream; a launch's stream waits
    // for that copy's event (once per stream and version), so a scene change never blocks the host
    // on the device.
    struct SceneBuf {
        rrte::DeviceBuf<uint8_t> d_buf;
        rrte::PinnedBuf<uint8_t> h_stage;
        rrte::Version ver;  // upload event, ordered streams, readers
    };
    static constexpr int kSceneVersions = 4;
    SceneBuf sb[kSceneVersions];
    int sb_cur = -1;
    rrte::Stream upload_stream;  // scene and tile-list H2D copies (never queued behind frames or gathers)
    rrte::DPrim* d_prims = nullptr;
    rrte::DMaterial* d_mats = nullptr;
    rrte::DLight* d_lights = nullptr;
    rrte_sdf_node* d_nodes = nullptr;
    float4* d_bounds = nullptr;
    rrte::MeshView mesh_view{};
    // device buffers replaced by larger ones while launches in flight may still read them: freed at
    // the next point where the context is idle (rrte_hip_synchronize, rrte_hip_destroy) instead of by an
    // inline free that could wait on the device
    std::vector<rrte::DeviceMem> graveyard;
    rrte::PinnedBuf<uint8_t> h_warm;  // the upload stream's warm-up copy (rrte_hip_create)
    rrte::DeviceBuf<uint8_t> d_warm;
    rrte::Retire launched;                 // every stream that launched a frame since the last synchronisation
    uint32_t n_prims = 0, n_mats = 0, n_lights = 0, n_nodes = 0;
    // frame buffers for the blocking entry points
    rrte::DeviceBuf<uint32_t> d_rgba;
    rrte::DeviceBuf<float4> d_f32;
    // staging of the blocking ray queries (rrte_hip_raycast / rrte_hip_pick): rays or pixel pairs in, hits out
    rrte::DeviceBuf<uint8_t> d_qin, d_qout;
    // staging of the blocking frame AOVs (rrte_hip_render_aov): one chunk of every requested plane
    rrte::DeviceBuf<uint8_t> d_aov;
    rrte::DeviceBuf<unsigned long long> d_counters;  // shadow rays, kCounterShards x kCounterStride (accumulating)
    rrte::PinnedBuf<unsigned long long> h_counters;  // pinned copy
    unsigned long long shadow_base = 0;         // value at the start of the last frame
    // The blocking frame returns once the frame itself is complete; its counter copy lands after that
    // and is folded into rrte_stats when they are read (rrte_hip_stats) -- two pinned copy slots, so a
    // frame's copy never overwrites the one of the frame before it while that is unread
    rrte::PinnedBuf<unsigned long long> h_counters2;
    rrte::Event ev_done;              // the blocking frame complete (before its counter copy)
    bool ctr_pending = false;         // the last frame's counts are in slot ctr_slot, not yet in stats
    int ctr_slot = 0;
    // The two snapshot slots as versions (ev_up: the slot's copy landed; ordered: the streams that have
    // waited for the pending copy, issue_launch): a frame launched on another stream than the context's
    // must not add shadow rays to the counters while the blocking frame's snapshot of them is still
    // being copied.  Nothing retires a snapshot: only published and wait_upload are used.
    rrte::Version ctr[2];
    // multi-GPU
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    int comm_size = 0;               // ranks of the RCCL communicator (nranks may be emulated, RRTE_EMULATE_RANK)
    rrte::DeviceBuf<uint32_t> d_full;
    static constexpr int kSlabs = 16;  // per-frame gathers (batch 1) that may be in flight at once
    rrte::Event ev_gath[kSlabs];
    hipStream_t slab_stream[kSlabs] = {};  // stream of the slab's last user, a caller's (nullptr: never used)
    rrte::DeviceBuf<uint32_t> d_slab[kSlabs];
    // the last collective issued (either form): gathers must run in issue order on every rank
    hipStream_t last_gather_stream = nullptr;
    hipEvent_t last_gather_ev = nullptr;
    // Batched gather (rrte_hip_set_gather_batch, B > 1): a frame call only plans its render (camera,
    // tile rectangles); every B frames (or at rrte_hip_flush / synchronize / a scene or parameter
    // change) the batch renders in multi-frame launches (blockIdx.y = frame, up to kMaxLaunchFrames
    // per launch) on the slab's render stream into the send slab, and the comm stream gathers all B
    // frames to the root in ONE ncclGather and de-interleaves them.  Every collective is issued on
    // the one comm stream, in program order; slab k's render stream overlaps slab k-1's gather.
    static constexpr int kMaxBatch = 16, kBatchSlabs = 6;
    uint32_t gather_batch = 1;
    rrte::Stream comm_stream;
    rrte::Stream render_stream[kBatchSlabs];
    struct Batch {
        uint32_t n = 0, cap = 0;             // frames planned into it / frames it was opened for
        uint32_t rendered = 0;               // frames [0, rendered) already launched into the send slab
        bool in_place = false;               // root: its bands rendered straight into the frames (RGBA8)
        bool per_frame = false;              // each frame launched at its call (not at the batch's close)
        uint32_t width = 0, height = 0, band = 0;
        rrte::BandMap bm{};                        // the batch's band partition (a frame with another closes it)
        int root = 0;
        bool rgb24 = false;
        size_t slice = 0;                    // bytes of one frame of one rank (256-B aligned)
        rrte::LaunchPlan plan;                     // frame 0's plan; frame j's camera in cam[j % kMaxLaunchFrames]
        rrte::FrameCam cam[kMaxBatch];
        uint32_t* full[kMaxBatch] = {};      // root: each frame's caller buffer
        uint32_t nsrc = 0;                   // distinct caller streams of the batch's frames
        hipStream_t src[kMaxBatch] = {};
        rrte::Event ev_src[kMaxBatch];       // recorded on src[i] at the flush
    } batch;
    int bslot = 0;
    rrte::Event ev_batch[kBatchSlabs];   // the slab's last batch gathered and de-interleaved
    rrte::Event ev_render[kBatchSlabs];  // the slab's last batch rendered
    rrte::DeviceBuf<uint8_t> d_bsend[kBatchSlabs], d_brecv[kBatchSlabs];
    uint64_t gather_frames = 0;
    // Collective failure detection: every wait for a gather is bounded by comm_timeout_ms
    // and polls ncclCommGetAsyncError; a gather that fails or does not complete aborts the communicator
    // (ncclCommAbort) and every later gather call returns RRTE_RCCL_ERROR until rrte_hip_comm_init.
    uint32_t comm_timeout_ms;  // (Env::comm_timeout_ms, rrte_hip_set_comm_timeout)
    bool comm_failed = false;
    std::string comm_fail_msg;
    uint64_t gathers_issued = 0;       // collectives issued on this communicator (both forms)
    rrte::Event ev_poll[3 + kBatchSlabs];  // bounded waits: the context's streams + the last gather
    // the injected stall (Env::fault_stall_at), one per context
    rrte::PinnedBuf<uint32_t> h_stall;  // mapped and coherent: the device-visible release flag
    bool stall_armed = false, stall_fired = false;
    // Blocking drop-in path (rrte_hip_render into a host buffer, Raytracer::render's signature): render,
    // then one pageable hipMemcpy (the runtime's path runs at PCIe rate, ~53 GB/s, tools/micro/d2h.hip).
    // Measured and rejected: a band copy kernel beside the render, and touching the
    // caller's fresh pages from host threads while the render runs.
    rrte_stats stats{};
    bool pending_kernel_timing = false;
    uint64_t pending_primary = 0;
    // scene-specialised kernels (jit.hip)
    int jit_mode;  // (Env::jit_mode, rrte_hip_set_jit)
    uint32_t last_entry = 0;      // the last ray launch's kernel (rrte_hip_jit_entry): RRTE_ENTRY_*
    bool host_out = false;        // the launch being issued writes a pinned host frame (render_common's zero-copy path)
    uint64_t scene_gen = 0;       // bumped whenever the cached scene changes
    uint32_t scene_feat = rrte::kFeatAll;  // the cached scene's features (kFeat*): its generic kernel variant
    // The last built mesh data (one entry), kept on the host so that a scene change that leaves the mesh
    // arrays and the set of ranges alone re-uploads it without a BVH build (upload_scene)
    rrte::MeshData mesh_cache;
    std::vector<unsigned char> mesh_cache_key;  // MeshKey, then the arrays' content when mesh_version is 0
    bool mesh_cache_valid = false;
    uint64_t bvh_builds = 0;  // distinct ranges built since the context was created (rrte_hip_mesh_info)
    // Deforming meshes (include/rrte_hip_refit.h).  mesh_cache_indices: the indices the
    // cache was built from (rrte_hip_mesh_refit compares the caller's against them).  While
    // mesh_deformed is set the cache's key names arrays whose vertices differ from the ones mesh_cache's
    // records were built from: every scene version made from it is refitted on the device from the
    // scene's vertices (upload_scene) and mesh_cache itself is never uploaded unrefitted; only its
    // ranges' lo / hi (the culling spheres) follow the vertices on the host.  A real build clears it.
    std::vector<uint32_t> mesh_cache_indices;
    bool mesh_deformed = false;
    rrte::RefitStatic refit_static;         // of mesh_cache's topology (first refit after a build)
    bool refit_static_valid = false;
    uint64_t refits = 0, device_refits = 0;
    // The mesh build policy (include/rrte_hip_build.h): who builds on a mesh-cache miss.
    // The device builder's scratch is grown with ensure(), used on the upload stream only and waited
    // for before build_meshes_device returns.
    uint32_t mesh_build;  // (Env::mesh_build, rrte_hip_set_mesh_build)
    uint64_t device_builds = 0, host_fallbacks = 0;
    uint32_t build_depth = 0;
    rrte::DeviceBuilder builder;
    rrte::DeviceBuf<uint8_t> d_build;
    rrte::BuildTimes build_times;  // (RRTE_HOST_PROFILE)
    // The scene accelerator (include/rrte_hip_accel.h): a tree over the objects' culling
    // spheres, built by upload_scene into the scene version it belongs to (accel: that version's
    // device pointers, like d_prims).  accel_on: the cached version has one; its frames and queries
    // run the accelerated generic kernels (accel_kernels.hpp).
    uint32_t accel_policy, accel_min;  // (Env::accel_policy, accel_min; rrte_hip_set_scene_accel)
    uint32_t accel_flags = 0;
    uint64_t accel_builds = 0, accel_fallbacks = 0;
    bool accel_on = false;
    rrte::AccelView accel{};
    uint32_t accel_nodes = 0, accel_depth = 0, accel_bounded = 0, accel_unbounded = 0;
    // a change of policy or min_prims: the next frame or query uploads the cached scene again (upload_scene)
    bool accel_dirty = false;
    rrte::Event ev_accel;  // recorded behind the last counted launch (RRTE_ACCEL_COUNT), created on first use
    bool accel_counted = false;
    uint32_t tile_shift = 3;          // tile shape of the launch being planned (KParams::tile_shift)
    struct HostReg { void* p; size_t bytes; };
    std::vector<HostReg> host_regs;   // rrte_hip_host_register'ed ranges (unregistered at destroy)
    struct { uint64_t gen; int mode, jit_mode; bool cull, single, topo, uniform, valid; rrte::JitKernel* k; } jit_last{};
    bool jit_stream = true;         // the current call streams frames (false inside rrte_hip_render)
    uint64_t same_scene_renders = 0;             // consecutive renders of the cached scene
    // topology kernels (jit.hip JitTopo): the cached scene's topology key and structural decisions, and
    // how many consecutive scene changes kept that topology (value edits: an animation)
    std::string topo_key;
    rrte::JitTopo topo;
    uint64_t value_edits = 0;
    std::vector<rrte::DPrim> h_prims;                  // host copy of the lowered scene (JIT source)
    std::vector<float4> h_bounds;                // host copy of the per-object culling spheres
    std::vector<rrte::DMaterial> h_mats;
    std::vector<rrte::DLight> h_lights;
    std::vector<rrte_sdf_node> h_nodes;
    std::unordered_map<std::string, rrte::JitKernel> jit_cache;  // failed compiles cached with fn == nullptr
    std::unordered_map<std::string, std::future<rrte::JitCode>> jit_pending;  // AUTO: background compiles
    std::string jit_log;
    // RRTE_HOST_PROFILE sections (Env::host_prof), printed to stderr by rrte_hip_destroy
    double hp[16] = {};  // [0, 9): gather frames; [10, 15): asynchronous frames (rrte_hip_render_async)
    uint64_t hpa_frames = 0;
    double hpu[9] = {};     // scene uploads (upload_scene), RRTE_HOST_PROFILE sections (names at rrte_hip_destroy)
    uint64_t hpu_n = 0;
    bool hpa_cur = false;  // inside rrte_hip_render_async (its sections go to hp[10..15))
    uint64_t hp_frames = 0;
    // RRTE_TRACE records (Env::trace), printed to stderr by rrte_hip_destroy
    struct TraceRec { double us; const char* what; const void* st; const void* ev; uint32_t a, b; };
    std::vector<TraceRec> trace_log;
    std::chrono::steady_clock::time_point trace_t0 = std::chrono::steady_clock::now();
    // Tile order (KParams::hot).  Every kTileReprofile-th launch of one launch shape (size, rows, band
    // mapping, mode, kernel) times each tile of its frame 0 on the device and copies the durations back
    // asynchronously; once they have arrived, later launches of that shape dispatch every tile slowest
    // first (longest-processing-time order; RRTE_TILE_ORDER=1: only the 1024 slowest first, then image
    // order).  The order never changes a pixel, only when each tile starts.  RRTE_TILE_ORDER=0 turns it
    // off (A/B, tests).
    struct TileProfile {
        std::string key;                 // launch shape the tile list belongs to
        std::string pending_key;         // shape of the profile in flight
        bool pending = false;
        rrte::Event ev;                  // the profile's D2H copy done
        rrte::DeviceBuf<uint32_t> d_cost;
        rrte::PinnedBuf<uint32_t> h_cost;
        uint32_t tiles = 0, tiles_x = 0;                 // of the pending profile
        bool fixed = false;              // RRTE_TILE_ORDER=2 list
        std::vector<uint32_t> slots;     // packed hot_pack slots in dispatch order (every tile once)
        // device copies of slot lists (KParams::hot): a pool of immutable versions, one per upload.  The
        // current version is retired (Retire) when the next one is uploaded; an upload takes a retired
        // version whose launches have all completed, and when none has, the launch keeps the current
        // list (a stale order renders the same pixels) -- no render call ever waits for one.
        static constexpr int kVersions = 16;
        rrte::DeviceBuf<uint32_t> d_list[kVersions];  // (capacity in words)
        rrte::Version ver[kVersions];                 // upload event, ordered streams, readers
        // pinned staging, one slice of `arena_words` per version in ONE page-locked allocation (one
        // hipHostMalloc per growth, not one per version): a version's slice is rewritten only when the
        // version is reused, i.e. after every launch that read it -- each of which waited for its copy
        // (ev_up); the arena grows only when no copy out of it is pending
        rrte::PinnedBuf<uint32_t> h_arena;
        size_t arena_words = 0;
        int cur = -1;                    // version holding `slots` (-1: not uploaded)
        uint64_t launches = 0;           // launches of `key` since its last profile
        uint64_t profiles = 0;           // completed profiles
        uint64_t uploads = 0;            // list versions uploaded
        uint64_t cam_sig = 0;            // camera of the last profiled launch (frame 0's FrameCam)
        std::future<rrte::TilePlanResult> work;  // composition of the last profile's order (worker thread)
        bool working = false;
    };
    // One tile-order state per launch shape that alternates within a frame: slot 0 for whole frames
    // and rank shares, slot 1 + i for row chunk i of a blocking frame (render_chunked)
    // tile-profile slots: 0 frames into device buffers and the copy path, 1..kBndChunksMax the row
    // chunks of render_chunked, kZcProf zero-copy frames (their 32x2 tiles are another launch shape:
    // an engine alternating copy-path and zero-copy frames must not re-profile every frame)
    static constexpr int kBndChunksMax = 8, kZcProf = 1 + kBndChunksMax, kProfSlots = 2 + kBndChunksMax;
    TileProfile tprof[kProfSlots];
    // the row chunks of a blocking frame (render_chunked, Env::bnd_chunks): a stream and an event each,
    // and the stream of their copies
    rrte::Stream bnd_stream[kBndChunksMax];
    rrte::Stream bnd_copy;
    rrte::Event ev_bchunk[kBndChunksMax];
    rrte::Event ev_bcopy;
    // band partition of the last multi-GPU frame (frame_band_map)
    struct {
        bool valid = false;
        uint64_t gen = 0;
        uint32_t w = 0, h = 0, band = 0;
        int nranks = 0, root = 0, rank = 0;
        rrte_camera cam{};
        rrte::BandMap m{};
        uint32_t rows = 0, cap = 0;  // this rank's rows; the most rows any rank owns (slab rows)
    } band_cache;
    // camera-ray tile rectangles of the last camera (fill_tile_rects)
    struct {
        bool valid = false;
        uint64_t gen = 0;
        uint32_t width = 0, height = 0, band = 0;
        rrte_camera cam{};
        uint32_t tile_cull = 0, tile_n = 0;
        uint32_t rect[32] = {};
    } tile_rect_cache;
};

namespace rrte {

// Host-section timer for RRTE_HOST_PROFILE (no clock reads when it is off).
struct HostSection {
    rrte_ctx* c;
    std::chrono::steady_clock::time_point t;
    explicit HostSection(rrte_ctx* ctx) : c(ctx) {
        if (c->env.host_prof) t = std::chrono::steady_clock::now();
    }
    void lap(int k) {
        if (!c->env.host_prof) return;
        const auto n = std::chrono::steady_clock::now();
        c->hp[k] += std::chrono::duration<double, std::micro>(n - t).count();
        t = n;
    }
};

constexpr size_t kCounterBytes = sizeof(unsigned long long) * kCounterShards * kCounterStride;

inline rrte_status fail(rrte_ctx* c, rrte_status st, const char* fmt, ...) {
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return st;
}

#define HIPCHK(ctx, expr)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail((ctx), RRTE_HIP_ERROR, "%s failed: %s", #expr, hipGetErrorString(e_));     \
    } while (0)

// (the communicator is non-blocking: ncclInProgress is settled by polling, nccl_settle)
#define NCCLCHK(ctx, expr)                                                                         \
    do {                                                                                           \
        ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess) {                                                                   \
            rrte_status s_ = nccl_settle((ctx), r_, #expr);                                        \
            if (s_ != RRTE_OK) return s_;                                                          \
        }                                                                                          \
    } while (0)

inline void trace_rec(rrte_ctx* c, const char* what, const void* st, const void* ev, uint32_t a = 0, uint32_t b = 0) {
    if (!c->env.trace) return;
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - c->trace_t0).count();
    c->trace_log.push_back({us, what, st, ev, a, b});
}
inline hipError_t ev_record(rrte_ctx* c, hipEvent_t ev, hipStream_t st, const char* tag) {
    trace_rec(c, tag, st, ev);
    return hipEventRecord(ev, st);
}
inline hipError_t ev_wait(rrte_ctx* c, hipStream_t st, hipEvent_t ev, const char* tag) {
    trace_rec(c, tag, st, ev);
    return hipStreamWaitEvent(st, ev, 0);
}

// Device buffer of at least n elements; a smaller one goes to the graveyard (launches in flight may
// still read it; freed when the context is next idle).
template <typename T>
rrte_status ensure(rrte_ctx* c, DeviceBuf<T>& buf, size_t n) {
    if (n <= buf.cap() && buf) return RRTE_OK;
    if (buf) c->graveyard.push_back(std::move(buf));
    HIPCHK(c, buf.alloc(n < 1 ? 1 : n));
    return RRTE_OK;
}

// ---- functions that cross files ----

// context.hip
rrte_status retire(rrte_ctx* c, Retire& r);
bool retired_done(const Retire& r);
rrte_status wait_retired(rrte_ctx* c, Retire& r);
Env read_env();
uint32_t env_guard_setting();
int env_cull_setting();

// scene_upload.hip
void mat4_srt(const float trs[10], float m[16]);
void to_affine12(const float* m16, float* m12);
rrte_status validate_scene(rrte_ctx* c, const rrte_scene_ir* s);
rrte_status validate(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p);
void lower_scene(const rrte_scene_ir* s, std::vector<DPrim>& prims, std::vector<DMaterial>& mats,
                 std::vector<DLight>& lights, std::vector<float4>* bounds = nullptr);
std::string topology_of(const std::vector<DPrim>& prims, const std::vector<DLight>& lights,
                        std::vector<rrte_sdf_node>& nodes, JitTopo& topo);
rrte_status upload_scene(rrte_ctx* c, const rrte_scene_ir* s, hipStream_t st, double* upload_ms);

// launch_plan.hip
KParams make_params(const rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, uint32_t rows);
uint32_t rows_for_rank(uint32_t height, uint32_t band_rows, int nranks, int rank, uint32_t sky = 0u,
                       uint32_t root_bands = 1u, uint32_t peer_bands = 1u);
bool cull_policy(const rrte_scene_ir* s, uint32_t mode, int env_cull);
uint32_t tile_grid_rows(const KParams& k, uint32_t rows);
LaunchPlan plan_launch(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, uint32_t rows,
                       uint32_t internal_flags, uint32_t row0 = 0u, const BandMap* bm = nullptr);
const BandMap& frame_band_map(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, int root,
                              uint32_t* rows = nullptr, uint32_t* cap = nullptr);

// jit_select.hip
JitKernel* jit_kernel_for(rrte_ctx* c, int mode, bool cull, bool single);

// tile_order.hip
bool plan_tile_order(rrte_ctx* c, LaunchPlan& L, const void* kern, hipStream_t st);
rrte_status finish_tile_order(rrte_ctx* c, const LaunchPlan& L, bool profile, hipStream_t st);

// rrte_hip.hip
rrte_status issue_launch(rrte_ctx* c, LaunchPlan& L, uint32_t* d_rgba, float4* d_f32, hipStream_t st);
rrte_status launch(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, uint32_t rows,
                   uint32_t* d_rgba, float4* d_f32, hipStream_t st, uint32_t internal_flags = 0u, uint32_t row0 = 0u,
                   int prof = 0, const BandMap* bm = nullptr);
hipError_t load_ray_kernels();
rrte_status resolve_counters(rrte_ctx* c);
rrte_status finish_frame(rrte_ctx* c, bool deferred = false);
void dump_if_asked(const rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p);
// Rays (pixels) per launch of the blocking queries and AOVs: bounds the context's staging buffers
// however large the call is.
constexpr uint32_t kQueryChunk = 1u << 22;
rrte_status accel_launch_view(rrte_ctx* c, hipStream_t st, AccelView& av, bool fresh = true);
rrte_status accel_launch_done(rrte_ctx* c, hipStream_t st);
rrte_status query_scene(rrte_ctx* c, const rrte_scene_ir* s, hipStream_t st);

// gather.hip
rrte_status render_batch(rrte_ctx* c, bool at_flush);
rrte_status nccl_settle(rrte_ctx* c, ncclResult_t r, const char* what);
rrte_status poll_events(rrte_ctx* c, const Event* ev, size_t n);
rrte_status wait_bounded(rrte_ctx* c);
hipError_t load_gather_kernels();

// ---- struct Version ----

inline hipError_t Version::published(hipStream_t upload) {
    const hipError_t e = hipEventRecord(ev_up, upload);
    ordered.clear();
    return e;
}
inline hipError_t Version::wait_upload(rrte_ctx* c, hipStream_t st, const char* tag) {
    if (std::find(ordered.begin(), ordered.end(), st) != ordered.end()) return hipSuccess;
    const hipError_t e = ev_wait(c, st, ev_up, tag);
    if (e == hipSuccess) ordered.push_back(st);
    return e;
}
inline hipError_t Version::begin_read(rrte_ctx* c, hipStream_t st, const char* tag) {
    const hipError_t e = wait_upload(c, st, tag);
    if (e == hipSuccess) ret.use(st);
    return e;
}
inline rrte_status Version::retire(rrte_ctx* c) { return rrte::retire(c, ret); }
inline bool Version::retired_done() const { return rrte::retired_done(ret); }
inline rrte_status Version::wait_retired(rrte_ctx* c) { return rrte::wait_retired(c, ret); }

}  // namespace rrte
