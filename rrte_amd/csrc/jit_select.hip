// jit_select.hip — which scene-specialised kernel a launch runs (issue_launch asks jit_kernel_for):
// the FULL / TOPOLOGY choice, the cache of compiled kernels and the background compiles of the AUTO
// policy, and the context-free exports about the generated code (rrte_hip_jit_check / build_id /
// jit_cache_key).  Host only: no kernel is instantiated here.
#include <chrono>
#include <cstdlib>
#include <future>

#include "context.hpp"
#include "sdf_guard.hpp"

using namespace rrte;

namespace rrte {

// Scene-specialised kernel for the cached scene + mode, compiling it if the
// JIT policy says so; nullptr = use the generic kernel.
constexpr uint32_t kJitMaxPrims = 128, kJitMaxNodes = 1024;

// FULL or TOPOLOGY kernel (RRTE_JIT_TOPO, rrte_hip.h).  Adaptive: topology while the scene's values keep
// changing under one topology (one compile for a whole animation), full once the scene has been
// rendered unchanged for kJitFullAfter frames (until that full kernel is ready, the topology kernel).
constexpr uint64_t kJitFullAfter = 16;

static bool jit_wants_topology(const rrte_ctx* c) {
    return c->env.jit_topo == 1 ||
           (c->env.jit_topo == 2 && c->value_edits >= 1 && c->same_scene_renders < kJitFullAfter);
}

static std::string jit_key(const rrte_ctx* c, bool topo, int mode, bool cull, bool single, bool uniform) {
    std::string key(1, topo ? 'T' : 'F');
    if (topo) key += c->topo_key;
    else key.append(c->scene_key.begin(), c->scene_key.end());
    key.push_back((char)mode);
    key.push_back((char)cull);
    key.push_back((char)single);
    key.push_back((char)uniform);
    return key;
}

static bool jit_uniform_guards(const rrte_ctx* c) { return c->env.guard_policy == 2 ? c->jit_stream : c->env.guard_policy == 1; }

// The cached kernel for `key`, compiling it if the JIT policy says so; nullptr = not available (yet).
static JitKernel* jit_lookup(rrte_ctx* c, const std::string& key, bool topo, int mode, bool cull, bool single, bool uniform) {
    auto it = c->jit_cache.find(key);
    if (it != c->jit_cache.end()) return it->second.fn ? &it->second : nullptr;
    JitKernel jk;
    std::string log;
    auto pend = c->jit_pending.find(key);
    if (pend != c->jit_pending.end()) {
        // AUTO: a background compile of this kernel is running; keep the current kernel until it lands
        if (pend->second.wait_for(std::chrono::seconds(0)) != std::future_status::ready) return nullptr;
        const JitCode jc = pend->second.get();
        c->jit_pending.erase(pend);
        trace_rec(c, "jit: module load begin", nullptr, nullptr, (uint32_t)jc.code.size());
        const bool loaded = hipSetDevice(c->device) == hipSuccess && jit_load(jc, jk, log);
        trace_rec(c, "jit: module load end", nullptr, nullptr, loaded);
        if (!loaded) {
            c->jit_log = log;
            jk = JitKernel{};
        } else {
            c->stats.jit_compile_ms = jk.compile_ms;
        }
    } else {
        if (!(c->jit_mode == RRTE_JIT_ON || c->same_scene_renders >= 1 || topo)) return nullptr;
        if (c->jit_cache.size() >= 32) {
            // frames launched from these modules may still run on caller streams (a mode / cull /
            // sample-count change does not re-upload the scene, so upload_scene's sync has not run)
            // (bounded: RRTE_RCCL_ERROR surfaces at the next gather call if a stalled gather blocks it)
            if (hipSetDevice(c->device) != hipSuccess || retire(c, c->launched) != RRTE_OK ||
                wait_retired(c, c->launched) != RRTE_OK)
                return nullptr;
            for (auto& kv : c->jit_cache) jit_release(kv.second);
            c->jit_cache.clear();
            c->jit_last.valid = false;
        }
        std::string src = jit_source(c->h_prims.data(), (uint32_t)c->h_prims.size(), c->h_mats.data(),
                                     (uint32_t)c->h_mats.size(), c->h_lights.data(), (uint32_t)c->h_lights.size(),
                                     c->h_nodes.data(), (uint32_t)c->h_nodes.size(), mode, cull, single,
                                     topo ? &c->topo : nullptr);
        if (uniform) src = "#define RRTE_GUARD_UNIFORM 1\n" + src;
        if (c->jit_mode == RRTE_JIT_AUTO) {
            // compile on a background thread (hiprtc only); frames keep running on the current kernel
            c->jit_pending.emplace(key, std::async(std::launch::async, [src]() { return jit_compile_code(src); }));
            return nullptr;
        }
        if (hipSetDevice(c->device) != hipSuccess || !jit_compile(src, jk, log)) {
            c->jit_log = log;  // stay on the generic kernel for this scene
            jk = JitKernel{};
        } else {
            c->stats.jit_compile_ms = jk.compile_ms;
        }
    }
    jk.topology = topo;
    auto& slot = c->jit_cache[key];
    slot = jk;
    return slot.fn ? &slot : nullptr;
}

JitKernel* jit_kernel_for(rrte_ctx* c, int mode, bool cull, bool single) {
    if (c->jit_mode == RRTE_JIT_OFF) return nullptr;
    auto& last = c->jit_last;  // per-frame fast path: same scene, mode, policy and kernel kind as the last frame
    const bool topo = jit_wants_topology(c);
    const bool uniform = jit_uniform_guards(c);
    if (last.valid && last.gen == c->scene_gen && last.mode == mode && last.cull == cull && last.single == single &&
        last.jit_mode == c->jit_mode && last.topo == topo && last.uniform == uniform)
        return last.k;
    if (c->h_prims.size() > kJitMaxPrims || c->h_nodes.size() > kJitMaxNodes) return nullptr;
    const std::string key = jit_key(c, topo, mode, cull, single, uniform);
    JitKernel* k = jit_lookup(c, key, topo, mode, cull, single, uniform);
    if (!k && !c->jit_cache.count(key)) {
        // not available yet (AUTO: not due, or compiling in the background): not remembered, asked again
        // next frame.  The full kernel of a scene that stopped changing: its topology kernel meanwhile
        if (!topo && c->env.jit_topo == 2 && c->value_edits >= 1) {
            auto it = c->jit_cache.find(jit_key(c, true, mode, cull, single, uniform));
            if (it != c->jit_cache.end() && it->second.fn) return &it->second;
        }
        return nullptr;
    }
    last.gen = c->scene_gen;
    last.mode = mode;
    last.jit_mode = c->jit_mode;
    last.cull = cull;
    last.single = single;
    last.topo = topo;
    last.uniform = uniform;
    last.k = k;
    last.valid = true;
    return k;
}

}  // namespace rrte

extern "C" {

rrte_status rrte_hip_build_id(char* out, size_t out_len) {
    if (!out || out_len < 33) return RRTE_INVALID_ARG;
    // the device code's identity: the embedded headers, every hiprtc option (RRTE_JIT_EXTRA_OPTS
    // included) and the hiprtc version -- the JIT cache key of an empty source
    snprintf(out, out_len, "%s", jit_cache_name(std::string(), nullptr).c_str());
    return RRTE_OK;
}

rrte_status rrte_hip_jit_cache_key(const char* source, const char* headers_override, char* out, size_t out_len) {
    if (!source || !out || out_len < 33) return RRTE_INVALID_ARG;
    snprintf(out, out_len, "%s", jit_cache_name(source, headers_override).c_str());
    return RRTE_OK;
}

rrte_status rrte_hip_jit_check(const rrte_scene_ir* s, int mode, char* log, size_t log_len) {
    if (!s || (s->num_prims && !s->prims) || (s->num_sdf_nodes && !s->sdf_nodes)) return RRTE_INVALID_ARG;
    std::vector<DPrim> prims;
    std::vector<DMaterial> mats;
    std::vector<DLight> lights;
    if ((s->num_mesh_indices && !s->mesh_indices) || (s->num_mesh_vertices && !s->mesh_vertices)) return RRTE_INVALID_ARG;
    lower_scene(s, prims, mats, lights);
    MeshData md;
    build_mesh_bvhs(s, prims.data(), md, nullptr);
    // RRTE_JIT_CHECK_MULTI=1: the multi-sample / multi-bounce variant (as the renderer picks it for
    // spp > 1 or max_depth > 1) instead of the straight-line one
    const char* mv = getenv("RRTE_JIT_CHECK_MULTI");
    const bool single = !(mv && mv[0] == '1');
    std::vector<rrte_sdf_node> nodes = decorate_scene_sdf(s, env_guard_setting());
    JitTopo topo;
    topology_of(prims, lights, nodes, topo);
    // RRTE_JIT_TOPO=1: the topology kernel instead of the full one
    const char* tv = getenv("RRTE_JIT_TOPO");
    const bool want_topo = tv && tv[0] == '1';
    std::string src = jit_source(prims.data(), (uint32_t)prims.size(), mats.data(), (uint32_t)mats.size(),
                                 lights.data(), (uint32_t)lights.size(), nodes.data(), s->num_sdf_nodes, mode,
                                 cull_policy(s, (uint32_t)mode, env_cull_setting()), single,
                                 want_topo ? &topo : nullptr);
    std::string msg;
    bool ok = jit_compile_only(src, msg);
    if (log && log_len) {
        snprintf(log, log_len, "%s", ok ? "" : msg.c_str());
    }
    return ok ? RRTE_OK : RRTE_HIP_ERROR;
}

}  // extern "C"
