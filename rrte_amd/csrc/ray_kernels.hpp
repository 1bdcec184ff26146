// ray_kernels.hpp — the per-pixel ray->scene loop for gfx950 (CDNA4): the top of the device-header
// stack (DESIGN.md §23 has the map).
//
// One wave64 lane per pixel, one wave per 8x8 pixel tile (rays in a wave are
// spatially coherent, so the wave-uniform object loop and the sphere-tracing
// loop diverge little), one wave per 64-thread workgroup.  Scene records are
// read with wave-uniform indices -> scalar loads into SGPRs; no MFMA (there is
// no dense contraction on this path).  Operation order mirrors the reference
// (file:line cited per function, paths relative to Melthizar/RRTE).
//
// This file holds the launch plumbing (image_row, camera_tile_mask, launch_tile, launch_indices_ok),
// the kernel body (ray_kernel_body) and the generic entry point (ray_kernel).  Includes shade.hpp
// (and through it search.hpp, cull.hpp, intersect.hpp, mesh_walk.hpp, sdf_eval.hpp, scene_view.hpp,
// device_scene.hpp) and pixel_encode.hpp.  Included by context.hpp and accel_kernels.hpp, and by every
// generated scene-specialised source; embedded for hiprtc (the Makefile's DEVICE_HDR).
#pragma once

#include "pixel_encode.hpp"
#include "shade.hpp"

namespace rrte {

// Map this launch's local row to the image row (band interleave, §8e).
template <class LT = LaunchAny>
__device__ __forceinline__ uint32_t image_row(const KParams& kp, uint32_t r) {
    if constexpr (LT::kPlain) return r;
    if (kp.band_rows == 0) return r + kp.row0;
    const uint32_t b = r / kp.band_rows, w = r - b * kp.band_rows;
    const BandMap m{kp.band_rows, kp.nranks, kp.sky_bands, kp.root_bands, kp.peer_bands};
    return band_of_local(m, kp.rank, b) * kp.band_rows + w;
}

// Camera-ray tile culling mask of this wave's 8x8 tile (kp.tile_cull = 3) or the 16x16
// block (4) (KParams::tile_rect): lane j tests object j's rectangle and a ballot makes the mask
// wave-uniform (one load and a handful of VALU ops per wave; a scalar loop over the objects cost ~8
// SALU ops and a scalar load each).  Call with all 64 lanes active.  The host enables it only when
// a tile's local rows are consecutive image rows (no band mapping, or bands of a multiple of the
// tile height).
template <class LT = LaunchAny>
__device__ __forceinline__ uint32_t camera_tile_mask(const KParams& kp, const FrameCam& cm, uint32_t tx,
                                                     uint32_t ty) {
    const uint32_t sh = cm.tile_cull;
    if (!sh) return ~0u;
    // one tile per workgroup: (1 << tile_shift) x (64 >> tile_shift) pixels (its rows lie in one 8-row
    // block of consecutive image rows: 64 >> tile_shift divides 8 and band heights are multiples of 8)
    const uint32_t bx = (tx << kp.tile_shift) >> sh;
    const uint32_t bx1 = ((tx << kp.tile_shift) + (1u << kp.tile_shift) - 1u) >> sh;
    const uint32_t by = image_row<LT>(kp, ty * (64u >> kp.tile_shift)) >> sh;
    const uint32_t j = threadIdx.x & 63u;
    bool in = false;
    if (j < cm.tile_n) {  // the rectangle meets the tile's blocks [bx, bx1] x by
        const uint32_t t = cm.tile_rect[j];
        in = bx1 >= (t & 255u) && bx <= ((t >> 8) & 255u) && by >= ((t >> 16) & 255u) && by <= (t >> 24);
    }
    const uint32_t m = (uint32_t)__ballot(in);
    return m | (cm.tile_n < 32u ? (~0u << cm.tile_n) : 0u);  // objects past the table: never culled
}

// The tile (x, y in workgroup units) and frame of this workgroup: with a tile list (KParams::hot,
// measured-cost order) slot k = blockIdx.z * tiles_x + blockIdx.x renders tile hot[k] (a wave-uniform
// index: one scalar load); run = false for the unused slots of the last slot row.
struct LaunchTile { uint32_t x, y, z; bool run; };
__device__ __forceinline__ LaunchTile launch_tile(const KParams& kp) {
    LaunchTile t{blockIdx.x, blockIdx.z, blockIdx.y, true};
    if (kp.hot) {
        const uint32_t k = blockIdx.z * kp.tiles_x + blockIdx.x;
        t.run = k < kp.hot_n;
        const uint32_t h = kp.hot[t.run ? (k & 7u) * kp.hot_stride + (k >> 3) : 0u];
        t.x = hot_x(h);
        t.y = hot_y(h);
    }
    return t;
}

// RRTE_DEBUG bit 2: the launch's derived indices, checked before any memory access that uses them.
// Check-word bits: 1 list slot out of range, 2 decoded tile outside the launch's tiles, 4 frame index
// >= nframes, 8 an output row outside the frame.
__device__ __forceinline__ bool launch_indices_ok(const KParams& kp, unsigned long long* counters) {
    uint32_t bad = 0u;
    const uint32_t th = 64u >> kp.tile_shift, gy = (kp.rows + th - 1u) / th;
    const uint32_t k = blockIdx.z * kp.tiles_x + blockIdx.x;
    if (blockIdx.y >= kp.nframes || blockIdx.y >= kMaxLaunchFrames) bad |= 4u;
    if (kp.hot) {
        if (k < kp.hot_n) {
            const uint32_t at = (k & 7u) * kp.hot_stride + (k >> 3);
            if (kp.hot_stride * 8u < kp.hot_n || at >= kp.hot_stride * 8u) bad |= 1u;
            else {
                const uint32_t h = kp.hot[at];
                if (hot_x(h) >= kp.tiles_x || hot_y(h) >= gy) bad |= 2u;
            }
        }
    } else if (blockIdx.x >= kp.tiles_x || blockIdx.z >= gy) {
        bad |= 2u;
    }
    if (!bad && kp.rows && kp.band_rows == 0u && kp.row0 + kp.rows > kp.height) bad |= 8u;
    if (bad && (threadIdx.x & 63u) == 0u) atomicOr(counters + 1, (unsigned long long)bad);
    return bad == 0u;
}

// One lane per pixel; wave = workgroup = 8x8 tile.  Every lane
// of a wave runs the sample loop (lanes past the image edge are idle but
// present) so the culling reductions see converged waves.  CULL selects the
// shadow-culled LAMBERT_SHADOW variant (the host picks it per scene).
// LT: the launch traits (LaunchAny, LaunchPlain above).
template <int MODE, class S, bool SINGLE = false, bool CULL = false, class LT = LaunchAny>
__device__ __forceinline__ void ray_kernel_body(const KParams& kp, const S& sc, const Cull& cl,
                                                uint32_t* __restrict__ out_rgba8, float4* __restrict__ out_f32,
                                                unsigned long long* __restrict__ counters) {
    constexpr bool kPlain = LT::kPlain;
    static_assert(!kPlain || SINGLE, "a plain launch renders one sample per pixel");
    const uint32_t debug = launch_debug<LT>(kp);
    const uint32_t lane = threadIdx.x & 63u;
    // RRTE_DEBUG bit 2 (diagnostics): every index this wave derives from the launch (list slot, tile,
    // frame) is range-checked before use; a violation sets a bit in the check word (counters[1], an
    // unused word of shard 0; rrte_hip_check_word) and the wave stops instead of touching memory
    if ((debug & 4u) && !launch_indices_ok(kp, counters)) return;
    LaunchTile tile = launch_tile(kp);
    if (!tile.run) return;
    if constexpr (kPlain) tile.z = 0u;
    // frame tile.z of the launch: its camera, its output (multi-frame launches have no f32 output)
    const FrameCam& cm = kp.cam[tile.z];
    if constexpr (!kPlain) {
        if (kp.out_image_rows)
            out_rgba8 = cm.out;
        else if (out_rgba8 && tile.z)
            out_rgba8 = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(out_rgba8) + tile.z * kp.frame_stride);
    }
    // RRTE_DEBUG bit 4 (diagnostics, tools/wave_times.py): per-wave start / duration from the 100 MHz
    // wall clock into the f32 buffer instead of colours
    const bool stamps = !kPlain && (debug & 16u) && out_f32;
    const uint32_t tiles_x = kp.tiles_x;
    // bit 5: only workgroup (debug >> 16) runs (its waves' durations alone on the GPU)
    const uint32_t brow = tile.y;
    if ((debug & 32u) && brow * tiles_x + tile.x != (debug >> 16)) return;
    const bool timed = stamps || (kp.tile_cost && tile.z == 0u);
    const uint64_t t_wave0 = timed ? wall_clock64() : 0ull;
    const uint32_t ts = kp.tile_shift;  // (tile 1 << ts wide, 64 >> ts rows)
    const uint32_t x = (tile.x << ts) + (lane & ((1u << ts) - 1u));
    const uint32_t lr = brow * (64u >> ts) + (lane >> ts);
    bool live = x < kp.width && lr < kp.rows;
    const uint32_t xc = live ? x : 0u;
    const uint32_t y = image_row<LT>(kp, live ? lr : 0u);
    if ((debug & 4u) && live && y >= kp.height) {  // (bit 2: a band mapping past the frame)
        atomicOr(counters + 1, 8ull);
        live = false;
    }
    const uint32_t pix = y * kp.width + xc;
    uint32_t nshadow = 0;
    Col acc{0.0f, 0.0f, 0.0f, 1.0f};  // BLACK
    const uint32_t nsamples = SINGLE ? 1u : kp.spp;
    const uint32_t pmask = camera_tile_mask<LT>(kp, cm, tile.x, tile.y);
    // camera ray of sample s (raytracer.rs:66-70): per-(pixel, sample) RNG stream, jitter, generate_ray
    auto camera_ray = [&](uint32_t s, uint32_t& st) {
        st = pcg_hash(pcg_hash(pcg_hash(kp.seed) ^ pix) ^ s);
        float jx = 0.5f, jy = 0.5f;
        if (kp.jitter == RRTE_JITTER_RANDOM) {
            jx = rng_f32(st);
            jy = rng_f32(st);
        }
        float u = ((float)xc + jx) / (float)kp.width;
        float v = ((float)y + jy) / (float)kp.height;
        return generate_ray(cm, u, v);
    };
    auto accumulate = [&](const Col& c) {
        acc.r = acc.r + c.r;
        acc.g = acc.g + c.g;
        acc.b = acc.b + c.b;
        acc.a = acc.a + c.a;
    };
    // All-miss tile: every object of the scene is in the rectangle table and none of their rectangles
    // meets this tile, so no camera ray of the wave can hit anything (the bound camera_tile_mask
    // culls single tests with).  Each sample then adds what the search adds for a miss -- the
    // background, or BLACK at max_depth 0 -- without ray generation, search or shading; such lanes cast
    // no shadow ray.  (pmask's bits past the table are set: only the table's bits count.)
    const uint32_t tn = cm.tile_n;
    const bool all_miss = cm.tile_cull != 0u && tn >= kp.num_prims && (pmask & (tn < 32u ? ~(~0u << tn) : ~0u)) == 0u;
    if (all_miss) {
        const Col c = kp.max_depth == 0 ? Col{0.0f, 0.0f, 0.0f, 1.0f} : Col{kp.bg[0], kp.bg[1], kp.bg[2], kp.bg[3]};
        for (uint32_t s = 0; s < nsamples; ++s) accumulate(c);
    } else if constexpr (MODE == RRTE_MODE_REFCOMPAT && !SINGLE) {
        // Path regeneration: one loop advances every lane's current path by one bounce; a lane
        // whose path ends adds its colour and starts its next sample at once.  A wave then costs
        // the largest per-lane total of bounces instead of the sum over samples of each sample's
        // longest path.  Same per-sample RNG streams and accumulation order as the nested loops.
        if (kp.max_depth == 0) {
            for (uint32_t s = 0; s < nsamples; ++s) accumulate(Col{0.0f, 0.0f, 0.0f, 1.0f});
        } else {
            uint32_t s = 0, st = 0;
            bool active = false;
            PathState ps;
#pragma unroll 1
            for (;;) {
                if (!active && live && s < nsamples) {
                    path_begin(ps, camera_ray(s, st));
                    active = true;
                }
                if (!__any(active)) break;
                // (camera-ray tile culling while every active lane is on its camera ray was measured
                // slower, 0.94 -> 1.00 ms on the stock config: the runtime mask costs every bounce)
                if (active && path_step(sc, kp, ps, st)) {
                    accumulate(ps.out);
                    active = false;
                    ++s;
                }
            }
        }
    } else {
        for (uint32_t s = 0; s < nsamples; ++s) {
            uint32_t st;
            Ray r = camera_ray(s, st);
            Col c{0.0f, 0.0f, 0.0f, 1.0f};
            if (MODE == RRTE_MODE_LAMBERT_SHADOW) {
                c = shade_lambert<S, CULL, LT>(sc, kp, cl, r, live, nshadow, pmask);
            } else if (live) {
                c = ray_color_ref<S, SINGLE>(sc, kp, r, st, SINGLE ? pmask : ~0u);
            }
            accumulate(c);
        }
    }
    if constexpr (kPlain) {
        // inv_spp = 1 (x * 1 = x), gamma 2.2, RGBA8 in device memory at the packed rows: the general
        // epilogue below with its run-time choices taken
        if (live) {
            const size_t o = (size_t)lr * kp.width + x;
            out_rgba8[o] = gamma22_u8(acc.r) | (gamma22_u8(acc.g) << 8) | (gamma22_u8(acc.b) << 16) |
                           (sat_u8(acc.a) << 24);
        }
    } else if (live) {
        acc.r = acc.r * kp.inv_spp;
        acc.g = acc.g * kp.inv_spp;
        acc.b = acc.b * kp.inv_spp;
        acc.a = acc.a * kp.inv_spp;
        const float ig = kp.inv_gamma;
        const float ga = rclamp(acc.a);
        const size_t o = (size_t)(kp.out_image_rows ? y : lr) * kp.width + x;  // packed local rows, or image rows
        // the parity float buffer (or a gamma other than the reference's 2.2) needs powf itself
        const bool exact_pow = (out_f32 && !stamps) || ig != kInvGamma22;
        float gr = 0.0f, gg = 0.0f, gb = 0.0f;
        if (exact_pow) {
            gr = rclamp(powf(acc.r, ig));
            gg = rclamp(powf(acc.g, ig));
            gb = rclamp(powf(acc.b, ig));
        }
        if (out_rgba8) {
            const uint32_t px = exact_pow ? (to_u8(gr) | (to_u8(gg) << 8) | (to_u8(gb) << 16) | (to_u8(ga) << 24))
                                          : (gamma22_u8(acc.r) | (gamma22_u8(acc.g) << 8) | (gamma22_u8(acc.b) << 16) |
                                             (to_u8(ga) << 24));
            if (kp.flags & kFlagSlabRgb24) {  // gather slab, alpha proven 255: 3 bytes per pixel
                uint8_t* b = reinterpret_cast<uint8_t*>(out_rgba8) + 3u * o;
                b[0] = (uint8_t)px;
                b[1] = (uint8_t)(px >> 8);
                b[2] = (uint8_t)(px >> 16);
            } else if (kp.flags & kFlagHostStore) {  // zero-copy frame: out now, not at the kernel's end
                __hip_atomic_store(out_rgba8 + o, px, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            } else {
                out_rgba8[o] = px;
            }
        }
        if (out_f32 && !stamps) {
            if (kp.flags & RRTE_FLAG_F32_LINEAR)
                out_f32[o] = make_float4(acc.r, acc.g, acc.b, acc.a);
            else
                out_f32[o] = make_float4(gr, gg, gb, ga);
        }
    }
    if (MODE != RRTE_MODE_REFCOMPAT) {
        // wave-reduce the shadow-ray count, one atomic per wave
        uint32_t v = nshadow;  // (DPP row sums, then the four rows' lanes: as wave_min)
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);
        v = (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
            (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
        // 256 counter shards, one 128-B line each: same-address atomics from
        // every wave of the grid would serialise at the memory side.
        if (lane == 0 && v) {
            const uint32_t shard = (tile.x + tile.y * tiles_x + threadIdx.x / 64u * 61u) & (kCounterShards - 1u);
            atomicAdd(counters + shard * kCounterStride, (unsigned long long)v);
        }
    }
    if (kp.tile_cost && tile.z == 0u && lane == 0)  // tile profile (TileProfile, rrte_hip.hip)
        kp.tile_cost[brow * tiles_x + tile.x] = (uint32_t)(wall_clock64() - t_wave0);
    if (stamps && lane == 0) {
        const uint64_t t1 = wall_clock64();
        const uint32_t wid = (brow * tiles_x + tile.x) * 4u;  // (every fourth record: tools/wave_times.py)
        uint32_t* s = reinterpret_cast<uint32_t*>(out_f32) + 4u * wid;
        s[0] = (uint32_t)t_wave0;
        s[1] = (uint32_t)(t_wave0 >> 32);
        s[2] = (uint32_t)(t1 - t_wave0);
        s[3] = __smid();
    }
}

// Generic kernel: the scene is read from HBM through wave-uniform (scalar) loads; F = the features
// compiled in (kFeat*, a superset of the scene's).
// Register budget of the generic kernel (waves per SIMD it must fit): 5 (<= 96 VGPRs, a few spills)
// instead of the compiler's 4 -- frames in a stream 0.172 -> 0.164 ms per 1080p showcase frame, a lone
// launch +13 % -- and, once the scene records were scalar loads, 6 (<= 80 VGPRs) for LAMBERT_SHADOW
// variants without meshes or deformers: 0.139 -> 0.131 ms; with meshes (+39 %) or deformers (+5 %) 6 waves
// lose, so those keep 5, as do the REFCOMPAT variants (6 waves: one sample -3 %, the reference's stock config
// spp 4 / depth 50 +6 %; DESIGN.md §13, tools/mw_check.sh, tools/refc_check.sh)
#ifndef RRTE_GENERIC_MINWAVES
#define RRTE_GENERIC_MINWAVES 5
#endif
#ifndef RRTE_GENERIC_MINWAVES_PLAIN
#define RRTE_GENERIC_MINWAVES_PLAIN 6
#endif
template <int MODE, uint32_t F>
constexpr int generic_min_waves() {
    return MODE == RRTE_MODE_LAMBERT_SHADOW && (F & (kFeatMesh | kFeatDeform)) == 0u ? RRTE_GENERIC_MINWAVES_PLAIN
                                                                                        : RRTE_GENERIC_MINWAVES;
}
template <int MODE, bool CULL, uint32_t F = kFeatAll>
__global__ __launch_bounds__(kBlockThreads, (generic_min_waves<MODE, F>())) void ray_kernel(KParams kp, SceneView sc, Cull cl, uint32_t* __restrict__ out_rgba8,
                                                  float4* __restrict__ out_f32,
                                                  unsigned long long* __restrict__ counters) {
    SceneViewF<F> s;
    static_cast<SceneView&>(s) = sc;
    ray_kernel_body<MODE, SceneViewF<F>, false, CULL>(kp, s, cl, out_rgba8, out_f32, counters);
}

}  // namespace rrte
