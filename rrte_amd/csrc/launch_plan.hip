// launch_plan.hip — what one launch of the ray kernel is, decided on the host: the kernel parameters,
// the camera-ray tile rectangles, the band partition of a multi-GPU frame and the launch plan.  Host
// arithmetic only; no kernel is instantiated or launched here.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>

#include "context.hpp"

using namespace rrte;

namespace rrte {

KParams make_params(const rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, uint32_t rows) {
    KParams k;
    memset(&k, 0, sizeof k);
    k.width = p->width;
    k.height = p->height;
    k.spp = p->samples_per_pixel;
    k.max_depth = p->max_depth;
    k.jitter = p->jitter;
    k.seed = p->seed;
    k.flags = p->flags;
    k.num_prims = s->num_prims;
    k.num_lights = s->num_lights;
    k.num_materials = s->num_materials;
    k.rows = rows;
    k.band_rows = c->nranks > 1 ? p->band_rows : 0;
    k.nranks = (uint32_t)c->nranks;
    k.rank = (uint32_t)c->rank;
    k.sky_bands = 0;  // (the plain interleave; plan_launch applies a frame's BandMap)
    k.root_bands = 1;
    k.peer_bands = 1;
    memcpy(k.bg, p->background, sizeof k.bg);
    k.t_min = p->t_min;
    k.bias = p->shadow_bias;
    k.inv_gamma = 1.0f / p->gamma;                        // raytracer.rs:79 -> color.rs:60
    k.inv_spp = 1.0f / (float)p->samples_per_pixel;       // raytracer.rs:76
    k.nframes = 1;
    k.frame_stride = 0;
    const rrte_camera& cam = s->camera;
    FrameCam& fc = k.cam[0];
    fc.projection = cam.projection;
    memcpy(fc.cam_pos, cam.position, sizeof fc.cam_pos);
    memcpy(fc.cam_rot, cam.rotation, sizeof fc.cam_rot);
    fc.half_h = tanf(cam.fov * 0.5f);                     // camera.rs:104
    fc.aspect = cam.aspect_ratio;
    fc.ortho_l = cam.left; fc.ortho_r = cam.right; fc.ortho_b = cam.bottom; fc.ortho_t = cam.top;
    float trs[10] = {cam.position[0], cam.position[1], cam.position[2], cam.rotation[0], cam.rotation[1],
                     cam.rotation[2], cam.rotation[3], cam.scale[0], cam.scale[1], cam.scale[2]};
    float m[16];
    mat4_srt(trs, m);
    to_affine12(m, fc.cam_xf);
    k.debug = c->env.debug;  // RRTE_DEBUG ablation bits (profiling only)
    return k;
}

// Camera-ray tile culling (KParams::tile_rect, ray_kernels.hpp camera_tile_mask), perspective frames:
// for each of the first 32 objects, the 8x8-pixel tiles (16x16 for frames wider or taller than 2048)
// whose camera rays can reach its culling
// sphere (the conservative bound shadow culling uses: centre, radius).  In camera space a ray
// direction (x, y, -1) that meets the sphere projects, in the xz plane, onto a line through the eye
// that meets the sphere's disc there, so x lies between the tangents of that disc (likewise y in the
// yz plane).  Double precision, then 2 pixels of margin per side -- orders of magnitude above the f32
// error of the device's ray directions (~1e-6 of the field of view) and of random jitter's extent
// (inside the pixel).  A sphere that contains the eye keeps the whole frame; one that reaches the
// plane z = 0 from outside the eye keeps every column and the rows from its silhouette's top down.
// Bit-identical results by construction: a skipped test is one every lane would miss
// (tests/test_gpu_parity.py test_camera_tile_culling_is_exact).
static void fill_tile_rects_uncached(const rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, KParams& kk);

// The rectangles depend only on the camera, the frame size, the band height and the cached scene's
// bounds: frames of an unchanged camera reuse the last result (the double-precision trigonometry is
// most of a frame call's host time in the batched multi-GPU path).
static void fill_tile_rects(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, KParams& kk) {
    auto& tc = c->tile_rect_cache;
    if (tc.valid && tc.gen == c->scene_gen && tc.width == p->width && tc.height == p->height &&
        tc.band == kk.band_rows && !memcmp(&tc.cam, &s->camera, sizeof tc.cam)) {
        kk.cam[0].tile_cull = tc.tile_cull;
        kk.cam[0].tile_n = tc.tile_n;
        memcpy(kk.cam[0].tile_rect, tc.rect, sizeof tc.rect);
        return;
    }
    fill_tile_rects_uncached(c, s, p, kk);
    tc.valid = true;
    tc.gen = c->scene_gen;
    tc.width = p->width;
    tc.height = p->height;
    tc.band = kk.band_rows;
    tc.cam = s->camera;
    tc.tile_cull = kk.cam[0].tile_cull;
    tc.tile_n = kk.cam[0].tile_n;
    memcpy(tc.rect, kk.cam[0].tile_rect, sizeof tc.rect);
}

static void tile_rects(bool enabled, const std::vector<float4>& bounds, const rrte_scene_ir* s, const rrte_render_params* p,
                       KParams& kk);
static void fill_tile_rects_uncached(const rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, KParams& kk) {
    tile_rects(c->env.tile_cull, c->h_bounds, s, p, kk);
}
static void tile_rects(bool enabled, const std::vector<float4>& bounds, const rrte_scene_ir* s, const rrte_render_params* p,
                       KParams& kk) {
    FrameCam& k = kk.cam[0];
    const uint32_t band_rows = kk.band_rows;
    k.tile_cull = 0;
    // 8x8 tiles (one per wave) when their indices fit 8 bits and bands keep 8-row tiles whole,
    // else 16x16 blocks (four 8x8 workgroups)
    auto fits = [&](uint32_t sh) {
        const uint32_t t = 1u << sh;
        return (p->width + t - 1) / t <= 256 && (p->height + t - 1) / t <= 256 &&
               (band_rows == 0 || band_rows % t == 0);
    };
    const uint32_t sh = fits(3) ? 3u : (fits(4) ? 4u : 0u);
    if (!enabled || s->camera.projection != RRTE_PERSPECTIVE || sh == 0 || bounds.size() < s->num_prims)
        return;
    const uint32_t nbx = (p->width + (1u << sh) - 1) >> sh, nby = (p->height + (1u << sh) - 1) >> sh;
    const rrte_camera& cam = s->camera;
    // an eye beyond kCullReachHost: the reference's own arithmetic overflows there (hits with t = NaN
    // for rays that pass nowhere near an object), so no tile is culled
    for (int k = 0; k < 3; ++k)
        if (!(std::fabs((double)cam.position[k]) < kCullReachHost)) return;
    double q[4] = {cam.rotation[0], cam.rotation[1], cam.rotation[2], cam.rotation[3]};
    const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(qn > 0.0) || !std::isfinite(qn)) return;
    for (double& v : q) v /= qn;
    const double hh = std::tan(0.5 * (double)cam.fov), hw = (double)cam.aspect_ratio * hh;
    if (!(hh > 0.0) || !(hw > 0.0) || !std::isfinite(hh) || !std::isfinite(hw)) return;
    // world -> camera: the inverse rotation (conjugate quaternion) of v - position
    auto to_cam = [&](const double v[3], double out[3]) {
        const double bx = -q[0], by = -q[1], bz = -q[2], w = q[3];
        const double vb = v[0] * bx + v[1] * by + v[2] * bz, k0 = w * w - (bx * bx + by * by + bz * bz);
        const double cx = by * v[2] - bz * v[1], cy = bz * v[0] - bx * v[2], cz = bx * v[1] - by * v[0];
        out[0] = v[0] * k0 + 2.0 * bx * vb + 2.0 * w * cx;
        out[1] = v[1] * k0 + 2.0 * by * vb + 2.0 * w * cy;
        out[2] = v[2] * k0 + 2.0 * bz * vb + 2.0 * w * cz;
    };
    const uint32_t n = s->num_prims < 32u ? s->num_prims : 32u;
    const double margin = 2.0;
    for (uint32_t i = 0; i < n; ++i) {
        const float4 b = bounds[i];
        uint32_t rect = 0u | ((nbx - 1) << 8) | (0u << 16) | ((nby - 1) << 24);  // whole frame
        const double R = (double)b.w;
        const double w[3] = {(double)b.x - cam.position[0], (double)b.y - cam.position[1], (double)b.z - cam.position[2]};
        double v[3];
        to_cam(w, v);
        const bool finite = std::isfinite(R) && std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);
        const bool in_front = finite && R >= 0.0 && v[2] < -R * 1.001 - 1e-6;
        // A sphere that reaches the eye plane but keeps the eye outside (a ground sphere under the
        // camera): its top row from a tangent plane of the cone of directions that meet it.  Let w be
        // the unit vector of the image plane (x, y) towards the centre and r the centre's distance
        // from the view axis.  A camera ray (x, s, -1) t projects, along the direction of the image
        // plane normal to w, onto the half-line (q, -1) t with q = (x, s) . w, and a ray that meets the
        // sphere then meets its disc there (centre (r, cz), radius R: dropping a coordinate only
        // brings a point closer to the centre).  With the origin outside the disc (the eye outside
        // the sphere) the directions that meet it lie within beta = asin(R / D) of the centre's
        // direction alpha = atan2(r, -cz) in [0, 180] degrees, measured from the view axis towards w;
        // a camera ray is at atan(q) in (-90, 90), so a hit needs q >= tan(alpha - beta) =: t -- for
        // alpha - beta >= 90 degrees no camera ray hits at all, at or below -90 nothing is known.  With
        // w pointing down the image (wy < 0) that reads s <= (x wx - t) / -wy, at most
        // (hw |wx| - t) / -wy over the frame's columns |x| <= hw: the horizon's highest point.
        // Only the top is bounded; double precision and the margin of the other sides.  The eye keeps
        // a distance of 1e-4 R from the surface: closer, the device's f32 discriminant is too coarse
        // for a bound of two pixels.
        const double dist = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), rad = std::sqrt(v[0] * v[0] + v[1] * v[1]);
        if (finite && R > 0.0 && !in_front && dist > R * 1.0001 && rad > 1e-9 * dist) {
            const double kHalfPi = 1.57079632679489661923, lo = std::atan2(rad, -v[2]) - std::asin(R / dist);
            const double wx = v[0] / rad, wy = v[1] / rad, H = p->height;
            if (lo > kHalfPi - 1e-9) {
                if (lo > kHalfPi + 1e-9) rect = 0xFFu | (0xFFu << 16);  // behind the eye: no block (as below)
            } else if (lo > -kHalfPi + 1e-9 && wy < -1e-9) {
                const double s_top = (hw * std::fabs(wx) - std::tan(lo)) / -wy;
                const double py0 = (1.0 - s_top / hh) * H * 0.5 - 0.5 - margin;
                if (py0 > H - 1.0) {
                    rect = 0xFFu | (0xFFu << 16);
                } else if (std::isfinite(py0) && py0 > 0.0) {
                    const uint32_t by0 = (uint32_t)std::min<double>(std::floor(py0 / (double)(1u << sh)), (double)(nby - 1));
                    rect = 0u | ((nbx - 1) << 8) | (by0 << 16) | ((nby - 1) << 24);
                }
            }
        }
        if (in_front) {  // entirely in front of the eye (z < 0)
            // tangent slopes of the disc (centre (c, -d), radius R, d > R) seen from the origin:
            // tan(alpha -/+ beta) with tan alpha = c / d and tan beta = R / sqrt(D^2 - R^2), by the
            // angle-sum identity (no trigonometry: this runs per object for every new camera).  The
            // disc lies in z < 0, so both tangents point forward (|alpha +/- beta| < pi/2) and both
            // denominators are positive; a non-positive one (rounding at the limit) leaves that
            // side unbounded
            auto range = [&](double cc, double& lo, double& hi) {
                const double d = -v[2], h2 = cc * cc + d * d - R * R;
                const double inf = std::numeric_limits<double>::infinity();
                if (!(h2 > 0.0)) {
                    lo = -inf;
                    hi = inf;
                    return;
                }
                const double ta = cc / d, tb = R / std::sqrt(h2);
                const double dl = 1.0 + ta * tb, dh = 1.0 - ta * tb;
                lo = dl > 0.0 ? (ta - tb) / dl : -inf;
                hi = dh > 0.0 ? (ta + tb) / dh : inf;
            };
            double xl, xh, yl, yh;
            range(v[0], xl, xh);
            range(v[1], yl, yh);
            // ndc_x = x / hw, pixel x = (ndc_x + 1) W / 2 - 1/2;  ndc_y = y / hh, pixel y = (1 - ndc_y) H / 2 - 1/2
            const double W = p->width, H = p->height;
            const double px0 = (xl / hw + 1.0) * W * 0.5 - 0.5 - margin, px1 = (xh / hw + 1.0) * W * 0.5 - 0.5 + margin;
            const double py0 = (1.0 - yh / hh) * H * 0.5 - 0.5 - margin, py1 = (1.0 - yl / hh) * H * 0.5 - 0.5 + margin;
            if (std::isfinite(px0) && std::isfinite(px1) && std::isfinite(py0) && std::isfinite(py1)) {
                if (px1 < 0.0 || py1 < 0.0 || px0 > W - 1.0 || py0 > H - 1.0) {
                    rect = 0xFFu | (0xFFu << 16);  // bx0 = 255 > bx1 = 0: no block (block indices <= 255)
                } else {
                    auto blk = [sh](double px, uint32_t nb) {
                        const double b = std::floor(px / (double)(1u << sh));
                        return (uint32_t)std::min<double>(std::max<double>(b, 0.0), (double)(nb - 1));
                    };
                    rect = blk(px0, nbx) | (blk(px1, nbx) << 8) | (blk(py0, nby) << 16) | (blk(py1, nby) << 24);
                }
            }
        }
        k.tile_rect[i] = rect;
    }
    k.tile_n = n;
    k.tile_cull = sh;
}

constexpr uint32_t kMaxCycleBands = 8u;  // largest root_bands / peer_bands of a partition

uint32_t rows_for_rank(uint32_t height, uint32_t band_rows, int nranks, int rank, uint32_t sky,
                       uint32_t root_bands, uint32_t peer_bands) {
    if (nranks <= 1 || band_rows == 0) return height;
    const BandMap m{band_rows, (uint32_t)nranks, sky, root_bands, peer_bands};
    uint32_t nb = (height + band_rows - 1) / band_rows, rows = 0;
    for (uint32_t b = 0; b < nb; ++b) {
        uint32_t lb = 0;
        if (band_owner(m, b, lb) != (uint32_t)rank) continue;
        uint32_t r0 = b * band_rows, r1 = r0 + band_rows < height ? r0 + band_rows : height;
        rows += r1 - r0;
    }
    return rows;
}

// The number of leading bands no object reaches (band_layout); 0 when it cannot be judged.
static uint32_t sky_band_count(const rrte_camera& cam, const std::vector<float4>& bounds, uint32_t num_prims,
                               uint32_t height, uint32_t band_rows) {
    if (cam.projection != RRTE_PERSPECTIVE || bounds.size() < num_prims || num_prims == 0) return 0u;
    double q[4] = {cam.rotation[0], cam.rotation[1], cam.rotation[2], cam.rotation[3]};
    const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double hh = std::tan(0.5 * (double)cam.fov), hw = (double)cam.aspect_ratio * hh;
    if (!(qn > 0.0) || !std::isfinite(qn) || !(hh > 0.0) || !(hw > 0.0) || !std::isfinite(hh * hw)) return 0u;
    for (double& v : q) v /= qn;
    auto to_cam = [&](const double v[3], double out[3]) {  // the inverse rotation (as fill_tile_rects)
        const double bx = -q[0], by = -q[1], bz = -q[2], w = q[3];
        const double vb = v[0] * bx + v[1] * by + v[2] * bz, k0 = w * w - (bx * bx + by * by + bz * bz);
        const double cx = by * v[2] - bz * v[1], cy = bz * v[0] - bx * v[2], cz = bx * v[1] - by * v[0];
        out[0] = v[0] * k0 + 2.0 * bx * vb + 2.0 * w * cx;
        out[1] = v[1] * k0 + 2.0 * by * vb + 2.0 * w * cy;
        out[2] = v[2] * k0 + 2.0 * bz * vb + 2.0 * w * cz;
    };
    double top = std::numeric_limits<double>::infinity();  // topmost image row any object reaches
    for (uint32_t i = 0; i < num_prims; ++i) {
        const float4 b = bounds[i];
        const double R = b.w;
        const double w[3] = {(double)b.x - cam.position[0], (double)b.y - cam.position[1], (double)b.z - cam.position[2]};
        double v[3];
        to_cam(w, v);
        const double D = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (!std::isfinite(R) || !std::isfinite(D) || D <= R * 1.0001) return 0u;  // unbounded / around the eye
        const double u[3] = {v[0] / D, v[1] / D, v[2] / D}, cos2 = 1.0 - (R / D) * (R / D);
        for (int col = 0; col <= 16; ++col) {
            // image-plane point (px, s, -1): inside the cone iff d = u.p > 0 and d^2 >= cos2 |p|^2
            const double px = (2.0 * col / 16.0 - 1.0) * hw, k = u[0] * px - u[2], mm = px * px + 1.0;
            const double A = u[1] * u[1] - cos2, B = 2.0 * u[1] * k, C = k * k - cos2 * mm;
            auto inside = [&](double s) { return u[1] * s + k > 0.0 && A * s * s + B * s + C >= -1e-12; };
            double cand[3] = {hh, -std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
            const double disc = B * B - 4.0 * A * C;
            if (A != 0.0 && disc >= 0.0) {
                const double sq = std::sqrt(disc);
                cand[1] = (-B + sq) / (2.0 * A);
                cand[2] = (-B - sq) / (2.0 * A);
            } else if (A == 0.0 && B != 0.0) {
                cand[1] = -C / B;
            }
            std::sort(cand, cand + 3, [](double x, double y) { return x > y; });
            for (double sv : cand) {
                if (!(sv <= hh) || !(sv >= -hh) || !inside(sv)) continue;
                top = std::min(top, (1.0 - sv / hh) * height * 0.5 - 0.5);  // image row of ndc_y = s / hh
                break;
            }
        }
    }
    const double free_rows = top - band_rows;  // one band of margin
    const uint32_t nb = (height + band_rows - 1) / band_rows;
    uint32_t sky = free_rows > 0.0 ? (uint32_t)std::min<double>(std::floor(free_rows / band_rows), nb) : 0u;
    return sky >= nb ? 0u : sky;  // (nothing visible at all: the plain interleave)
}

// The band partition of a multi-GPU frame (BandMap, device_scene.hpp).  The leading "sky" bands --
// rows above every object's silhouette, where every camera ray misses (the cheapest rows of the
// frame) -- go to the root; the other bands go round robin, root_bands for the root per peer_bands
// for every peer, the pair chosen by a work model so the busiest rank is least busy.
// The silhouette top: per object, the cone of directions from the eye that meet its culling sphere,
// cut at 17 columns across the frame on the image plane (a quadratic per column, double precision),
// minus one band of margin.  This decides only WHICH rank renders a band -- never a pixel -- so the
// sampling need not be conservative.  Every rank computes the same partition from the same scene and
// camera (host arithmetic only).  RRTE_BAND_SKY=0: the plain interleave (sky 0, 1:1).
static BandMap band_layout(const rrte_camera& cam, const std::vector<float4>& bounds, uint32_t num_prims, uint32_t width,
                           uint32_t height, uint32_t band_rows, int nranks, int root, bool enabled) {
    BandMap m{band_rows, (uint32_t)std::max(nranks, 1), 0u, 1u, 1u};
    if (!enabled || nranks <= 1 || root != 0 || band_rows == 0) return m;
    m.sky = sky_band_count(cam, bounds, num_prims, height, band_rows);
    // The root's round-robin share: the (root_bands, peer_bands) pair giving the smallest busiest rank
    // under a work model over the actual band counts, fitted to emulated rank frames of the 1080p
    // showcase: a non-sky row costs 1, a sky row kSkyCost (camera rays that miss), and the root spends
    // kExpandCost per peer row it receives and expands (RCCL receive + the RGB24 expansion); ties
    // keep the smaller cycle
    constexpr double kSkyCost = 0.15, kExpandCost = 0.09;
    const uint32_t nb = (height + band_rows - 1) / band_rows;
    // The choice depends on the sky count, not on the camera itself: a moving camera repeats a few sky
    // counts, so each (sky, frame height, band height, ranks) is searched once (the search over every
    // pair and band was most of a moving-camera frame call's host time)
    struct Choice { uint32_t sky, height, band_rows, nranks, a, b; };
    thread_local std::vector<Choice> memo;
    for (const Choice& ch : memo)
        if (ch.sky == m.sky && ch.height == height && ch.band_rows == band_rows && ch.nranks == (uint32_t)nranks) {
            m.root_bands = ch.a;
            m.peer_bands = ch.b;
            return m;
        }
    std::vector<double> load((size_t)nranks);
    double best = std::numeric_limits<double>::infinity();
    for (uint32_t a = 0; a <= kMaxCycleBands; ++a)
        for (uint32_t b = 1; b <= kMaxCycleBands; ++b) {
            if (a == 0 ? b != 1 : std::gcd(a, b) != 1) continue;  // (one representative per ratio)
            if (a == 0 && m.sky == 0) continue;                   // (the root would own nothing)
            const BandMap t{band_rows, (uint32_t)nranks, m.sky, a, b};
            std::fill(load.begin(), load.end(), 0.0);
            for (uint32_t band = 0; band < nb; ++band) {
                uint32_t lb = 0;
                const uint32_t rows = std::min(band_rows, height - band * band_rows), o = band_owner(t, band, lb);
                load[o] += band < m.sky ? kSkyCost * rows : (double)rows;
                if (o != 0) load[0] += kExpandCost * rows;
            }
            const double busiest = *std::max_element(load.begin(), load.end());
            if (busiest < best - 1e-9) best = busiest, m.root_bands = a, m.peer_bands = b;
        }
    if (memo.size() >= 64) memo.clear();
    memo.push_back(Choice{m.sky, height, band_rows, (uint32_t)nranks, m.root_bands, m.peer_bands});
    return m;
}

// Shadow-ray culling (cull.hpp, shadow_cull) for LAMBERT_SHADOW frames: one lane per object,
// so scenes of <= 64 objects; it pays where an occlusion test is expensive (sphere-traced SDF
// objects) and costs a few percent on all-analytic scenes (measured).  RRTE_CULL=0/1
// forces it off/on (A/B runs, tests).
bool cull_policy(const rrte_scene_ir* s, uint32_t mode, int env_cull) {
    if (mode != RRTE_MODE_LAMBERT_SHADOW || s->num_prims > 64) return false;
    if (env_cull >= 0) return env_cull != 0;
    for (uint32_t i = 0; i < s->num_prims; ++i)
        if (s->prims[i].kind == RRTE_PRIM_SDF) return true;
    return false;
}

// Tile rows of a launch of `rows` rows (KParams::tile_shift: tiles 64 >> tile_shift rows high).
uint32_t tile_grid_rows(const KParams& k, uint32_t rows) {
    const uint32_t th = 64u >> k.tile_shift;
    return (rows + th - 1u) / th;
}

LaunchPlan plan_launch(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, uint32_t rows,
                       uint32_t internal_flags, uint32_t row0, const BandMap* bm) {
    LaunchPlan L;
    L.k = make_params(c, s, p, rows);
    if (bm && L.k.band_rows) {
        L.k.sky_bands = bm->sky;
        L.k.root_bands = bm->root_bands;
        L.k.peer_bands = bm->peer_bands;
    }
    L.k.row0 = row0;  // (image rows [row0, row0 + rows); band_rows == 0)
    L.k.flags |= internal_flags;
    L.mode = (int)p->mode;
    L.cull = cull_policy(s, p->mode, c->env.cull);
    // single-sample, single-bounce frames get the straight-line specialisation (SINGLE); others the
    // specialisation with runtime sample / bounce loops
    L.single = p->samples_per_pixel == 1 && (p->mode == RRTE_MODE_LAMBERT_SHADOW || p->max_depth <= 1);
    L.num_prims = s->num_prims;
    L.num_lights = s->num_lights;
    L.num_materials = s->num_materials;
    L.k.tile_shift = c->tile_shift;  // one tile per 64-thread workgroup (kBlockThreads): 8x8 unless overridden
    L.gx = (p->width + (1u << L.k.tile_shift) - 1u) >> L.k.tile_shift;
    L.gy = tile_grid_rows(L.k, rows);
    fill_tile_rects(c, s, p, L.k);
    return L;
}

// The band partition of one multi-GPU frame of this context (band_layout from the frame's camera-ray
// tile rectangles; `p` with its band_rows set).
// The band partition of a multi-GPU frame, this rank's rows under it and the slab rows (the most any
// rank owns); the last answer is kept (the same camera, scene, size, rank and rank count)
const BandMap& frame_band_map(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p, int root,
                              uint32_t* rows, uint32_t* cap) {
    auto& bc = c->band_cache;
    if (!(bc.valid && bc.gen == c->scene_gen && bc.w == p->width && bc.h == p->height && bc.band == p->band_rows &&
          bc.nranks == c->nranks && bc.root == root && bc.rank == c->rank &&
          !memcmp(&bc.cam, &s->camera, sizeof bc.cam))) {
        bc.m = band_layout(s->camera, c->h_bounds, s->num_prims, p->width, p->height, p->band_rows, c->nranks, root,
                           c->env.band_sky);
        bc.valid = true;
        bc.gen = c->scene_gen;
        bc.w = p->width;
        bc.h = p->height;
        bc.band = p->band_rows;
        bc.nranks = c->nranks;
        bc.root = root;
        bc.rank = c->rank;
        bc.cam = s->camera;
        // every rank's rows in one pass over the bands (as rows_for_rank counts them)
        std::vector<uint32_t> per((size_t)c->nranks, 0u);
        if (c->nranks <= 1 || p->band_rows == 0) {
            per.assign((size_t)std::max(c->nranks, 1), p->height);
        } else {
            const uint32_t nb = (p->height + p->band_rows - 1) / p->band_rows;
            for (uint32_t b = 0; b < nb; ++b) {
                uint32_t lb = 0;
                const uint32_t r0 = b * p->band_rows, r1 = std::min(r0 + p->band_rows, p->height);
                per[band_owner(bc.m, b, lb)] += r1 - r0;
            }
        }
        bc.rows = per[(size_t)c->rank];
        bc.cap = *std::max_element(per.begin(), per.end());
    }
    if (rows) *rows = bc.rows;
    if (cap) *cap = bc.cap;
    return bc.m;
}

}  // namespace rrte

extern "C" {

uint32_t rrte_hip_band_rows_for_rank(uint32_t height, uint32_t band_rows, int nranks, int rank) {
    return rows_for_rank(height, band_rows, nranks, rank);
}

rrte_status rrte_hip_band_layout(const rrte_scene_ir* s, const rrte_render_params* p, int nranks, int root,
                                 uint32_t* sky_bands, uint32_t* root_bands, uint32_t* peer_bands) {
    if (!s || !p || !sky_bands || !root_bands || !peer_bands || nranks < 1 || root < 0 || root >= nranks) return RRTE_INVALID_ARG;
    if ((s->num_prims && !s->prims) || (s->num_mesh_indices && !s->mesh_indices) ||
        (s->num_mesh_vertices && !s->mesh_vertices))
        return RRTE_INVALID_ARG;
    rrte_render_params pp = *p;
    if (!pp.band_rows) pp.band_rows = 16;
    std::vector<DPrim> prims;
    std::vector<DMaterial> mats;
    std::vector<DLight> lights;
    std::vector<float4> bounds;
    lower_scene(s, prims, mats, lights, &bounds);
    MeshData md;
    build_mesh_bvhs(s, prims.data(), md, bounds.data());
    const char* g = getenv("RRTE_BAND_SKY");
    const BandMap m = band_layout(s->camera, bounds, s->num_prims, pp.width, pp.height, pp.band_rows, nranks, root,
                                  !(g && g[0] == '0'));
    *sky_bands = m.sky;
    *root_bands = m.root_bands;
    *peer_bands = m.peer_bands;
    return RRTE_OK;
}

// include/rrte_hip_jit.h
rrte_status rrte_hip_tile_rects(const rrte_scene_ir* s, const rrte_render_params* p, uint32_t* tile_shift,
                                uint32_t* count, uint32_t* rects) {
    if (!s || !p || !tile_shift || !count || !rects || p->width == 0 || p->height == 0) return RRTE_INVALID_ARG;
    if ((s->num_prims && !s->prims) || (s->num_mesh_indices && !s->mesh_indices) ||
        (s->num_mesh_vertices && !s->mesh_vertices))
        return RRTE_INVALID_ARG;
    std::vector<DPrim> prims;
    std::vector<DMaterial> mats;
    std::vector<DLight> lights;
    std::vector<float4> bounds;
    lower_scene(s, prims, mats, lights, &bounds);
    MeshData md;
    build_mesh_bvhs(s, prims.data(), md, bounds.data());
    KParams k{};
    tile_rects(true, bounds, s, p, k);  // (k.band_rows 0: a whole frame on one context)
    *tile_shift = k.cam[0].tile_cull;
    *count = k.cam[0].tile_cull ? k.cam[0].tile_n : 0u;
    for (uint32_t i = 0; i < *count; ++i) rects[i] = k.cam[0].tile_rect[i];
    return RRTE_OK;
}

uint32_t rrte_hip_band_rows_for_rank_ex(uint32_t height, uint32_t band_rows, int nranks, int rank, uint32_t sky_bands,
                                        uint32_t root_bands, uint32_t peer_bands) {
    if (root_bands > kMaxCycleBands || peer_bands < 1u || peer_bands > kMaxCycleBands ||
        (root_bands == 0u && sky_bands == 0u))
        return 0u;  // (outside the documented range)
    return rows_for_rank(height, band_rows, nranks, rank, sky_bands, root_bands, peer_bands);
}

}  // extern "C"
