// pixel_encode.hpp — a colour channel to its byte.
//
// The reference's truncating `as u8` and clamp (to_u8, rclamp) and the fixed gamma 2.2 encode without
// powf in the common case (sat_u8, gamma22_u8), bit-identical for all 2^32 inputs.
//
// Includes scene_view.hpp (kInf).  Included by ray_kernels.hpp and by fpcheck.hip, whose sweep checks
// gamma22_u8.  Embedded for hiprtc (the Makefile's DEVICE_HDR).
#pragma once

#include "scene_view.hpp"

namespace rrte {

// Rust `(x * 255.0) as u8` (raytracer.rs:82-85) and f32::clamp (color.rs:48-55)
__device__ __forceinline__ uint32_t to_u8(float c) {
    float v = c * 255.0f;
    if (!(v > 0.0f)) return 0u;
    if (v >= 255.0f) return 255u;
    return (uint32_t)v;
}
__device__ __forceinline__ float rclamp(float x) {
    if (x < 0.0f) return 0.0f;
    if (x > 1.0f) return 1.0f;
    return x;
}

// One channel of the reference's fixed to_gamma(2.2) -> clamp -> truncating u8 (raytracer.rs:79-85,
// color.rs:58-65) without powf in the common case.  The compiler's powf is a ~100-instruction
// double-float sequence, a tenth of the headline kernel with three per pixel.  y = exp2(log2(c)/2.2)
// from v_log_f32 / v_exp_f32 is within a few ulp of it; RN(p*255) and the clamp are monotone in p,
// so when y(1 - m) and y(1 + m) quantise to the same byte every p in between -- powf's result
// included -- does too, and that byte is the answer.  Lanes near a byte boundary, +inf and -inf
// take powf.  Bit-identical to to_u8(rclamp(powf(c, RN(1/2.2)))) for all 2^32 inputs
// (rrte_hip_fpcheck RRTE_FPCHECK_GAMMA_U8, tests/test_gpu_fpexact.py).
constexpr float kInvGamma22 = 1.0f / 2.2f;
constexpr float kGammaMargin = 0x1p-20f;  // relative, ~8 ulp
// to_u8(rclamp(y)) in three straight-line VALU ops: v = RN(y * 255), the hardware's saturating
// float -> unsigned convert (v_cvt_u32_f32: NaN and negatives, -0 included, give 0; in-range values
// truncate; values past 2^32 - 1 give 2^32 - 1), an unsigned min with 255.  Equal for every y:
//  - y NaN: rclamp passes it on, v is NaN, !(v > 0) gives 0; the convert gives 0.
//  - y < 0 (-inf included): rclamp gives 0, byte 0; here v <= -0 (an underflow keeps the sign), byte 0.
//  - y = -0 or +0: rclamp keeps it, v = -0 or +0, !(v > 0) gives 0; the convert gives 0.
//  - 0 < y <= 1: the same v in [0, 255] on both sides; v = 0 (underflow) gives 0 and v = 255 gives
//    255 either way, anything between trunc(v).
//  - y > 1 (+inf included): rclamp gives 1, byte 255; RN(. * 255) is monotone and RN(1 * 255) = 255,
//    so v >= 255, the convert gives >= 255 and the min 255.
// (The branches of to_u8 / rclamp compile to nested EXEC save / branch diamonds at -O1.)
__device__ __forceinline__ uint32_t sat_u8(float y) {
    uint32_t q;
    asm("v_cvt_u32_f32_e32 %0, %1" : "=v"(q) : "v"(y * 255.0f));
    return q < 255u ? q : 255u;
}
__device__ __forceinline__ uint32_t gamma22_u8(float c) {
    const float y = __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(c) * kInvGamma22);
    const float m = y * kGammaMargin;
    const uint32_t a = sat_u8(y - m), b = sat_u8(y + m);
    // c = -inf: log2 gives NaN (byte 0) but powf(-inf, 1/2.2) = +inf (byte 255)
    if (__builtin_expect(a == b && c != -kInf, 1)) return a;
    return to_u8(rclamp(powf(c, kInvGamma22)));
}

}  // namespace rrte
