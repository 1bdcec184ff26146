// mesh_box.hpp — the f32 box arithmetic of the mesh BVH, shared by the host builder (bvh.hip) and the
// device refit (mesh_refit.hip): both must produce the same bits from the same vertices.
//
// Every min / max is the compare-and-select std::min / std::max perform (the first operand wins a
// tie, so +0 against -0 keeps whichever came first); fminf / fmaxf may choose the other signed zero.
// The library is compiled with -ffp-contract=off: inflate()'s d is three individually rounded ops.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rrte {

struct Box {
    float lo[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
    float hi[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
    __host__ __device__ void grow(const float* p) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = p[k] < lo[k] ? p[k] : lo[k];
            hi[k] = hi[k] < p[k] ? p[k] : hi[k];
        }
    }
    __host__ __device__ void grow(const Box& b) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = b.lo[k] < lo[k] ? b.lo[k] : lo[k];
            hi[k] = hi[k] < b.hi[k] ? b.hi[k] : hi[k];
        }
    }
    float area() const {
        float d[3];
        for (int k = 0; k < 3; ++k) d[k] = 0.0f < hi[k] - lo[k] ? hi[k] - lo[k] : 0.0f;
        return 2.0f * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]);
    }
};

// nextafterf(x, +inf) for every x (NaN and +inf return x), as integer steps on the bit pattern.
__host__ __device__ inline float next_up(float x) {
    if (!(x < __builtin_huge_valf())) return x;
    if (x == 0.0f) return __builtin_bit_cast(float, 1u);  // either zero -> the smallest subnormal
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    return __builtin_bit_cast(float, x > 0.0f ? u + 1u : u - 1u);
}
__host__ __device__ inline float next_down(float x) { return -next_up(-x); }

// Inflation: 1 % of the box's extent plus a relative term on its coordinates, then one ulp outward.
// Monotone: a box that contains another (and so has at least its extent and magnitude) inflates to a
// box that contains the other's inflation.
__host__ __device__ inline Box inflate(Box b) {
    float ext = 0.0f, mag = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float e = b.hi[k] - b.lo[k];
        ext = ext < e ? e : ext;
        const float al = __builtin_fabsf(b.lo[k]), ah = __builtin_fabsf(b.hi[k]);
        const float m = al < ah ? ah : al;
        mag = mag < m ? m : mag;
    }
    const float d = 1e-2f * ext + 1e-5f * mag + 1e-6f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = next_down(b.lo[k] - d);
        b.hi[k] = next_up(b.hi[k] + d);
    }
    return b;
}

}  // namespace rrte
