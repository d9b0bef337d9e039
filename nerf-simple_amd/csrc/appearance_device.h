// appearance_device.h -- the per-image colour correction (appearance.hip, and the AFFINE term of
// composite_backward_device.h's LossHead): image m holds theta[m] = (a[3], b[3]) in fp32, and a ray of it sees
//
//     c'_k = (1 + a_k) c_k + b_k          k = r, g, b          (c: the compositor's rgb, before any clip)
//
// evaluated as fl(fl(fl(1 + a) c) + b): three separately rounded fp32 operations per channel, no fma (nerf_device.h
// add_rn / mul_rn), so torch's eager fp32 expression (1 + a) * c + b has the same bits.  Its backward, each one rounded product:
//
//     g_c = g fl(1 + a),   g_a = g c,   g_b = g
//
// One copy: the stages and the training head include this header and so form the same bits.  A ray whose global id lies
// outside [0, M HW) has a row of NaN (nan_row): its colour and everything behind it is NaN, and no image receives it.
#pragma once
#include "nerf_device.h"          // mul_rn / add_rn: one operation, one rounding, never contracted

namespace nerf_appearance {

struct Row { float a[3], b[3]; };

// six floats, 8-byte aligned (a [*,6] fp32 table, or one row for every ray)
__device__ __forceinline__ Row load_row(const float* p) {
    const float2* q = reinterpret_cast<const float2*>(p);
    const float2 v0 = q[0], v1 = q[1], v2 = q[2];
    return Row{{v0.x, v0.y, v1.x}, {v1.y, v2.x, v2.y}};
}
__device__ __forceinline__ void store_row(float* p, const float* a, const float* b) {
    float2* q = reinterpret_cast<float2*>(p);
    q[0] = make_float2(a[0], a[1]);
    q[1] = make_float2(a[2], b[0]);
    q[2] = make_float2(b[1], b[2]);
}
__device__ __forceinline__ Row nan_row() {
    const float n = __builtin_nanf("");
    return Row{{n, n, n}, {n, n, n}};
}

// gain[k] = fl(1 + a_k): what the forward multiplies by and the backward hands to g_c
__device__ __forceinline__ void gains(const Row& r, float* gain) {
#pragma unroll
    for (int k = 0; k < 3; ++k) gain[k] = add_rn(1.0f, r.a[k]);
}
__device__ __forceinline__ float apply(float gain, float c, float b) { return add_rn(mul_rn(gain, c), b); }

// g [3] = d loss / d c', c [3] the uncorrected colour -> g_c [3] and the ray's row of d loss / d theta = (g c, g)
__device__ __forceinline__ void apply_backward(const float* g, const float* c, const float* gain, float* g_c, float* g_a) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g_c[k] = mul_rn(g[k], gain[k]);
        g_a[k] = mul_rn(g[k], c[k]);
    }
}

}  // namespace nerf_appearance
