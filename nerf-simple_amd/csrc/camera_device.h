// camera_device.h -- the per-pose routine of the camera optimiser (camera.hip): a stored pose [R0 | t0] and its learnable
// correction xi = (w, tau) -> the pose the rays are formed from,
//
//     R = exp([w]x) R0,   t = t0 + tau          (tests/input_grad_model.pose_rays)
//
// and the pixel's world direction in raygen.hip's operation order.  One copy: the rays kernel, its backward and the pose
// export call it and so see the same bits.
//
// exp([w]x) = I + a K + b K^2 (Rodrigues), with x = theta^2 = |w|^2 and K^2 = w w^T - x I taken entry by entry:
//     a = sin(theta) / theta,  b = 2 sin^2(theta / 2) / theta^2,  c = (theta - sin(theta)) / theta^3
// (c: the left Jacobian J = I + b K + c K^2 of the backward).  Below x < TAYLOR_BELOW = 1 the three come from their Taylor
// polynomials of degree 4 in x (the first dropped term is x^5 / 11! = 2.5e-8 for a, x^5 / 12! for b, x^5 / 13! for c:
// under half an fp32 ulp of the value up to x = 1), above from the closed forms -- where theta - sin(theta) has lost at
// most log2(6 / x) < 3 bits to cancellation.  Every step is an explicitly rounded operation (nerf_device.h mul_rn / add_rn /
// sub_rn, __fmaf_rn, __fdiv_rn) or a named library function (sqrtf, sinf): the compiler contracts and reorders nothing, so
// every kernel that includes this header forms the same bits.
//
// x == 0 (and a NULL xi) hands back the stored rotation itself, and tau == 0 the stored translation: the arithmetic
// would give equal values (a = 1, b = 1/2, K = 0), but not the sign of a stored zero.
#pragma once
#include "nerf_device.h"          // mul_rn / add_rn / sub_rn / sqrt_rn: one operation, one rounding, never contracted

namespace nerf_camera {

struct Pose { float r[9]; float t[3]; };

constexpr float TAYLOR_BELOW = 1.0f;         // on x = theta^2

__device__ inline float poly4(float x, float c0, float c1, float c2, float c3, float c4) {
    return __fmaf_rn(__fmaf_rn(__fmaf_rn(__fmaf_rn(c4, x, c3), x, c2), x, c1), x, c0);
}

__device__ inline void exp_coefficients(float x, float& a, float& b, float& c) {
    if (x < TAYLOR_BELOW) {
        a = poly4(x, 1.0f, -1.0f / 6, 1.0f / 120, -1.0f / 5040, 1.0f / 362880);
        b = poly4(x, 0.5f, -1.0f / 24, 1.0f / 720, -1.0f / 40320, 1.0f / 3628800);
        c = poly4(x, 1.0f / 6, -1.0f / 120, 1.0f / 5040, -1.0f / 362880, 1.0f / 39916800);
    } else {
        const float th = sqrt_rn(x), s = sinf(th), h = sinf(mul_rn(0.5f, th));
        a = __fdiv_rn(s, th);
        b = __fdiv_rn(mul_rn(2.0f, mul_rn(h, h)), x);
        c = __fdiv_rn(sub_rn(th, s), mul_rn(x, th));
    }
}

__device__ inline float norm2(const float* w) { return __fmaf_rn(w[2], w[2], __fmaf_rn(w[1], w[1], mul_rn(w[0], w[0]))); }

// pose12: row-major 3x4 [R0 | t0]; xi6 = (w, tau) or NULL
__device__ inline Pose corrected_pose(const float* __restrict__ pose12, const float* __restrict__ xi6) {
    Pose p;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.r[3 * r + c] = pose12[4 * r + c];
        p.t[r] = pose12[4 * r + 3];
    }
    if (!xi6) return p;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (xi6[3 + k] != 0.0f) p.t[k] = add_rn(p.t[k], xi6[3 + k]);
    const float w[3] = {xi6[0], xi6[1], xi6[2]};
    const float x = norm2(w);
    if (x == 0.0f) return p;
    float a, b, c;
    exp_coefficients(x, a, b, c);
    const float w01 = mul_rn(w[0], w[1]), w02 = mul_rn(w[0], w[2]), w12 = mul_rn(w[1], w[2]);
    const float aw0 = mul_rn(a, w[0]), aw1 = mul_rn(a, w[1]), aw2 = mul_rn(a, w[2]);
    const float q0 = mul_rn(w[0], w[0]), q1 = mul_rn(w[1], w[1]), q2 = mul_rn(w[2], w[2]);
    float e[9];
    e[0] = __fmaf_rn(-b, add_rn(q1, q2), 1.0f); e[1] = __fmaf_rn(b, w01, -aw2);                e[2] = __fmaf_rn(b, w02, aw1);
    e[3] = __fmaf_rn(b, w01, aw2);                 e[4] = __fmaf_rn(-b, add_rn(q0, q2), 1.0f); e[5] = __fmaf_rn(b, w12, -aw0);
    e[6] = __fmaf_rn(b, w02, -aw1);                e[7] = __fmaf_rn(b, w12, aw0);                 e[8] = __fmaf_rn(-b, add_rn(q0, q1), 1.0f);
    float r0[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r0[k] = p.r[k];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            p.r[3 * i + j] = __fmaf_rn(e[3 * i + 2], r0[6 + j], __fmaf_rn(e[3 * i + 1], r0[3 + j], mul_rn(e[3 * i], r0[j])));
    return p;
}

// the world direction of pixel (h, w): R dir_cam with dir_cam = ((w - W//2)/f, -(h - H//2)/f, -1), as raygen.hip forms it
__device__ inline void world_direction(const Pose& p, int H, int W, float f, int h, int w, float* y) {
    const float dx = __fdiv_rn((float)(w - W / 2), f);
    const float dy = -__fdiv_rn((float)(h - H / 2), f);
    const float dz = -1.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        y[k] = __fmaf_rn(p.r[3 * k + 2], dz, __fmaf_rn(p.r[3 * k + 1], dy, mul_rn(p.r[3 * k], dx)));
}

// u x v
__device__ inline void cross(const float* u, const float* v, float* o) {
    o[0] = __fmaf_rn(u[1], v[2], -mul_rn(u[2], v[1]));
    o[1] = __fmaf_rn(u[2], v[0], -mul_rn(u[0], v[2]));
    o[2] = __fmaf_rn(u[0], v[1], -mul_rn(u[1], v[0]));
}

// g_w = J^T s, J = I + b K + c K^2 the left Jacobian of exp at w: J^T s = s - b (w x s) + c (w x (w x s))
__device__ inline void left_jacobian_transposed(const float* w, const float* s, float* g) {
    const float x = norm2(w);
    float a, b, c;
    exp_coefficients(x, a, b, c);
    float ws[3], wws[3];
    cross(w, s, ws);
    cross(w, ws, wws);
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = __fmaf_rn(c, wws[k], __fmaf_rn(-b, ws[k], s[k]));
}

}  // namespace nerf_camera
