// composite_dist_device.h -- mip-NeRF 360's distortion loss of ONE ray's weights and its gradient to them, shared by
// nerf_amd_distortion_loss (composite_dist.hip: t and w read from HBM) and the training head behind it
// (composite_backward_ray with a LossHead<.., DIST, ..>: w straight from the forward sweep's registers).  With
//   delta_i = t_{i+1} - t_i (i < N - 1), delta_{N-1} = max(t_far - t_{N-1}, 0), m_i = t_i + delta_i / 2
//   D        = 2 sum_i w_i sum_{j<i} w_j (m_i - m_j) + (1/3) sum_i w_i^2 delta_i
//   dD/dw_i  = 2 [ sum_{j<i} w_j (m_i - m_j) + sum_{j>i} w_j (m_j - m_i) ] + (2/3) w_i delta_i
// the ordered form of sum_ij w_i w_j |m_i - m_j| (equal to it on nondecreasing positions, which nothing checks).  O(N) per
// ray through four running sums, P_i = sum_{j<i} w_j, Q_i = sum_{j<i} w_j m_j and the suffix sums S_i, R_i over j > i:
//   dD/dw_i  = 2 [(m_i P_i - Q_i) + (R_i - m_i S_i)] + (2/3) w_i delta_i
//   D        = sum_i w_i 2 (m_i P_i - Q_i) + (1/3) sum_i w_i^2 delta_i
// The midpoints are centred on the ray first (m_i - t_0: D depends on differences only, and the products w m lose fewer bits).
// ONE wavefront per ray, one sample per lane, chunks of 64 walked forward once (prefix sums, carries between chunks) and
// backward once (suffix sums); no atomics, no LDS, nothing crosses a wave.  Every floating-point operation is one explicitly
// rounded op, as in composite_backward_device.h, so both callers write the same bits from the same t and w.
#pragma once
#include "composite_device.h"

namespace nerf_composite {

// inclusive sum scan over the 64 lanes: wave_scan_mul's tree with adds
__device__ __forceinline__ float wave_scan_add(float x) {
    x = add_rn(x, dpp_move<0x111, 0xf>(0.f, x));      // row_shr:1
    x = add_rn(x, dpp_move<0x112, 0xf>(0.f, x));      // row_shr:2
    x = add_rn(x, dpp_move<0x114, 0xf>(0.f, x));      // row_shr:4
    x = add_rn(x, dpp_move<0x118, 0xf>(0.f, x));      // row_shr:8
    x = add_rn(x, dpp_move<0x142, 0xa>(0.f, x));      // row_bcast:15 -> rows 1, 3
    x = add_rn(x, dpp_move<0x143, 0xc>(0.f, x));      // row_bcast:31 -> rows 2, 3
    return x;
}

// sample i = 64 ch + lane of the ray: its interval delta and its centred midpoint.  t[ch] holds t_i per lane (anything at
// i >= N); t_{i+1} comes from the next lane, or from lane 0 of the next chunk.
template <int CHUNKS>
__device__ __forceinline__ void distortion_interval(const float (&t)[CHUNKS], int ch, int lane, int N, float t_far, float t0,
                                                    float& delta, float& m) {
    const int i = ch * 64 + lane;
    float t_next = __shfl_down(t[ch], 1);
    if (ch + 1 < CHUNKS) {
        const float first = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t[ch + 1 < CHUNKS ? ch + 1 : ch]), 0));
        if (lane == 63) t_next = first;
    }
    delta = (i == N - 1) ? fmaxf(sub_rn(t_far, t[ch]), 0.f) : sub_rn(t_next, t[ch]);
    m = add_rn(sub_rn(t[ch], t0), mul_rn(0.5f, delta));
}

// t[ch], w[ch]: the ray's positions and weights, chunk by chunk; w MUST be 0 at i >= N.  2 <= N <= 64 CHUNKS.
// gw[ch] = coef dD/dw_i (0 at i >= N); returns coef D as a wave-uniform value.
template <int CHUNKS>
__device__ __forceinline__ float distortion_ray(const float (&t)[CHUNKS], const float (&w)[CHUNKS], int N, int lane,
                                                float t_far, float coef, float (&gw)[CHUNKS]) {
    const float t0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t[0]), 0));
    // forward sweep: a_i = m_i P_i - Q_i per chunk, and the loss terms
    float a[CHUNKS];
    float cp = 0.f, cq = 0.f, acc = 0.f;
#pragma unroll
    for (int ch = 0; ch < CHUNKS; ++ch) {
        a[ch] = 0.f; gw[ch] = 0.f;
        if (ch * 64 < N) {
            const bool valid = ch * 64 + lane < N;
            float delta, m;
            distortion_interval<CHUNKS>(t, ch, lane, N, t_far, t0, delta, m);
            const float wi = w[ch];
            const float wm = valid ? mul_rn(wi, m) : 0.f;
            const float ip = wave_scan_add(wi), iq = wave_scan_add(wm);
            const float P = add_rn(cp, dpp_move<0x138, 0xf>(0.f, ip));            // wave_shr:1 = the exclusive sum
            const float Q = add_rn(cq, dpp_move<0x138, 0xf>(0.f, iq));
            cp = add_rn(cp, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ip), 63)));
            cq = add_rn(cq, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(iq), 63)));
            if (valid) {
                a[ch] = sub_rn(mul_rn(m, P), Q);
                const float self = mul_rn(mul_rn(0.333333343f, mul_rn(wi, wi)), delta);
                acc = add_rn(acc, add_rn(mul_rn(wi, mul_rn(2.0f, a[ch])), self));
            }
        }
    }
    // backward sweep: the suffix sums over j > i, carried from the later chunks
    float cs = 0.f, cr = 0.f;
#pragma unroll
    for (int ch = CHUNKS - 1; ch >= 0; --ch) {
        if (ch * 64 < N) {
            const bool valid = ch * 64 + lane < N;
            float delta, m;
            distortion_interval<CHUNKS>(t, ch, lane, N, t_far, t0, delta, m);
            const float wi = w[ch];
            const float wm = valid ? mul_rn(wi, m) : 0.f;
            float ts_, tr_;
            const float S = add_rn(wave_suffix_excl(wi, lane, ts_), cs);
            const float R = add_rn(wave_suffix_excl(wm, lane, tr_), cr);
            cs = add_rn(cs, ts_); cr = add_rn(cr, tr_);
            if (valid) {
                const float b = sub_rn(R, mul_rn(m, S));
                const float g = add_rn(mul_rn(2.0f, add_rn(a[ch], b)), mul_rn(mul_rn(0.666666687f, wi), delta));
                gw[ch] = mul_rn(coef, g);
            }
        }
    }
    return mul_rn(coef, wave_total(acc));
}

}  // namespace nerf_composite
