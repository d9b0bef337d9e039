// input_grad.hip -- gradients with respect to the network's INPUTS: the query points v [P,6] of Nerf.forward
// (reference utils/nets.py:34-43) and the rays [B,6] of render_nerf (utils/rendering.py:24-40), through the positional
// encoder (utils/xyz.py:6-36).  The parameter-gradient path (mlp_bwd_16.hip, dw_gemm.hip) stops at the pre-activation
// gradients of the layers that read the encoder outputs; the three steps that take those back to the inputs live here:
//
//   1. the products into the encoder features (bf16 MFMA, fp32 accumulate), on the dY the dX chain already wrote:
//        d posx [P,63] = dY0 . W0 + dY5 . W5[:, 256:319]        K = 512 (dY0 | dY5), 63 columns padded to 64
//        d posd [P,27] = dY9 . C0[:, 256:283]                   K = 128, 27 columns padded to 32
//   2. the encoder's Jacobian, in fp32 on the point recomputed in fp32 exactly as the forward formed it:
//        d/dx_c = d posx[c] + sum_i 2^i (cos(2^i x_c) g_sin[i,c] - sin(2^i x_c) g_cos[i,c])
//      (enc_jacobian_term below; the fp32 encoder backward uses the same function);
//   3. the reduction from samples to rays (x_n = o + t_n d, d_hat = d / |d|, t_n constant):
//        d_o = sum_n dx_n,   d_d = sum_n t_n dx_n + (g - d_hat (d_hat . g)) / |d|,   g = sum_n d(d_hat)_n.
//      The compositor also sees the direction, as deltas * |d_hat| (utils/rendering.py:37,43,56): |d_hat| == 1 for
//      every d, so that term's gradient is exactly zero and nothing of it is added here.
//
// Determinism: no atomics.  Every output element is written by one lane, every sum is taken in a fixed order (the
// MFMA k order, a fixed butterfly over the four lane groups, samples of a ray in index order), so two launches on the
// same inputs give identical bits.
#include "nerf_device.h"
#include "launchers.h"

using namespace nerf_layout;

namespace {

// ---- the encoder's Jacobian (shared by every kernel in this file) --------------------------------------------------
// d/dx of column (level, trig) of gamma(x) (trig 0: sin(2^level x), 1: cos(2^level x)) times that column's gradient.
// 2^level x is formed exactly (ldexpf), as the fp32 encoder (encode.hip enc_value) and the reference form it; the
// accurate ocml sinf / cosf: at level 9 one ulp of phase error is multiplied by 512 here.
__device__ __forceinline__ float enc_jacobian_term(float x, int level, int trig, float g) {
    const float a = ldexpf(x, level);
    const float r = trig ? -sinf(a) : cosf(a);
    return ldexpf(r, level) * g;
}

// d gamma(x, L) -> dx for one scalar: g[2l + trig] at stride gs, summed in level order
__device__ __forceinline__ float gamma_backward_one(float x, const float* g, long long gs, int L) {
    float acc = 0.f;
    for (int l = 0; l < L; ++l) {
        acc += enc_jacobian_term(x, l, 0, g[(2 * l) * gs]);
        acc += enc_jacobian_term(x, l, 1, g[(2 * l + 1) * gs]);
    }
    return acc;
}

// ---- (b) fp32 encoder backward -------------------------------------------------------------------------------------
// gamma (utils/xyz.py:6-14) for a [n] column: d_out [n, 2L] -> d_x [n]
__global__ __launch_bounds__(256) void gamma_backward_kernel(const float* __restrict__ x, long long x_stride,
                                                             const float* __restrict__ d_out, float* __restrict__ d_x,
                                                             long long n, int L) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    d_x[i] = gamma_backward_one(x[i * x_stride], d_out + i * 2 * L, 1, L);
}

// positional_encoder (utils/xyz.py:16-36): d posx [P, 3+6Lp], d posd [P, 3+6Ld] -> d vec [P,6]; one thread per
// (point, coordinate): the raw column first, then the coordinate's 2L encoder columns in level order
__global__ __launch_bounds__(256) void posenc_backward_kernel(const float* __restrict__ vec, const float* __restrict__ d_posx,
                                                              const float* __restrict__ d_posd, float* __restrict__ d_vec,
                                                              long long P, int Lp, int Ld) {
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= P * 6) return;
    const long long p = e / 6;
    const int c = (int)(e - p * 6);
    const bool pos = c < 3;
    const int L = pos ? Lp : Ld, cc = pos ? c : c - 3, C = 3 + 6 * L;
    const float* g = (pos ? d_posx : d_posd) + p * C;
    d_vec[e] = g[cc] + gamma_backward_one(vec[e], g + 3 + 2 * L * cc, 1, L);
}

// ---- (c) samples -> rays -------------------------------------------------------------------------------------------
// d_q [B*N, 6] (gradient w.r.t. the query points [o + t d, d / |d|]) -> d_rays [B,6].  One thread per ray, samples in
// index order.  |d| and d_hat are recomputed exactly as fetch_point_rays forms them.
__global__ __launch_bounds__(256) void rays_reduce_kernel(const float* __restrict__ rays, const float* __restrict__ ts,
                                                          const float* __restrict__ d_q, float* __restrict__ d_rays,
                                                          long long B, int N) {
    const long long b = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (b >= B) return;
    float go[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f}, gu[3] = {0.f, 0.f, 0.f};
    const float* q = d_q + b * N * 6;
    const float* t = ts + b * N;
    for (int n = 0; n < N; ++n) {
        const f32x2 a = *reinterpret_cast<const f32x2*>(q + 6 * n);
        const f32x2 c = *reinterpret_cast<const f32x2*>(q + 6 * n + 2);
        const f32x2 e = *reinterpret_cast<const f32x2*>(q + 6 * n + 4);
        const float tn = t[n];
        const float dx[3] = {a.x, a.y, c.x}, du[3] = {c.y, e.x, e.y};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            go[k] += dx[k];
            gd[k] = __fmaf_rn(tn, dx[k], gd[k]);
            gu[k] += du[k];
        }
    }
    const float* r = rays + b * 6;
    const float dx = r[3], dy = r[4], dz = r[5];
    const float nrm = norm3(dx, dy, dz);
    const float u[3] = {__fdiv_rn(dx, nrm), __fdiv_rn(dy, nrm), __fdiv_rn(dz, nrm)};
    const float ug = u[0] * gu[0] + u[1] * gu[1] + u[2] * gu[2];
    float out[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out[k] = go[k];
        out[3 + k] = gd[k] + (gu[k] - u[k] * ug) / nrm;
    }
    f32x2* dst = reinterpret_cast<f32x2*>(d_rays + b * 6);
    dst[0] = f32x2{out[0], out[1]};
    dst[1] = f32x2{out[2], out[3]};
    dst[2] = f32x2{out[4], out[5]};
}

// ---- (a) bf16 input gradient of the fused network ------------------------------------------------------------------
// Transposed products, D[c][p] = sum_k Wt[c][k] dY[p][k]: the weight slices (A operand, rows = encoder columns c) sit in
// LDS as bf16 [c][k] images, dY (B operand, columns = points) comes straight from HBM -- lane (point l&15, group g) reads
// features 32s + 8g .. +7 of k-step s, one 16-byte granule of the point-blocked layout (nerf_layout.h), 256 contiguous
// bytes per quarter-wave.  The accumulator puts point l&15 on the lane and columns 4g .. 4g+3 of each 16-column tile
// in its registers: every lane applies the Jacobian to its 24 columns, four lane groups are summed by a fixed butterfly.
constexpr int IG_THREADS = 512;                    // 8 waves, each a 16-point group at a time
constexpr int IG_KX = 512, IG_KD = 128;            // K of the two products
constexpr int IG_RX = IG_KX * 2 + 16;              // bytes per LDS row: 16-byte pad -> rows c .. c+15 hit distinct slots
constexpr int IG_RD = IG_KD * 2 + 16;
constexpr int IG_LDS = 64 * IG_RX + 32 * IG_RD;    // 75,264 bytes: two workgroups per CU

struct InputGradArgs {
    const __bf16* dys;     // nerf_amd_mlp_backward's pre-activation gradients, P points
    const float* params;   // flat fp32 parameters (state_dict order)
    const float* pts;      // points mode [P,6], else NULL
    const float* rays;     // rays mode [B,6]
    const float* ts;       // rays mode [B,N]: the sample positions the forward used
    float* dv;             // out [P,6]
    long long P;
    int N;
};

__device__ __forceinline__ bf16x8 load_dy(const __bf16* dys, int L, long long p, int chunk, long long P) {
    const long long off = act_offset_bytes(L, P) + (p / ACT_TILE_PTS) * ACT_BLOCK_BYTES +
                          ((long long)chunk * ACT_TILE_PTS + p % ACT_TILE_PTS) * 16;
    return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(dys) + off);
}

__global__ __launch_bounds__(IG_THREADS) void input_grad_kernel(InputGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ig_lds[];
    char* wx = ig_lds;                     // [c 64][k 512] bf16: k < 256 W0[k][c], k >= 256 W5[k-256][256+c]
    char* wd = ig_lds + 64 * IG_RX;        // [c 32][k 128] bf16: C0[k][256+c]
    const int tid = threadIdx.x;
    // stage: one 16-byte LDS store per (column, 8 k's); consecutive threads read consecutive columns of a weight row
    for (int e = tid; e < 64 * (IG_KX / 8) + 32 * (IG_KD / 8); e += IG_THREADS) {
        const bool isx = e < 64 * (IG_KX / 8);
        const int e2 = isx ? e : e - 64 * (IG_KX / 8);
        const int nc = isx ? 64 : 32;
        const int c = e2 % nc, k8 = e2 / nc;
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * k8 + j;
            float w = 0.f;
            if (isx) {
                if (c < 63) w = k < 256 ? a.params[OFF_L0_W + k * 63 + c] : a.params[OFF_SKIP_W + (k - 256) * 319 + 256 + c];
            } else {
                if (c < 27) w = a.params[OFF_C0_W + k * 283 + 256 + c];
            }
            v[j] = (__bf16)w;             // round to nearest even, as the packers round (pack.hip)
        }
        char* dst = isx ? wx + c * IG_RX + k8 * 16 : wd + c * IG_RD + k8 * 16;
        *reinterpret_cast<bf16x8*>(dst) = v;
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, g = lane >> 4;
    MlpArgs ra{};
    ra.pts = a.pts; ra.rays = a.rays; ra.u = a.ts; ra.N = a.N; ra.flags = NERF_FLAG_TS_GIVEN; ra.P = a.P;
    const long long groups = (a.P + 15) / 16;
    for (long long grp = (long long)blockIdx.x * (IG_THREADS / 64) + wave; grp < groups;
         grp += (long long)gridDim.x * (IG_THREADS / 64)) {
        const long long p = grp * 16 + col;
        const bool live = p < a.P;
        // B fragments: 16 k-steps of dY0 | dY5 (chunks 4s + g of 32), 4 of dY9 (chunks 4s + g of 16)
        bf16x8 bx[16], bd[4];
        const bf16x8 zero = {};
#pragma unroll
        for (int s = 0; s < 16; ++s)
            bx[s] = live ? load_dy(a.dys, s < 8 ? 0 : 5, p, 4 * (s & 7) + g, a.P) : zero;
#pragma unroll
        for (int s = 0; s < 4; ++s) bd[s] = live ? load_dy(a.dys, 9, p, 4 * s + g, a.P) : zero;
        f32x4 ax[4] = {}, ad[2] = {};
#pragma unroll
        for (int s = 0; s < 16; ++s) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const bf16x8 w = *reinterpret_cast<const bf16x8*>(wx + (16 * m + col) * IG_RX + (32 * s + 8 * g) * 2);
                ax[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, bx[s], ax[m], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);      // keep the weight fragments of one k-step live at a time
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const bf16x8 w = *reinterpret_cast<const bf16x8*>(wd + (16 * m + col) * IG_RD + (32 * s + 8 * g) * 2);
                ad[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, bd[s], ad[m], 0, 0, 0);
            }
        // D layout (16x16x32): lane (col, g) holds rows 4g + i of each 16-row tile for point `col`
        // epilogue: the point in fp32, exactly as the forward formed it
        PointIn pt{};
        if (live) pt = a.pts ? fetch_point_pts(ra, p) : fetch_point_rays(ra, p);
        const float xs[3] = {pt.x, pt.y, pt.z}, ds[3] = {pt.d1, pt.d2, pt.d3};
        float gv[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = 16 * m + 4 * g + i;          // posx column [x,y,z, gamma(x), gamma(y), gamma(z)]
                const float gc = ax[m][i];
                if (c < 3) {
                    gv[c] += gc;
                } else if (c < 63) {
                    const int k = (c - 3) / 20, idx = (c - 3) % 20;
                    gv[k] += enc_jacobian_term(xs[k], idx >> 1, idx & 1, gc);
                }
            }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = 16 * m + 4 * g + i;          // posd column [d1,d2,d3, gamma(d1), gamma(d2), gamma(d3)]
                const float gc = ad[m][i];
                if (c < 3) {
                    gv[3 + c] += gc;
                } else if (c < 27) {
                    const int k = (c - 3) / 8, idx = (c - 3) % 8;
                    gv[3 + k] += enc_jacobian_term(ds[k], idx >> 1, idx & 1, gc);
                }
            }
        // the four lane groups of a point, in a fixed butterfly (every lane ends with the same bits)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            gv[k] += __shfl_xor(gv[k], 16);
            gv[k] += __shfl_xor(gv[k], 32);
        }
        if (live && g < 3) {
            const float lo = g == 0 ? gv[0] : g == 1 ? gv[2] : gv[4];
            const float hi = g == 0 ? gv[1] : g == 1 ? gv[3] : gv[5];
            *reinterpret_cast<f32x2*>(a.dv + p * 6 + 2 * g) = f32x2{lo, hi};
        }
    }
}

}  // namespace

extern "C" int nerf_amd_launch_input_gradients(const void* dys, const float* params, const float* pts, const float* rays,
                                               const float* ts, float* dv, float* d_rays, long long P, int N,
                                               hipStream_t stream) {
    (void)hipGetLastError();
    if (P == 0) return 0;
    InputGradArgs a{reinterpret_cast<const __bf16*>(dys), params, pts, rays, ts, dv, P, N};
    hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(input_grad_kernel), IG_LDS);
    if (e != hipSuccess) return (int)e;
    // two workgroups per CU (LDS), each stages the weights once and walks 16-point groups
    const long long groups = (P + 15) / 16, per_wg = IG_THREADS / 64;
    long long wg = (groups + per_wg - 1) / per_wg;
    const long long cap = 2LL * device_cus();
    if (wg > cap) wg = cap;
    hipLaunchKernelGGL(input_grad_kernel, dim3((unsigned)wg), dim3(IG_THREADS), IG_LDS, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess || !rays) return (int)e;
    const long long B = P / N;
    hipLaunchKernelGGL(rays_reduce_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, rays, ts, dv, d_rays, B, N);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_query_points_backward(const float* rays, const float* ts, const float* d_q, float* d_rays,
                                                     long long B, int N, hipStream_t stream) {
    (void)hipGetLastError();
    if (B == 0) return 0;
    hipLaunchKernelGGL(rays_reduce_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, rays, ts, d_q, d_rays, B, N);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_gamma_backward(const float* x, long long x_stride, const float* d_out, float* d_x, long long n,
                                              int L, hipStream_t stream) {
    (void)hipGetLastError();
    if (n == 0) return 0;
    hipLaunchKernelGGL(gamma_backward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, x_stride, d_out, d_x, n, L);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_posenc_backward(const float* vec, const float* d_posx, const float* d_posd, float* d_vec,
                                               long long P, int Lp, int Ld, hipStream_t stream) {
    (void)hipGetLastError();
    if (P == 0) return 0;
    hipLaunchKernelGGL(posenc_backward_kernel, dim3((unsigned)((P * 6 + 255) / 256)), dim3(256), 0, stream, vec, d_posx, d_posd,
                       d_vec, P, Lp, Ld);
    return (int)hipGetLastError();
}
