// occupancy_train.hip -- training with empty-space skipping: the backward of the masked compositor and the running density
// volume a training occupancy grid is refreshed from.  Not in the reference.
//
//   occ_composite_backward_kernel -- d loss / d raw_live[P', 4] of nerf_amd_volume_render_masked.  One wavefront per ray,
//       lane = ORIGINAL sample index, N walked in chunks of 64 exactly as composite_backward_kernel (composite.hip) walks the
//       dense raw[B, N, 4]: positions recomputed (fetch_point_rays) into the wave's LDS slice, the network's output read at
//       offsets[ray] + rank for a live sample -- rank from popcounts of the mask words -- and (0, 0, 0, -inf) for a dead one.
//       A dead sample has softplus' = 0, alpha = 0 and w = 0 there: it receives nothing and adds exact zeros to the suffix
//       sums.  The sweep's expressions are those of composite.hip, restated here (that file is not edited): the result is
//       the rows at the live samples of the dense backward on the overwritten raw.  No atomics: row offsets[ray] + rank is
//       written by exactly one lane.
//   occ_decay_max_kernel -- state = max(fl(state decay), softplus(sigma_now)), softplus as the compositor's.
#include "composite_device.h"

namespace {

constexpr int OCCT_RAYS_PER_BLOCK = 4;
constexpr int OCCT_MAX_CHUNKS = 8;             // N <= 512, the dense backward's limit
constexpr int OCCT_MAX_N = 64 * OCCT_MAX_CHUNKS;

__device__ __forceinline__ void occt_wave_lds_fence() {
    __builtin_amdgcn_s_waitcnt(0xc07f);        // lgkmcnt(0): this wave's LDS writes are done
    __builtin_amdgcn_wave_barrier();
}

// composite.hip's wave_suffix_excl: inclusive suffix sum, then shift down by one lane
__device__ __forceinline__ float occt_wave_suffix_excl(float v, int lane, float& total) {
    float incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float dn = __shfl_down(incl, off);
        if (lane + off < 64) incl += dn;
    }
    total = __shfl(incl, 0);
    float ex = __shfl_down(incl, 1);
    if (lane == 63) ex = 0.f;
    return ex;
}

__global__ __launch_bounds__(64 * OCCT_RAYS_PER_BLOCK) void occ_composite_backward_kernel(
    MlpArgs a, const unsigned long long* __restrict__ mask, const long long* __restrict__ offsets,
    const float* __restrict__ raw_live, const float* __restrict__ g_rgb, const float* __restrict__ g_disp,
    const float* __restrict__ g_alpha, const float* __restrict__ g_acc, const float* __restrict__ g_w,
    float* __restrict__ d_raw_live, long long B) {
    constexpr int CHUNKS = OCCT_MAX_CHUNKS;
    __shared__ float s_t[OCCT_RAYS_PER_BLOCK][OCCT_MAX_N];
    const int wv = threadIdx.x >> 6;
    const long long ray = (long long)blockIdx.x * OCCT_RAYS_PER_BLOCK + wv;
    if (ray >= B) return;                      // whole wave leaves together; no workgroup barrier below
    const int lane = threadIdx.x & 63;
    const int N = a.N;
    const long long first = offsets[ray];
    const long long n_live = offsets[ray + 1] - first;
    if (n_live <= 0 || !raw_live) return;      // a ray with no live sample writes nothing (NULL buffers: P' = 0 only)
    const unsigned long long* m = mask + ray * ((N + 63) >> 6);
    const f32x4* rraw = reinterpret_cast<const f32x4*>(raw_live) + first;
    f32x4* rout = reinterpret_cast<f32x4*>(d_raw_live) + first;
    if (N == 1) {
        // the reference composites an EMPTY sample axis at N == 1 (composite_device.h): no output depends on raw
        if (lane == 0 && (m[0] & 1ull)) rout[0] = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    for (int i = lane; i < N; i += 64) s_t[wv][i] = fetch_point_rays<false>(a, ray * N + i, RaySample{ray, i}).t;
    occt_wave_lds_fence();
    const float* rts = s_t[wv];
    const float* d = a.rays + ray * 6 + 3;
    float d0 = d[0], d1 = d[1], d2 = d[2];
    {
        const float n = norm3(d0, d1, d2);
        d0 = __fdiv_rn(d0, n); d1 = __fdiv_rn(d1, n); d2 = __fdiv_rn(d2, n);
    }
    const float dnorm = norm3(d0, d1, d2);

    // forward sweep: per chunk keep alpha, T, fac, delta*softplus' and the colour; rk = the row of a live sample, -1 dead
    float al[CHUNKS], Tt[CHUNKS], fc[CHUNKS], ds[CHUNKS], tt[CHUNKS];
    f32x4 cc[CHUNKS];
    int rk[CHUNKS];
    float carry = 1.0f, depth = 0.f, accw = 0.f;
    long long before = 0;                      // live samples of this ray in earlier chunks
#pragma unroll
    for (int ch = 0; ch < CHUNKS; ++ch) {
        const int base = ch * 64;
        al[ch] = 0.f; Tt[ch] = 0.f; fc[ch] = 1.f; ds[ch] = 0.f; tt[ch] = 0.f;
        cc[ch] = f32x4{0.f, 0.f, 0.f, 0.f};
        rk[ch] = -1;
        if (base < N) {
            const int i = base + lane;
            const bool valid = i < N;
            const unsigned long long mw = m[ch];
            float a_ = 0.f, fac = 1.0f;
            if (valid) {
                const long long rank = before + __popcll(mw & ((1ull << lane) - 1ull));
                const bool live = ((mw >> lane) & 1ull) && rank < n_live;
                if (live) rk[ch] = (int)rank;
                const float t = rts[i];
                const f32x4 c = live ? rraw[rank] : f32x4{0.f, 0.f, 0.f, -__builtin_inff()};
                float delta = (i == N - 1) ? 1e10f : sub_rn(rts[i + 1], t);
                delta = mul_rn(delta, dnorm);
                const float sigma = c[3];
                const float z = expf(sigma);
                const float sp = sigma > 20.f ? sigma : log1pf(z);
                // softplus' as torch's backward forms it: z / (z + 1) keeps exp(sigma) down to the subnormals, where
                // 1 / (1 + exp(-sigma)) is 0 from sigma = -88.7 on (a last sample's delta = 1e10 brings that back up)
                const float spd = sigma > 20.f ? 1.0f : z / (z + 1.0f);
                const float e = expf(mul_rn(-sp, delta));
                a_ = sub_rn(1.0f, e);
                fac = add_rn(sub_rn(1.0f, a_), 1e-10f);
                // e itself, not 1 - alpha: that recovers e to an absolute 2^-24, a relative 2^-24 / e on a nearly opaque sample
                ds[ch] = e * delta * spd;      // d alpha / d sigma
                tt[ch] = t; cc[ch] = c;
            }
            before += __popcll(mw);
            // the forward compositor's scan (composite_device.h): same tree, same rounded products
            const float incl = nerf_composite::wave_scan_mul(fac);
            const float excl = nerf_composite::dpp_move<0x138, 0xf>(1.0f, incl);          // wave_shr:1
            al[ch] = a_; fc[ch] = fac; Tt[ch] = mul_rn(carry, excl);
            carry = mul_rn(carry, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(incl), 63)));
            if (valid) { depth += a_ * Tt[ch] * tt[ch]; accw += a_ * Tt[ch]; }
        }
    }
    depth = nerf_composite::wave_sum(depth); accw = nerf_composite::wave_sum(accw);

    // upstream gradients that reach every w_i of the ray
    const float gr = g_rgb ? g_rgb[ray * 3 + 0] : 0.f, gg = g_rgb ? g_rgb[ray * 3 + 1] : 0.f,
                gb = g_rgb ? g_rgb[ray * 3 + 2] : 0.f;
    float gdep = 0.f, gac = g_acc ? g_acc[ray] : 0.f;
    if (g_disp) {
        const float q = depth / accw;
        if (q > 1e-10f) {                        // disp = 1/q there; the clamp branch has zero slope
            const float dq = -g_disp[ray] / (q * q);
            gdep = dq / accw;
            gac += -dq * depth / (accw * accw);
        }
    }
    // backward sweep over chunks, carrying sum_{k in later chunks} G_k w_k
    float later = 0.f;
#pragma unroll
    for (int ch = CHUNKS - 1; ch >= 0; --ch) {
        const int base = ch * 64;
        if (base < N) {
            const int i = base + lane;
            const bool valid = i < N;
            const float w = al[ch] * Tt[ch];
            float G = 0.f;
            if (valid) {
                G = gr * cc[ch][0] + gg * cc[ch][1] + gb * cc[ch][2] + gdep * tt[ch] + gac;
                if (g_w) G += g_w[ray * N + i];
            }
            float tot;
            const float suffix = occt_wave_suffix_excl(valid ? G * w : 0.f, lane, tot) + later;
            later += tot;
            if (valid && rk[ch] >= 0) {
                float dalpha = G * Tt[ch] - suffix / fc[ch];
                if (g_alpha) dalpha += g_alpha[ray * N + i];
                const f32x4 o = {w * gr, w * gg, w * gb, dalpha * ds[ch]};
                rout[rk[ch]] = o;
            }
        }
    }
}

__global__ __launch_bounds__(256) void occ_decay_max_kernel(float* __restrict__ state, const float* __restrict__ sigma_now,
                                                            float decay, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float s = sigma_now[i];
        const float sp = s > 20.f ? s : log1pf(expf(s));      // the compositor's softplus (beta = 1, identity above 20)
        const float dcy = mul_rn(state[i], decay);
        // the maximum that keeps a NaN of either side (a NaN state is live in nerf_amd_occupancy_from_density)
        state[i] = (dcy != dcy) ? dcy : (sp != sp) ? sp : (dcy > sp ? dcy : sp);
    }
}

}  // namespace

extern "C" int nerf_amd_occ_train_max_n(void) { return OCCT_MAX_N; }

extern "C" int nerf_amd_launch_occ_composite_backward(const MlpArgs* args, const unsigned long long* mask, const long long* offsets,
                                                      const float* raw_live, const float* g_rgb, const float* g_disp,
                                                      const float* g_alpha, const float* g_acc, const float* g_w,
                                                      float* d_raw_live, long long B, hipStream_t stream) {
    (void)hipGetLastError();
    if (B == 0) return 0;
    if (args->N > OCCT_MAX_N) return -2;
    const long long blocks = (B + OCCT_RAYS_PER_BLOCK - 1) / OCCT_RAYS_PER_BLOCK;
    hipLaunchKernelGGL(occ_composite_backward_kernel, dim3((unsigned)blocks), dim3(64 * OCCT_RAYS_PER_BLOCK), 0, stream, *args, mask,
                       offsets, raw_live, g_rgb, g_disp, g_alpha, g_acc, g_w, d_raw_live, B);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_occ_decay_max(float* state, const float* sigma_now, float decay, long long n, hipStream_t stream) {
    (void)hipGetLastError();
    if (n == 0) return 0;
    long long blocks = (n + 255) / 256;
    if (blocks > 65536 * 16) blocks = 65536 * 16;
    hipLaunchKernelGGL(occ_decay_max_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, state, sigma_now, decay, n);
    return (int)hipGetLastError();
}
