// occupancy_graph.hip -- the two light passes of the GRAPHED masked training step (include/nerf_amd.h, "graphed masked
// training step").  A captured step has no host in it, so the live count P' of a batch cannot size
// anything: the network kernels run on a fixed capacity of C points, and these two kernels make the rows beyond
// min(P', C) inert.  Not in the reference.
//
//   occ_emit_capped_kernel -- pts[C, 6]: row r < min(P', C) is the row nerf_amd_occupancy_points writes (one wavefront per
//       ray, the same fetch_point_rays), every row behind is the pad point; counts = {P', min(P', C)}.  P' = offsets[B] is
//       read from device memory.  Every row of pts is written by exactly one lane on every launch.
//   occ_head_capped_kernel -- masked compositor forward -> g_rgb = 2 (rgb - gt) / (3 B) -> masked compositor backward in one
//       launch, under the capacity clamp: sample i of ray b is KEPT iff its mask bit is set and offsets[b] + (set bits of the
//       ray below i) < C.  The walk is occ_composite_backward_kernel's (occupancy_train.hip), restated here with the forward
//       compositor's rgb sums (composite_device.h) beside it, as composite.hip's training head carries them; that file and
//       this one share no code but the headers.  d_raw_live[C, 4]: kept rows from the sweep, rows behind min(P', C) zero.
//
// No atomics; the kept rows and the pad rows are disjoint ranges, so no two lanes write one address and two runs write the
// same bytes.  The host wrappers below are the C ABI themselves (argument checking included): api.hip is not involved.
#include "composite_device.h"
#include "../../include/nerf_amd.h"

namespace {

constexpr int OCCG_RAYS_PER_BLOCK = 4;
constexpr int OCCG_THREADS = 64 * OCCG_RAYS_PER_BLOCK;
constexpr int OCCG_MAX_CHUNKS = 8;             // N <= 512: the masked compositor backward's limit
constexpr int OCCG_MAX_N = 64 * OCCG_MAX_CHUNKS;
constexpr long long OCCG_MAX_RAYS = 1ll << 32;

__device__ __forceinline__ void occg_wave_lds_fence() {
    __builtin_amdgcn_s_waitcnt(0xc07f);        // lgkmcnt(0): this wave's LDS writes are done
    __builtin_amdgcn_wave_barrier();
}

// composite.hip's wave_suffix_excl: inclusive suffix sum, then shift down by one lane
__device__ __forceinline__ float occg_wave_suffix_excl(float v, int lane, float& total) {
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

__device__ __forceinline__ long long occg_min(long long a, long long b) { return a < b ? a : b; }

// ---- capped emit ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OCCG_THREADS) void occ_emit_capped_kernel(MlpArgs a, const unsigned long long* __restrict__ mask,
                                                                       const long long* __restrict__ offsets,
                                                                       float* __restrict__ pts, long long* __restrict__ counts,
                                                                       long long C, long long B) {
    const long long ray = (long long)blockIdx.x * OCCG_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long long total = offsets[B];
    const long long kept = occg_min(total, C);
    if (blockIdx.x == 0 && threadIdx.x == 0) { counts[0] = total; counts[1] = kept; }
    if (ray < B) {
        long long out = offsets[ray];
        // nothing live on this ray, or every live sample of it behind the capacity
        if (offsets[ray + 1] != out && out < C) {
            const int words = (a.N + 63) >> 6;
            for (int q = 0; q < words; ++q) {
                const unsigned long long m = mask[ray * words + q];
                const int i = q * 64 + lane;
                if (((m >> lane) & 1ull) && i < a.N) {
                    const long long row = out + __popcll(m & ((1ull << lane) - 1ull));
                    if (row >= 0 && row < C) {                 // the kept rows: global rank below the capacity
                        const PointIn pt = fetch_point_rays<true>(a, ray * a.N + i, RaySample{ray, i});
                        float* o = pts + row * 6;
                        o[0] = pt.x; o[1] = pt.y; o[2] = pt.z; o[3] = pt.d1; o[4] = pt.d2; o[5] = pt.d3;
                    }
                }
                out += __popcll(m);
            }
        }
    }
    // the surplus rows [kept, C): the pad point, grid-stride over their floats
    const float pad_point[6] = NERF_AMD_OCCUPANCY_PAD_POINT;
    const long long n_pad = (C - kept) * 6;
    float* pad = pts + kept * 6;
    for (long long e = (long long)blockIdx.x * OCCG_THREADS + threadIdx.x; e < n_pad; e += (long long)gridDim.x * OCCG_THREADS)
        pad[e] = pad_point[e % 6];
}

// ---- fused masked head ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OCCG_THREADS) void occ_head_capped_kernel(
    MlpArgs a, const unsigned long long* __restrict__ mask, const long long* __restrict__ offsets,
    const float* __restrict__ raw_live, const float* __restrict__ gt, float* __restrict__ rgb_out,
    float* __restrict__ d_raw_live, long long C, long long B, float mse_scale) {
    constexpr int CHUNKS = OCCG_MAX_CHUNKS;
    __shared__ float s_t[OCCG_RAYS_PER_BLOCK][OCCG_MAX_N];
    const int wv = threadIdx.x >> 6;
    const long long ray = (long long)blockIdx.x * OCCG_RAYS_PER_BLOCK + wv;
    const int lane = threadIdx.x & 63;
    const int N = a.N;
    // the surplus rows [min(P', C), C) of d_raw_live: exact zeros, grid-stride (no wave depends on another's rows)
    {
        const long long kept = occg_min(offsets[B], C);
        f32x4* pad = reinterpret_cast<f32x4*>(d_raw_live) + kept;
        for (long long r = (long long)blockIdx.x * OCCG_THREADS + threadIdx.x; r < C - kept; r += (long long)gridDim.x * OCCG_THREADS)
            pad[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (ray >= B) return;                      // whole wave leaves together; no workgroup barrier below
    const long long first = occg_min(offsets[ray], C);
    const long long n_kept = occg_min(offsets[ray + 1], C) - first;
    const unsigned long long* m = mask + ray * ((N + 63) >> 6);
    const f32x4* rraw = reinterpret_cast<const f32x4*>(raw_live) + first;
    f32x4* rout = reinterpret_cast<f32x4*>(d_raw_live) + first;
    if (N == 1 || n_kept <= 0) {
        // N == 1: the reference composites an EMPTY sample axis (composite_device.h), no output depends on raw.  Nothing
        // kept: every sample is (0, 0, 0, -inf), w = 0 throughout.  Either way rgb = 0 and a kept row (N == 1) gets zeros.
        if (lane == 0) {
            rgb_out[ray * 3 + 0] = 0.f; rgb_out[ray * 3 + 1] = 0.f; rgb_out[ray * 3 + 2] = 0.f;
            if (n_kept > 0 && (m[0] & 1ull)) rout[0] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        return;
    }
    for (int i = lane; i < N; i += 64) s_t[wv][i] = fetch_point_rays<false>(a, ray * N + i, RaySample{ray, i}).t;
    occg_wave_lds_fence();
    const float* rts = s_t[wv];
    const float* d = a.rays + ray * 6 + 3;
    float d0 = d[0], d1 = d[1], d2 = d[2];
    {
        const float n = norm3(d0, d1, d2);
        d0 = __fdiv_rn(d0, n); d1 = __fdiv_rn(d1, n); d2 = __fdiv_rn(d2, n);
    }
    const float dnorm = norm3(d0, d1, d2);

    // forward sweep: per chunk keep alpha, T, fac, delta*softplus' and the colour; rk = the row of a kept sample, -1 dead
    float al[CHUNKS], Tt[CHUNKS], fc[CHUNKS], ds[CHUNKS], tt[CHUNKS];
    f32x4 cc[CHUNKS];
    int rk[CHUNKS];
    float carry = 1.0f;
    float sr = 0.f, sg = 0.f, sb = 0.f;        // the forward compositor's rgb, for the loss gradient
    long long before = 0;                      // set mask bits of this ray in earlier chunks
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
                const bool live = ((mw >> lane) & 1ull) && rank < n_kept;
                if (live) rk[ch] = (int)rank;
                const float t = rts[i];
                const f32x4 c = live ? rraw[rank] : f32x4{0.f, 0.f, 0.f, -__builtin_inff()};
                float delta = (i == N - 1) ? 1e10f : sub_rn(rts[i + 1], t);
                delta = mul_rn(delta, dnorm);
                const float sigma = c[3];
                const float z = expf(sigma);
                const float sp = sigma > 20.f ? sigma : log1pf(z);
                // softplus' as torch's backward forms it (composite.hip): z / (z + 1)
                const float spd = sigma > 20.f ? 1.0f : z / (z + 1.0f);
                const float e = expf(mul_rn(-sp, delta));
                a_ = sub_rn(1.0f, e);
                fac = add_rn(sub_rn(1.0f, a_), 1e-10f);
                ds[ch] = e * delta * spd;      // d alpha / d sigma, from e itself
                tt[ch] = t; cc[ch] = c;
            }
            before += __popcll(mw);
            // the forward compositor's scan (composite_device.h): same tree, same rounded products
            const float incl = nerf_composite::wave_scan_mul(fac);
            const float excl = nerf_composite::dpp_move<0x138, 0xf>(1.0f, incl);          // wave_shr:1
            al[ch] = a_; fc[ch] = fac; Tt[ch] = mul_rn(carry, excl);
            carry = mul_rn(carry, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(incl), 63)));
            if (valid) {
                // the same ops as the forward compositor (composite_device.h), so rgb_out equals its rgb
                const float wt = mul_rn(a_, Tt[ch]);
                sr = __fmaf_rn(wt, cc[ch][0], sr); sg = __fmaf_rn(wt, cc[ch][1], sg); sb = __fmaf_rn(wt, cc[ch][2], sb);
            }
        }
    }
    // loss = MSELoss(rgb, gt) (train.py:52): d loss / d rgb = 2 (rgb - gt) / (3 B), formed here as the dense head forms it
    sr = nerf_composite::wave_total(sr); sg = nerf_composite::wave_total(sg); sb = nerf_composite::wave_total(sb);
    const float gr = 2.0f * (sr - gt[ray * 3 + 0]) * mse_scale;
    const float gg = 2.0f * (sg - gt[ray * 3 + 1]) * mse_scale;
    const float gb = 2.0f * (sb - gt[ray * 3 + 2]) * mse_scale;
    if (lane == 0) { rgb_out[ray * 3 + 0] = sr; rgb_out[ray * 3 + 1] = sg; rgb_out[ray * 3 + 2] = sb; }

    // backward sweep over chunks, carrying sum_{k in later chunks} G_k w_k (only rgb feeds the loss)
    float later = 0.f;
#pragma unroll
    for (int ch = CHUNKS - 1; ch >= 0; --ch) {
        const int base = ch * 64;
        if (base < N) {
            const int i = base + lane;
            const bool valid = i < N;
            const float w = al[ch] * Tt[ch];
            float G = 0.f;
            if (valid) G = gr * cc[ch][0] + gg * cc[ch][1] + gb * cc[ch][2];
            float tot;
            const float suffix = occg_wave_suffix_excl(valid ? G * w : 0.f, lane, tot) + later;
            later += tot;
            if (valid && rk[ch] >= 0) {
                const float dalpha = G * Tt[ch] - suffix / fc[ch];
                const f32x4 o = {w * gr, w * gg, w * gb, dalpha * ds[ch]};
                rout[rk[ch]] = o;
            }
        }
    }
}

// the jitter arguments of every rays-mode entry point (api.hip's rule, restated): explicit u / ts, the counter RNG, or the
// counter RNG with its seed offset in device memory (then `u` is that address)
inline bool occg_bad_jitter(uint32_t flags, const float* u, const float* tbins) {
    if (flags & ~(NERF_AMD_TS_GIVEN | NERF_AMD_DEVICE_RNG | NERF_AMD_SEED_IN_MEMORY)) return true;
    if (flags & NERF_AMD_SEED_IN_MEMORY) {
        if (!(flags & NERF_AMD_DEVICE_RNG) || (flags & NERF_AMD_TS_GIVEN) || !u) return true;
        if (reinterpret_cast<uintptr_t>(u) & 7) return true;
    } else if (!(flags & NERF_AMD_DEVICE_RNG) && !u) {
        return true;
    }
    return !(flags & NERF_AMD_TS_GIVEN) && !tbins;
}

// what both entry points share: 0 = go on, otherwise the code to return.  1 <= C <= B N, so B >= 1.
int occg_check(const float* rays, const float* u, const float* tbins, uint32_t flags, const uint64_t* mask, const int64_t* offsets,
               int64_t C, int64_t B, int N) {
    if (B < 0 || N <= 0 || C < 1) return NERF_AMD_EINVAL;
    if (occg_bad_jitter(flags, u, tbins)) return NERF_AMD_EINVAL;
    if (N > OCCG_MAX_N || B > OCCG_MAX_RAYS) return NERF_AMD_EUNSUP;
    if (C > B * (int64_t)N) return NERF_AMD_EINVAL;
    if (!rays || !mask || !offsets || ((uintptr_t)mask & 7) || ((uintptr_t)offsets & 7)) return NERF_AMD_EINVAL;
    return 0;
}

MlpArgs occg_args(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed, int64_t ray_id0, int64_t B,
                  int N) {
    MlpArgs a{};
    a.rays = rays; a.u = u; a.tbins = tbins;
    a.P = B * (int64_t)N; a.N = N; a.flags = flags; a.seed = seed; a.ray_id0 = ray_id0;
    return a;
}

}  // namespace

extern "C" int nerf_amd_occupancy_points_capped(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed,
                                                int64_t ray_id0, const uint64_t* mask, const int64_t* offsets, float* pts,
                                                int64_t* counts, int64_t capacity, int64_t B, int N, void* stream) {
    const int rc = occg_check(rays, u, tbins, flags, mask, offsets, capacity, B, N);
    if (rc) return rc;
    if (!pts || !counts || ((uintptr_t)pts & 3) || ((uintptr_t)counts & 7)) return NERF_AMD_EINVAL;
    (void)hipGetLastError();
    const MlpArgs a = occg_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    const long long blocks = (B + OCCG_RAYS_PER_BLOCK - 1) / OCCG_RAYS_PER_BLOCK;
    hipLaunchKernelGGL(occ_emit_capped_kernel, dim3((unsigned)blocks), dim3(OCCG_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a,
                       reinterpret_cast<const unsigned long long*>(mask), reinterpret_cast<const long long*>(offsets), pts,
                       reinterpret_cast<long long*>(counts), (long long)capacity, (long long)B);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_volume_render_masked_mse_backward(const float* raw_live, const float* rays, const float* u, const float* tbins,
                                                          uint32_t flags, uint64_t seed, int64_t ray_id0, const uint64_t* mask,
                                                          const int64_t* offsets, const float* gt, float* rgb, float* d_raw_live,
                                                          int64_t capacity, int64_t B, int N, void* stream) {
    const int rc = occg_check(rays, u, tbins, flags, mask, offsets, capacity, B, N);
    if (rc) return rc;
    if (!raw_live || !gt || !rgb || !d_raw_live || ((uintptr_t)raw_live & 15) || ((uintptr_t)d_raw_live & 15) ||
        ((uintptr_t)gt & 3) || ((uintptr_t)rgb & 3))
        return NERF_AMD_EINVAL;
    (void)hipGetLastError();
    const MlpArgs a = occg_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    const long long blocks = (B + OCCG_RAYS_PER_BLOCK - 1) / OCCG_RAYS_PER_BLOCK;
    hipLaunchKernelGGL(occ_head_capped_kernel, dim3((unsigned)blocks), dim3(OCCG_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a,
                       reinterpret_cast<const unsigned long long*>(mask), reinterpret_cast<const long long*>(offsets), raw_live, gt, rgb,
                       d_raw_live, (long long)capacity, (long long)B, 1.0f / (3.0f * (float)B));
    return (int)hipGetLastError();
}
