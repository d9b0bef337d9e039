// occupancy_hier.hip -- the masked COARSE head of the graphed masked hierarchical training step (include/nerf_amd.h,
// "masked hierarchical pair").  Not in the reference.
//
//   occ_head_capped_pdf_kernel<E> -- what occ_head_capped_kernel (occupancy_graph.hip) does under the capacity clamp -- masked
//       compositor forward -> g_rgb = 2 (rgb - gt) / (3 B) -> masked compositor backward -- and then, in the same wave, the
//       fine pass's sample placement (sample_pdf_device.h) from the weights of its own forward sweep, as composite.hip's
//       dense coarse head does it: wt = mul_rn(alpha, T) goes from registers to the wave's LDS slice beside the positions the
//       kernel has recomputed (a dead or over-capacity sample carries exactly 0), and the sampler reads both there after the
//       backward sweep.  w never reaches HBM.  The fine pass's mark depends on ts_out, so in a captured step both have to come
//       out of one node chain with no host in it; this is that node.
//
// Nc <= 256: four 64-lane chunks, E = keys per lane of the sampler's register sort (1, 2, 4, 8 by Nf).  One wavefront per
// ray, four rays per block; LDS per block 4 * (6 KB + 256 E B): 25 ... 32 KB, the dense head's figures (the positions live in
// the sampler's own ts[] slice, the mask walk is in registers).  No atomics; the kept rows and the pad rows are disjoint
// ranges, so two runs write the same bytes.  The host wrapper below is the C ABI itself: api.hip is not involved.
#include "composite_device.h"
#include "sample_pdf_device.h"
#include "../../include/nerf_amd.h"

namespace {

constexpr int OCCH_RAYS_PER_BLOCK = 4;
constexpr int OCCH_THREADS = 64 * OCCH_RAYS_PER_BLOCK;
constexpr int OCCH_CHUNKS = nerf_pdf::MAXC / 64;
constexpr long long OCCH_MAX_RAYS = 1ll << 32;

// composite.hip's wave_suffix_excl: inclusive suffix sum, then shift down by one lane
__device__ __forceinline__ float occh_wave_suffix_excl(float v, int lane, float& total) {
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

__device__ __forceinline__ long long occh_min(long long a, long long b) { return a < b ? a : b; }

struct PdfTail {
    const float* u_f;                  // u_f[B, Nf]; unused with the counter RNG
    float* ts_out;                     // [B, Nc + Nf]
    int Nf;
};

template <int E>
__global__ __launch_bounds__(OCCH_THREADS) void occ_head_capped_pdf_kernel(
    MlpArgs a, const unsigned long long* __restrict__ mask, const long long* __restrict__ offsets,
    const float* __restrict__ raw_live, const float* __restrict__ gt, float* __restrict__ rgb_out,
    float* __restrict__ d_raw_live, long long C, long long B, float mse_scale, PdfTail pdf) {
    constexpr int CHUNKS = OCCH_CHUNKS;
    __shared__ nerf_pdf::WaveLds<E> s_pdf[OCCH_RAYS_PER_BLOCK];
    __shared__ float s_pdf_w[OCCH_RAYS_PER_BLOCK][nerf_pdf::MAXC];
    const int wv = threadIdx.x >> 6;
    const long long ray = (long long)blockIdx.x * OCCH_RAYS_PER_BLOCK + wv;
    const int lane = threadIdx.x & 63;
    const int N = a.N;                         // 3 <= N <= 256
    // the surplus rows [min(P', C), C) of d_raw_live: exact zeros, grid-stride (no wave depends on another's rows)
    {
        const long long kept = occh_min(offsets[B], C);
        f32x4* pad = reinterpret_cast<f32x4*>(d_raw_live) + kept;
        for (long long r = (long long)blockIdx.x * OCCH_THREADS + threadIdx.x; r < C - kept; r += (long long)gridDim.x * OCCH_THREADS)
            pad[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (ray >= B) return;                      // whole wave leaves together; no workgroup barrier below
    const long long first = occh_min(offsets[ray], C);
    const long long n_kept = occh_min(offsets[ray + 1], C) - first;
    const unsigned long long* m = mask + ray * ((N + 63) >> 6);
    const f32x4* rraw = reinterpret_cast<const f32x4*>(raw_live) + first;
    f32x4* rout = reinterpret_cast<f32x4*>(d_raw_live) + first;
    float* rts = s_pdf[wv].ts;                 // the positions: the compositor's and the sampler's
    float* rw = s_pdf_w[wv];
    for (int i = lane; i < N; i += 64) rts[i] = fetch_point_rays<false>(a, ray * N + i, RaySample{ray, i}).t;
    nerf_pdf::wave_lds_fence();
    if (n_kept <= 0) {
        // nothing kept: every sample is (0, 0, 0, -inf), w = 0 throughout: rgb = 0, no row to write, and the sampler's
        // 1e-5 floor spreads the new samples uniformly
        if (lane == 0) { rgb_out[ray * 3 + 0] = 0.f; rgb_out[ray * 3 + 1] = 0.f; rgb_out[ray * 3 + 2] = 0.f; }
        for (int i = lane; i < N; i += 64) rw[i] = 0.f;
    } else {
        const float* d = a.rays + ray * 6 + 3;
        float d0 = d[0], d1 = d[1], d2 = d[2];
        {
            const float n = norm3(d0, d1, d2);
            d0 = __fdiv_rn(d0, n); d1 = __fdiv_rn(d1, n); d2 = __fdiv_rn(d2, n);
        }
        const float dnorm = norm3(d0, d1, d2);

        // forward sweep: per chunk keep alpha, T, fac, delta*softplus' and the colour; rk = the row of a kept sample, -1 dead
        float al[CHUNKS], Tt[CHUNKS], fc[CHUNKS], ds[CHUNKS];
        f32x4 cc[CHUNKS];
        int rk[CHUNKS];
        float carry = 1.0f;
        float sr = 0.f, sg = 0.f, sb = 0.f;    // the forward compositor's rgb, for the loss gradient
        long long before = 0;                  // set mask bits of this ray in earlier chunks
#pragma unroll
        for (int ch = 0; ch < CHUNKS; ++ch) {
            const int base = ch * 64;
            al[ch] = 0.f; Tt[ch] = 0.f; fc[ch] = 1.f; ds[ch] = 0.f;
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
                    ds[ch] = e * delta * spd;  // d alpha / d sigma, from e itself
                    cc[ch] = c;
                }
                before += __popcll(mw);
                // the forward compositor's scan (composite_device.h): same tree, same rounded products
                const float incl = nerf_composite::wave_scan_mul(fac);
                const float excl = nerf_composite::dpp_move<0x138, 0xf>(1.0f, incl);          // wave_shr:1
                al[ch] = a_; fc[ch] = fac; Tt[ch] = mul_rn(carry, excl);
                carry = mul_rn(carry, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(incl), 63)));
                if (valid) {
                    // the same ops as the forward compositor (composite_device.h), so rgb_out equals its rgb and wt its w
                    const float wt = mul_rn(a_, Tt[ch]);
                    sr = __fmaf_rn(wt, cc[ch][0], sr); sg = __fmaf_rn(wt, cc[ch][1], sg); sb = __fmaf_rn(wt, cc[ch][2], sb);
                    rw[i] = rk[ch] >= 0 ? wt : 0.f;            // the sampler's input: exactly 0 at a dead sample
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
                const float suffix = occh_wave_suffix_excl(valid ? G * w : 0.f, lane, tot) + later;
                later += tot;
                if (valid && rk[ch] >= 0) {
                    const float dalpha = G * Tt[ch] - suffix / fc[ch];
                    const f32x4 o = {w * gr, w * gg, w * gb, dalpha * ds[ch]};
                    rout[rk[ch]] = o;
                }
            }
        }
    }
    // the fine pass's positions from this ray's weights (nerf_amd_sample_pdf's body, same draws)
    nerf_pdf::wave_lds_fence();
    nerf_pdf::sample_ray<E>(s_pdf[wv], rw, N, pdf.Nf, lane, pdf.u_f, (a.flags & NERF_FLAG_DEVICE_RNG) != 0, effective_seed(a), a.ray_id0,
                            ray, pdf.ts_out + ray * (long long)(N + pdf.Nf));
}

}  // namespace

extern "C" int nerf_amd_volume_render_masked_mse_backward_pdf(const float* raw_live, const float* rays, const float* u,
                                                              const float* tbins, uint32_t flags, uint64_t seed, int64_t ray_id0,
                                                              const uint64_t* mask, const int64_t* offsets, const float* gt,
                                                              const float* u_f, float* rgb, float* d_raw_live, float* ts_out,
                                                              int64_t capacity, int64_t B, int Nc, int Nf, void* stream) {
    // the rules of the two section-14 entry points (occupancy_graph.hip), restated, with the sampler's limits
    if (B < 0 || Nc <= 0 || Nf < 0 || capacity < 1) return NERF_AMD_EINVAL;
    if (flags & ~(NERF_AMD_TS_GIVEN | NERF_AMD_DEVICE_RNG | NERF_AMD_SEED_IN_MEMORY)) return NERF_AMD_EINVAL;
    if (flags & NERF_AMD_SEED_IN_MEMORY) {
        if (!(flags & NERF_AMD_DEVICE_RNG) || (flags & NERF_AMD_TS_GIVEN) || !u) return NERF_AMD_EINVAL;
        if (reinterpret_cast<uintptr_t>(u) & 7) return NERF_AMD_EINVAL;
    } else if ((!(flags & NERF_AMD_DEVICE_RNG) || (flags & NERF_AMD_TS_GIVEN)) && !u) {
        return NERF_AMD_EINVAL;
    }
    if (!(flags & NERF_AMD_TS_GIVEN) && !tbins) return NERF_AMD_EINVAL;
    if (!(flags & NERF_AMD_DEVICE_RNG) && !u_f && Nf > 0) return NERF_AMD_EINVAL;
    if (Nc < 3 || Nc > nerf_pdf::MAXC || Nc + Nf > nerf_pdf::MAXM || B > OCCH_MAX_RAYS) return NERF_AMD_EUNSUP;
    if (capacity > B * (int64_t)Nc) return NERF_AMD_EINVAL;
    if (!rays || !mask || !offsets || ((uintptr_t)mask & 7) || ((uintptr_t)offsets & 7)) return NERF_AMD_EINVAL;
    if (!raw_live || !gt || !rgb || !d_raw_live || !ts_out || ((uintptr_t)raw_live & 15) || ((uintptr_t)d_raw_live & 15) ||
        ((uintptr_t)gt & 3) || ((uintptr_t)rgb & 3) || ((uintptr_t)ts_out & 3) || ((uintptr_t)u_f & 3))
        return NERF_AMD_EINVAL;
    (void)hipGetLastError();
    MlpArgs a{};
    a.rays = rays; a.u = u; a.tbins = tbins;
    a.P = B * (int64_t)Nc; a.N = Nc; a.flags = flags; a.seed = seed; a.ray_id0 = ray_id0;
    const dim3 grid((unsigned)((B + OCCH_RAYS_PER_BLOCK - 1) / OCCH_RAYS_PER_BLOCK)), block(OCCH_THREADS);
    const PdfTail pdf{u_f, ts_out, Nf};
    const float scale = 1.0f / (3.0f * (float)B);
#define OCCH_HEAD(E_)                                                                                                        \
    hipLaunchKernelGGL(occ_head_capped_pdf_kernel<E_>, grid, block, 0, reinterpret_cast<hipStream_t>(stream), a,             \
                       reinterpret_cast<const unsigned long long*>(mask), reinterpret_cast<const long long*>(offsets), raw_live, \
                       gt, rgb, d_raw_live, (long long)capacity, (long long)B, scale, pdf)
    switch (nerf_pdf::keys_per_lane(Nf)) {
        case 1: OCCH_HEAD(1); break;
        case 2: OCCH_HEAD(2); break;
        case 4: OCCH_HEAD(4); break;
        default: OCCH_HEAD(8); break;
    }
#undef OCCH_HEAD
    return (int)hipGetLastError();
}
