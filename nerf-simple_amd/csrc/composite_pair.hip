// composite_pair.hip -- the dense COARSE head of the coarse + fine pair with its training controls, ONE kernel: compositor + MSE
// gradient + compositor backward on composite_backward_ray (composite_backward_device.h) with
//   NOISE    Gaussian noise on the raw density in front of the softplus (sigma_noise_device.h Noisy<Src>)
//   BG       the loss behind a background colour                         (the stages: composite_bg.hip)
// as the dense head has them (composite_head.hip), and the fine pass's sample placement (sample_pdf_device.h, E keys per lane)
// behind the walk in the same wave, as composite_backward_kernel<E> (composite.hip) does it for the plain coarse head: the
// weights go from registers to the wave's LDS slice with the positions (PdfSink) and the sampler reads them there, so w never
// reaches HBM.  The sampler sees the weights of the NOISY compositor; the background never touches them.  The distortion term
// is not offered: it belongs on the final weights, not on what places the samples.
// (NOISE, BG) in {(0,1), (1,0), (1,1)} x E in {1, 2, 4, 8} are instantiated, and nothing else; with no term the launcher hands
// on to the plain coarse head's launch.  LDS per block 4 * (6 KB + 256 E B), the plain coarse head's.  No atomics.
#include "composite_backward_device.h"
#include "launchers.h"
#include "sample_pdf_device.h"
#include "sigma_noise_device.h"

namespace {

constexpr int RAYS_PER_BLOCK = 4;

// Nc >= 3 (the sampler's minimum): the reference's empty sample axis at N == 1 does not occur here.
template <bool NOISE, bool BG, int E>
__global__ __launch_bounds__(64 * RAYS_PER_BLOCK) void dense_head_pdf_kernel(const DenseHeadArgs a, const DensePdfArgs p) {
    static_assert(NOISE || BG, "with no term the coarse head is composite_backward_kernel<E>");
    __shared__ nerf_pdf::WaveLds<E> s_pdf[RAYS_PER_BLOCK];
    __shared__ float s_pdf_w[RAYS_PER_BLOCK][nerf_pdf::MAXC];
    const int wv = threadIdx.x >> 6;
    const long long ray = (long long)blockIdx.x * RAYS_PER_BLOCK + wv;
    if (ray >= a.B) return;                    // whole wave leaves together; no barriers below
    const int lane = threadIdx.x & 63, N = a.N;
    f32x4* rout = reinterpret_cast<f32x4*>(a.d_raw) + ray * N;
    const nerf_composite::LossHead<BG, false, false> up{a.target, a.rgb, a.scale, a.bg, a.bg_stride, 0.f, 0.f, nullptr,
                                                        nullptr, 0, nullptr};
    const float* d = a.rays + ray * 6 + 3;
    const float dnorm = nerf_composite::unit_dir_norm(d[0], d[1], d[2], true);
    const nerf_composite::DenseSamples dense{a.ts + ray * N, reinterpret_cast<const f32x4*>(a.raw) + ray * N};
    const nerf_composite::PdfSink sink{s_pdf[wv].ts, s_pdf_w[wv]};
    if constexpr (NOISE) {
        nerf_composite::composite_backward_ray<nerf_pdf::MAXC / 64>(
            nerf_noise::Noisy<nerf_composite::DenseSamples>{dense, a.std, nerf_noise::noise_key(a.seed, a.seed_mem),
                                                            (unsigned long long)((a.ray_id0 + ray) * N)},
            up, sink, N, lane, dnorm, ray, rout);
    } else {
        nerf_composite::composite_backward_ray<nerf_pdf::MAXC / 64>(dense, up, sink, N, lane, dnorm, ray, rout);
    }
    // the fine pass's positions from this ray's weights (nerf_amd_sample_pdf's body, same draws)
    wave_lds_fence();
    unsigned long long seed = p.seed;
    if (p.seed_in_mem) {
        const unsigned long long v = *reinterpret_cast<const unsigned long long*>(p.u);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        seed += ((unsigned long long)hi << 32) | lo;
    }
    nerf_pdf::sample_ray<E>(s_pdf[wv], s_pdf_w[wv], N, p.Nf, lane, p.u, p.device_rng != 0, seed, a.ray_id0, ray,
                            p.ts_out + ray * (N + p.Nf));
}

}  // namespace

// a.N = Nc; a.dist and a.theta are not looked at
extern "C" int nerf_amd_launch_dense_head_pdf(const DenseHeadArgs* args, const DensePdfArgs* pdf, hipStream_t stream) {
    DenseHeadArgs a = *args;
    const DensePdfArgs p = *pdf;
    const bool noise = a.std != 0.f, bg = a.bg != nullptr;
    if (!noise && !bg)                         // no term: the plain coarse head's launch itself (composite.hip)
        return nerf_amd_launch_composite_mse_backward_pdf(a.raw, a.ts, a.rays, a.target, a.rgb, a.d_raw, p.u, p.ts_out, a.B, a.N,
                                                          p.Nf, p.seed, a.ray_id0, p.device_rng, p.seed_in_mem, stream);
    (void)hipGetLastError();
    if (a.B == 0) return 0;
    if (p.Nf < 0 || nerf_pdf::unsupported_sizes(a.N, p.Nf)) return -2;
    const dim3 grid((unsigned)((a.B + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK)), block(64 * RAYS_PER_BLOCK);
    a.scale = 1.0f / (3.0f * (float)a.B);
#define NERF_HEAD_PDF(NOISE_, BG_, E_) \
    hipLaunchKernelGGL((dense_head_pdf_kernel<NOISE_, BG_, E_>), grid, block, 0, stream, a, p)
#define NERF_HEAD_PDF_E(NOISE_, BG_)                        \
    switch (nerf_pdf::keys_per_lane(p.Nf)) {                \
        case 1: NERF_HEAD_PDF(NOISE_, BG_, 1); break;       \
        case 2: NERF_HEAD_PDF(NOISE_, BG_, 2); break;       \
        case 4: NERF_HEAD_PDF(NOISE_, BG_, 4); break;       \
        default: NERF_HEAD_PDF(NOISE_, BG_, 8); break;      \
    }
    if (!noise) NERF_HEAD_PDF_E(false, true)
    else if (!bg) NERF_HEAD_PDF_E(true, false)
    else NERF_HEAD_PDF_E(true, true)
#undef NERF_HEAD_PDF_E
#undef NERF_HEAD_PDF
    return (int)hipGetLastError();
}
