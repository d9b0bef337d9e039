// composite_head.hip -- the dense training head with its optional terms, ONE kernel: compositor + MSE gradient + compositor
// backward on composite_backward_ray (composite_backward_device.h), one wavefront per ray, with any of
//   NOISE    Gaussian noise on the raw density in front of the softplus (sigma_noise_device.h Noisy<Src>)
//   BG       the loss behind a background colour                         (the stages: composite_bg.hip)
//   DIST     the distortion loss of the ray's weights beside the MSE     (the stage: composite_dist.hip)
//   AFFINE   the loss behind a per-image colour correction               (the stages: appearance.hip)
//   E        0: no sampler.  1, 2, 4, 8: the COARSE head of the coarse + fine pair -- the fine pass's sample placement
//            (sample_pdf_device.h, E keys per lane) runs behind the walk in the same wave, as composite_backward_kernel<E>
//            (composite.hip) does it for the plain coarse head: the weights go from registers to the wave's LDS slice with the
//            positions (PdfSink) and the sampler reads them there, so w never reaches HBM.  The sampler sees the weights of the
//            NOISY compositor; the background never touches them.  Not with DIST (the term belongs on the final weights, not on
//            what places the samples: DESIGN.md section 35) nor AFFINE.  Nc <= 256: four chunks, and Nc >= 3, so no empty
//            sample axis; LDS per block 4 * (6 KB + 256 E B), the plain coarse head's.
// Each is BY DEFINITION the composition of those stages with the compositor and its backward (LossHead's comment).  The
// combinations the entry points of api.hip reach are instantiated, and nothing else: eight without a sampler, and (NOISE, BG) in
// {(0,1), (1,0), (1,1)} x E in {1, 2, 4, 8}.  With no term at all the head is composite_backward_kernel<E> with the MSE head
// (composite.hip), whose launch the two launchers hand on to.  No atomics.
#include "composite_backward_device.h"
#include "launchers.h"
#include "sample_pdf_device.h"
#include "sigma_noise_device.h"

namespace {

constexpr int RAYS_PER_BLOCK = 4;
constexpr int MAX_CHUNKS = nerf_layout::COMPOSITE_BWD_MAX_CHUNKS;          // N <= 512

// `p` is looked at with a sampler only (E > 0).  The scheduler follows the order of the statements, and the instructions of every
// instantiation are pinned (profiles/one_head_isa_diff.txt): the wave index is read in front of the block index with a sampler
// only, and the sink is formed in front of the source.
template <bool NOISE, bool BG, bool DIST, bool AFFINE, int E>
__global__ __launch_bounds__(64 * RAYS_PER_BLOCK) void dense_head_kernel(const DenseHeadArgs a, const DensePdfArgs p) {
    static_assert(E == 0 || (!DIST && !AFFINE), "the sampler runs behind the MSE head, plain or with background / noise");
    static_assert(E == 0 || NOISE || BG, "with no term the coarse head is composite_backward_kernel<E>");
    constexpr int CHUNKS = E > 0 ? nerf_pdf::MAXC / 64 : MAX_CHUNKS;
    __shared__ nerf_pdf::WaveLds<(E > 0 ? E : 1)> s_pdf[E > 0 ? RAYS_PER_BLOCK : 1];
    __shared__ float s_pdf_w[E > 0 ? RAYS_PER_BLOCK : 1][nerf_pdf::MAXC];
    const int wv = E > 0 ? threadIdx.x >> 6 : 0;           // the wave's LDS slice: with a sampler only
    const long long ray = (long long)blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= a.B) return;                    // whole wave leaves together; no barriers below
    const int lane = threadIdx.x & 63, N = a.N;
    f32x4* rout = reinterpret_cast<f32x4*>(a.d_raw) + ray * N;
    const nerf_composite::LossHead<BG, DIST, AFFINE> up{a.target, a.rgb, a.scale, a.bg, a.bg_stride, a.t_far, a.coef, a.loss_ray,
                                                        a.theta, a.theta_stride, a.g_theta};
    if constexpr (E == 0) {                    // with a sampler N >= 3
        if (N == 1) {
            nerf_composite::loss_head_empty_ray(up, lane, ray, rout);
            return;
        }
    }
    const float* d = a.rays + ray * 6 + 3;
    const float dnorm = nerf_composite::unit_dir_norm(d[0], d[1], d[2], true);
    const nerf_composite::DenseSamples dense{a.ts + ray * N, reinterpret_cast<const f32x4*>(a.raw) + ray * N};
    const auto sink = [&] {
        if constexpr (E > 0) return nerf_composite::PdfSink{s_pdf[wv].ts, s_pdf_w[wv]};
        else return nerf_composite::NoSink{};
    }();
    const auto src = [&] {
        if constexpr (NOISE)
            return nerf_noise::Noisy<nerf_composite::DenseSamples>{dense, a.std, nerf_noise::noise_key(a.seed, a.seed_mem),
                                                                   (unsigned long long)((a.ray_id0 + ray) * N)};
        else return dense;
    }();
    nerf_composite::composite_backward_ray<CHUNKS>(src, up, sink, N, lane, dnorm, ray, rout);
    if constexpr (E > 0)
        nerf_pdf::sample_behind_walk<E>(s_pdf[wv], s_pdf_w[wv], N, lane, p, a.ray_id0, ray);
}

}  // namespace

extern "C" int nerf_amd_launch_dense_head(const DenseHeadArgs* args, hipStream_t stream) {
    DenseHeadArgs a = *args;
    const bool noise = a.std != 0.f, bg = a.bg != nullptr, affine = a.theta != nullptr;
    if (!noise && !bg && !a.dist && !affine)   // no term: the plain head's launch itself (composite.hip)
        return nerf_amd_launch_composite_mse_backward(a.raw, a.ts, a.rays, a.target, a.rgb, a.d_raw, a.B, a.N, stream);
    (void)hipGetLastError();
    if (a.B == 0) return 0;
    if (a.N > nerf_layout::COMPOSITE_BWD_MAX_N || (affine && (noise || bg || a.dist))) return -2;
    const dim3 grid((unsigned)((a.B + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK)), block(64 * RAYS_PER_BLOCK);
    a.scale = 1.0f / (3.0f * (float)a.B);
#define NERF_HEAD(NOISE_, BG_, DIST_, AFFINE_) \
    hipLaunchKernelGGL((dense_head_kernel<NOISE_, BG_, DIST_, AFFINE_, 0>), grid, block, 0, stream, a, DensePdfArgs{})
    if (affine) NERF_HEAD(false, false, false, true);
    else if (a.dist && !noise && !bg) NERF_HEAD(false, false, true, false);
    else if (a.dist) with_noise_bg(noise, bg, [&](auto n, auto b) { NERF_HEAD(n(), b(), true, false); });
    else with_noise_bg(noise, bg, [&](auto n, auto b) { NERF_HEAD(n(), b(), false, false); });
#undef NERF_HEAD
    return (int)hipGetLastError();
}

// the coarse head of the pair: a.N = Nc; a.dist and a.theta are not looked at
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
    nerf_pdf::with_keys_per_lane(p.Nf, [&](auto e) {
        with_noise_bg(noise, bg, [&](auto n, auto b) {
            hipLaunchKernelGGL((dense_head_kernel<n(), b(), false, false, e()>), grid, block, 0, stream, a, p);
        });
    });
    return (int)hipGetLastError();
}
