// composite_head.hip -- the dense training head with its optional terms, ONE kernel: compositor + MSE gradient + compositor
// backward on composite_backward_ray (composite_backward_device.h), one wavefront per ray, with any of
//   NOISE    Gaussian noise on the raw density in front of the softplus (sigma_noise_device.h Noisy<Src>)
//   BG       the loss behind a background colour                         (the stages: composite_bg.hip)
//   DIST     the distortion loss of the ray's weights beside the MSE     (the stage: composite_dist.hip)
//   AFFINE   the loss behind a per-image colour correction               (the stages: appearance.hip)
// Each is BY DEFINITION the composition of those stages with the compositor and its backward (LossHead's comment).  The
// combinations the three entry points of api.hip reach are instantiated, and nothing else; with no term at all the head is
// composite_backward_kernel<0> with the MSE head (composite.hip), whose launch this launcher hands on to.
#include "composite_backward_device.h"
#include "launchers.h"
#include "sigma_noise_device.h"

namespace {

constexpr int RAYS_PER_BLOCK = 4;
constexpr int MAX_CHUNKS = nerf_layout::COMPOSITE_BWD_MAX_CHUNKS;          // N <= 512

template <bool NOISE, bool BG, bool DIST, bool AFFINE>
__global__ __launch_bounds__(64 * RAYS_PER_BLOCK) void dense_head_kernel(const DenseHeadArgs a) {
    const long long ray = (long long)blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= a.B) return;                    // whole wave leaves together; no barriers below
    const int lane = threadIdx.x & 63, N = a.N;
    f32x4* rout = reinterpret_cast<f32x4*>(a.d_raw) + ray * N;
    const nerf_composite::LossHead<BG, DIST, AFFINE> up{a.target, a.rgb, a.scale, a.bg, a.bg_stride, a.t_far, a.coef, a.loss_ray,
                                                        a.theta, a.theta_stride, a.g_theta};
    if (N == 1) {
        nerf_composite::loss_head_empty_ray(up, lane, ray, rout);
        return;
    }
    const float* d = a.rays + ray * 6 + 3;
    const float dnorm = nerf_composite::unit_dir_norm(d[0], d[1], d[2], true);
    const nerf_composite::DenseSamples dense{a.ts + ray * N, reinterpret_cast<const f32x4*>(a.raw) + ray * N};
    if constexpr (NOISE) {
        nerf_composite::composite_backward_ray<MAX_CHUNKS>(
            nerf_noise::Noisy<nerf_composite::DenseSamples>{dense, a.std, nerf_noise::noise_key(a.seed, a.seed_mem),
                                                            (unsigned long long)((a.ray_id0 + ray) * N)},
            up, nerf_composite::NoSink{}, N, lane, dnorm, ray, rout);
    } else {
        nerf_composite::composite_backward_ray<MAX_CHUNKS>(dense, up, nerf_composite::NoSink{}, N, lane, dnorm, ray, rout);
    }
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
    hipLaunchKernelGGL((dense_head_kernel<NOISE_, BG_, DIST_, AFFINE_>), grid, block, 0, stream, a)
    if (affine) NERF_HEAD(false, false, false, true);
    else if (!a.dist && !noise) NERF_HEAD(false, true, false, false);
    else if (!a.dist && !bg) NERF_HEAD(true, false, false, false);
    else if (!a.dist) NERF_HEAD(true, true, false, false);
    else if (!noise && !bg) NERF_HEAD(false, false, true, false);
    else if (!noise) NERF_HEAD(false, true, true, false);
    else if (!bg) NERF_HEAD(true, false, true, false);
    else NERF_HEAD(true, true, true, false);
#undef NERF_HEAD
    return (int)hipGetLastError();
}
