// composite_dist.hip -- mip-NeRF 360's distortion loss for the dense training path: the regulariser every trainer with a
// non-uniform sampler pairs its placement with (it pulls a ray's weights together into one compact interval).
//   nerf_amd_distortion_loss   ts, w -> coef D per ray and coef dD/dw        (the per-ray routine: composite_dist_device.h)
//   nerf_amd_sum_f32           the sum of a vector in a fixed order (the step's distortion term from the per-ray values)
//   the training head          BY DEFINITION noise -> compositor -> distortion loss on its w -> blend -> MSE gradient -> the
//                              blend's backward -> compositor backward (g_rgb, g_acc, g_w), in one launch on
//                              composite_backward_ray with a DistMseHead (composite_backward_device.h)
#include "composite_backward_device.h"
#include "launchers.h"
#include "sigma_noise_device.h"

namespace {

using nerf_composite::wave_sum;

constexpr int RAYS_PER_BLOCK = 4;
constexpr int MAX_CHUNKS = nerf_layout::COMPOSITE_BWD_MAX_CHUNKS;          // N <= 512

// ONE wavefront per ray: the ray's positions and weights into registers, one sample per lane and chunk
__global__ __launch_bounds__(64 * RAYS_PER_BLOCK) void distortion_loss_kernel(const float* __restrict__ ts, const float* __restrict__ w,
                                                                             float t_far, float coef, float* __restrict__ loss_ray,
                                                                             float* __restrict__ g_w, long long B, int N) {
    const long long ray = (long long)blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= B) return;                      // whole wave leaves together; no barriers below
    const int lane = threadIdx.x & 63;
    if (N == 1) {
        // the reference's EMPTY sample axis at N == 1 (composite_device.h): no weight, D = 0 and no gradient
        if (lane == 0) {
            if (loss_ray) loss_ray[ray] = 0.f;
            if (g_w) g_w[ray] = 0.f;
        }
        return;
    }
    const float* rt = ts + ray * N;
    const float* rw = w + ray * N;
    float t[MAX_CHUNKS], wv[MAX_CHUNKS], gw[MAX_CHUNKS];
#pragma unroll
    for (int ch = 0; ch < MAX_CHUNKS; ++ch) {
        const int i = ch * 64 + lane;
        t[ch] = 0.f; wv[ch] = 0.f;
        if (i < N) { t[ch] = rt[i]; wv[ch] = rw[i]; }
    }
    const float dist = nerf_composite::distortion_ray<MAX_CHUNKS>(t, wv, N, lane, t_far, coef, gw);
    if (loss_ray && lane == 0) loss_ray[ray] = dist;
    if (g_w) {
#pragma unroll
        for (int ch = 0; ch < MAX_CHUNKS; ++ch) {
            const int i = ch * 64 + lane;
            if (i < N) g_w[ray * N + i] = gw[ch];
        }
    }
}

// One workgroup, fixed summation order (as mse_loss_kernel, composite.hip): bit-reproducible from run to run.
__global__ __launch_bounds__(1024) void sum_f32_kernel(const float* __restrict__ x, float* __restrict__ out, long long n) {
    __shared__ float red[16];
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += 1024) s = add_rn(s, x[i]);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int k = 0; k < 16; ++k) t = add_rn(t, red[k]);
        *out = t;
    }
}

// ---- the training head -----------------------------------------------------------------------------------------------------
// composite_bg_head_kernel (composite_bg.hip) with the distortion term: NOISE: sigma' in front of the softplus; BG: the MSE
// sits behind the blend.  All four combinations live here: (false, false) is the plain chain with the term.
template <bool NOISE, bool BG>
__global__ __launch_bounds__(64 * RAYS_PER_BLOCK) void composite_dist_head_kernel(
    const float* __restrict__ raw, const float* __restrict__ ts, const float* __restrict__ rays,
    const float* __restrict__ target, const float* __restrict__ bg, long long bg_stride, float std, unsigned long long seed,
    const unsigned long long* __restrict__ seed_mem, long long ray_id0, float t_far, float coef, float* __restrict__ rgb_out,
    float* __restrict__ loss_ray, float* __restrict__ d_raw, long long B, int N, float scale) {
    const long long ray = (long long)blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= B) return;                      // whole wave leaves together; no barriers below
    const int lane = threadIdx.x & 63;
    f32x4* rout = reinterpret_cast<f32x4*>(d_raw) + ray * N;
    if (N == 1) {
        // the reference's EMPTY sample axis at N == 1: rgb = acc = 0 (rgb_bg = bg exactly), no weight, so D = 0
        if (lane == 0) {
            rout[0] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (loss_ray) loss_ray[ray] = 0.f;
            if (rgb_out) {
                for (int c = 0; c < 3; ++c) rgb_out[ray * 3 + c] = BG ? add_rn(0.f, mul_rn(sub_rn(1.0f, 0.f), bg[ray * bg_stride + c])) : 0.f;
            }
        }
        return;
    }
    const float* d = rays + ray * 6 + 3;
    const float dnorm = nerf_composite::unit_dir_norm(d[0], d[1], d[2], true);
    const nerf_composite::DenseSamples dense{ts + ray * N, reinterpret_cast<const f32x4*>(raw) + ray * N};
    const nerf_composite::DistMseHead<BG> up{target, rgb_out, scale, bg, bg_stride, t_far, coef, loss_ray};
    if constexpr (NOISE) {
        nerf_composite::composite_backward_ray<MAX_CHUNKS>(
            nerf_noise::NoisySamples{dense, std, nerf_noise::noise_key(seed, seed_mem), (unsigned long long)((ray_id0 + ray) * N)}, up,
            nerf_composite::NoSink{}, N, lane, dnorm, ray, rout);
    } else {
        nerf_composite::composite_backward_ray<MAX_CHUNKS>(dense, up, nerf_composite::NoSink{}, N, lane, dnorm, ray, rout);
    }
}

}  // namespace

extern "C" int nerf_amd_launch_distortion_loss(const float* ts, const float* w, float t_far, float coef, float* loss_ray,
                                               float* g_w, long long B, int N, hipStream_t stream) {
    (void)hipGetLastError();
    if (B == 0 || (!loss_ray && !g_w)) return 0;
    if (N > nerf_layout::COMPOSITE_BWD_MAX_N) return -2;
    const long long blocks = (B + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK;
    if (blocks > 0x7fffffffll) return -2;                              // the grid's x extent
    hipLaunchKernelGGL(distortion_loss_kernel, dim3((unsigned)blocks), dim3(64 * RAYS_PER_BLOCK), 0, stream, ts, w, t_far, coef,
                       loss_ray, g_w, B, N);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_sum_f32(const float* x, float* out, long long n, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(sum_f32_kernel, dim3(1), dim3(1024), 0, stream, x, out, n);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_composite_mse_backward_dist(const float* raw, const float* ts, const float* rays,
                                                           const float* target, const float* bg, long long bg_stride, float std,
                                                           unsigned long long seed, const unsigned long long* seed_mem,
                                                           long long ray_id0, float t_far, float coef, float* rgb,
                                                           float* loss_ray, float* d_raw, long long B, int N,
                                                           hipStream_t stream) {
    (void)hipGetLastError();
    if (B == 0) return 0;
    if (N > nerf_layout::COMPOSITE_BWD_MAX_N) return -2;
    const dim3 grid((unsigned)((B + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK)), block(64 * RAYS_PER_BLOCK);
    const float scale = 1.0f / (3.0f * (float)B);
#define NERF_DIST_HEAD(NOISE_, BG_)                                                                                            \
    hipLaunchKernelGGL((composite_dist_head_kernel<NOISE_, BG_>), grid, block, 0, stream, raw, ts, rays, target, bg, bg_stride, \
                       std, seed, seed_mem, ray_id0, t_far, coef, rgb, loss_ray, d_raw, B, N, scale)
    if (std == 0.f && !bg) NERF_DIST_HEAD(false, false);
    else if (std == 0.f) NERF_DIST_HEAD(false, true);
    else if (!bg) NERF_DIST_HEAD(true, false);
    else NERF_DIST_HEAD(true, true);
#undef NERF_DIST_HEAD
    return (int)hipGetLastError();
}
