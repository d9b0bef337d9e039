// composite_dist.hip -- mip-NeRF 360's distortion loss for the dense training path: the regulariser every trainer with a
// non-uniform sampler pairs its placement with (it pulls a ray's weights together into one compact interval).
//   nerf_amd_distortion_loss   ts, w -> coef D per ray and coef dD/dw        (the per-ray routine: composite_dist_device.h)
//   nerf_amd_sum_f32           the sum of a vector in a fixed order (the step's distortion term from the per-ray values)
//   the training head          BY DEFINITION noise -> compositor -> distortion loss on its w -> blend -> MSE gradient -> the
//                              blend's backward -> compositor backward (g_rgb, g_acc, g_w), in one launch:
//                              dense_head_kernel<NOISE, BG, DIST, ..> (composite_head.hip)
#include "composite_dist_device.h"
#include "launchers.h"

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
