// occupancy_train.hip -- training with empty-space skipping: the backward of the masked compositor and the running density
// volume a training occupancy grid is refreshed from.  Not in the reference.
//
//   occ_composite_backward_kernel -- d loss / d raw_live[P', 4] of nerf_amd_volume_render_masked.  One wavefront per ray,
//       lane = ORIGINAL sample index, N walked in chunks of 64 by composite_backward_ray (composite_backward_device.h), the
//       walk of the dense raw[B, N, 4]: positions recomputed (fetch_point_rays) into the wave's LDS slice, the network's
//       output read at offsets[ray] + rank for a live sample -- rank from popcounts of the mask words -- and (0, 0, 0, -inf)
//       for a dead one.  A dead sample has softplus' = 0, alpha = 0 and w = 0 there: it receives nothing and adds exact
//       zeros to the suffix sums.  The result is the rows at the live samples of the dense backward on the overwritten raw,
//       bit for bit.  No atomics: row offsets[ray] + rank is written by exactly one lane.
//   occ_decay_max_kernel -- state = max(fl(state decay), softplus(sigma_now)), softplus as the compositor's.
#include "composite_backward_device.h"
#include "launchers.h"

namespace {

constexpr int OCCT_RAYS_PER_BLOCK = 4;
constexpr int OCCT_MAX_CHUNKS = nerf_layout::COMPOSITE_BWD_MAX_CHUNKS;      // N <= 512, the dense backward's limit
constexpr int OCCT_MAX_N = nerf_layout::COMPOSITE_BWD_MAX_N;

__global__ __launch_bounds__(64 * OCCT_RAYS_PER_BLOCK) void occ_composite_backward_kernel(
    MlpArgs a, const unsigned long long* __restrict__ mask, const long long* __restrict__ offsets,
    const float* __restrict__ raw_live, const float* __restrict__ g_rgb, const float* __restrict__ g_disp,
    const float* __restrict__ g_alpha, const float* __restrict__ g_acc, const float* __restrict__ g_w,
    float* __restrict__ d_raw_live, long long B) {
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
    f32x4* rout = reinterpret_cast<f32x4*>(d_raw_live) + first;
    if (N == 1) {
        // the reference composites an EMPTY sample axis at N == 1 (composite_device.h): no output depends on raw
        if (lane == 0 && (m[0] & 1ull)) rout[0] = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    for (int i = lane; i < N; i += 64) s_t[wv][i] = fetch_point_rays<false>(a, ray * N + i, RaySample{ray, i}).t;
    wave_lds_fence();
    const float* d = a.rays + ray * 6 + 3;
    const float dnorm = nerf_composite::unit_dir_norm(d[0], d[1], d[2], true);
    const nerf_composite::MaskedSamplesBwd src{s_t[wv], m, reinterpret_cast<const f32x4*>(raw_live) + first, n_live};
    nerf_composite::composite_backward_ray<OCCT_MAX_CHUNKS>(src, nerf_composite::FiveGrads{g_rgb, g_disp, g_alpha, g_acc, g_w},
                                                            nerf_composite::NoSink{}, N, lane, dnorm, ray, rout);
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
