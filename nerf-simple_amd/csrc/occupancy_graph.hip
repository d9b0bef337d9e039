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
//       ray below i) < C.  The walk is composite_backward_ray (composite_backward_device.h) over the masked samples with
//       the MSE head, as composite.hip's training head runs it over the dense ones; the clamp is in how the ray's first row
//       and kept count are formed.  d_raw_live[C, 4]: kept rows from the sweep, rows behind min(P', C) zero.
//
// No atomics; the kept rows and the pad rows are disjoint ranges, so no two lanes write one address and two runs write the
// same bytes.  The host wrappers below are the C ABI themselves (argument checking included, api_checks.h).
#include "composite_backward_device.h"
#include "occ_scan_device.h"
#include "api_checks.h"

namespace {

constexpr int OCCG_RAYS_PER_BLOCK = 4;
constexpr int OCCG_THREADS = 64 * OCCG_RAYS_PER_BLOCK;
constexpr int OCCG_MAX_CHUNKS = nerf_layout::COMPOSITE_BWD_MAX_CHUNKS;      // N <= 512: the masked compositor backward's limit
constexpr int OCCG_MAX_N = COMPOSITE_BWD_MAX_N;

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
        const long long first = offsets[ray];
        // skip a ray with nothing live, or with every live sample behind the capacity; the kept rows: global rank below it
        if (offsets[ray + 1] != first && first < C) emit_ray_rows(a, mask + ray * ((a.N + 63) >> 6), pts, first, C, ray, lane);
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
    wave_lds_fence();
    const float* d = a.rays + ray * 6 + 3;
    const float dnorm = nerf_composite::unit_dir_norm(d[0], d[1], d[2], true);
    const nerf_composite::MaskedSamplesBwd src{s_t[wv], m, reinterpret_cast<const f32x4*>(raw_live) + first, n_kept};
    // loss = MSELoss(rgb, gt) (train.py:52): only rgb feeds it
    nerf_composite::composite_backward_ray<OCCG_MAX_CHUNKS>(src, nerf_composite::MseHead{gt, rgb_out, mse_scale},
                                                            nerf_composite::NoSink{}, N, lane, dnorm, ray, rout);
}

// what both entry points share: 0 = go on, otherwise the code to return.  1 <= C <= B N, so B >= 1.
int occg_check(const float* rays, const float* u, const float* tbins, uint32_t flags, const uint64_t* mask, const int64_t* offsets,
               int64_t C, int64_t B, int N) {
    if (C < 1) return NERF_AMD_EINVAL;
    const int rc = masked_rays_check(rays, u, tbins, flags, B, N, N > OCCG_MAX_N);
    return rc ? rc : capped_check(mask, offsets, C, B, N);
}

}  // namespace

extern "C" int nerf_amd_occupancy_points_capped(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed,
                                                int64_t ray_id0, const uint64_t* mask, const int64_t* offsets, float* pts,
                                                int64_t* counts, int64_t capacity, int64_t B, int N, void* stream) {
    const int rc = occg_check(rays, u, tbins, flags, mask, offsets, capacity, B, N);
    if (rc) return rc;
    if (!pts || !counts || misaligned(pts, 4) || misaligned(counts, 8)) return NERF_AMD_EINVAL;
    (void)hipGetLastError();
    const MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
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
    if (!raw_live || !gt || !rgb || !d_raw_live || misaligned(raw_live, 16) || misaligned(d_raw_live, 16) ||
        misaligned(gt, 4) || misaligned(rgb, 4))
        return NERF_AMD_EINVAL;
    (void)hipGetLastError();
    const MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    const long long blocks = (B + OCCG_RAYS_PER_BLOCK - 1) / OCCG_RAYS_PER_BLOCK;
    hipLaunchKernelGGL(occ_head_capped_kernel, dim3((unsigned)blocks), dim3(OCCG_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a,
                       reinterpret_cast<const unsigned long long*>(mask), reinterpret_cast<const long long*>(offsets), raw_live, gt, rgb,
                       d_raw_live, (long long)capacity, (long long)B, 1.0f / (3.0f * (float)B));
    return (int)hipGetLastError();
}
