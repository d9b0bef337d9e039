// occupancy_graph.hip -- the light passes of the GRAPHED masked training steps (include/nerf_amd.h, "graphed masked
// training step" and "masked hierarchical pair"; DESIGN.md sections 14 and 15).  A captured step has no host in it, so the
// live count P' of a batch cannot size anything: the network kernels run on a fixed capacity of C points, and these passes
// make the rows beyond min(P', C) inert.  Not in the reference.
//
//   occ_emit_capped_kernel -- pts[C, 6]: row r < min(P', C) is the row nerf_amd_occupancy_points writes (one wavefront per
//       ray, the same fetch_point_rays), every row behind is the pad point; counts = {P', min(P', C)}.  P' = offsets[B] is
//       read from device memory.  Every row of pts is written by exactly one lane on every launch.
//   the two fused heads -- masked compositor forward -> g_rgb = 2 (rgb - gt) / (3 B) -> masked compositor backward in one
//       launch under the capacity clamp, and for the coarse head of the hierarchical pair the fine pass's sample placement
//       behind it in the same wave (the fine pass's mark depends on ts_out, so in a captured step both have to come out of
//       one node chain with no host in it).  Both are masked_backward_kernel<MseHead, false, E> (occupancy_train.hip) with
//       capacity = C; this source holds their entry points, which fill MaskedBackwardArgs through capped_head_args
//       (launchers.h) as the head with the training controls does (masked_controls.hip).
//
// No atomics; the kept rows and the pad rows are disjoint ranges, so no two lanes write one address and two runs write the
// same bytes.  The host wrappers below are the C ABI themselves (argument checking included, api_checks.h).
#include "occ_scan_device.h"
#include "sample_pdf_device.h"
#include "api_checks.h"
#include "launchers.h"

namespace {

// ---- capped emit ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MASKED_THREADS) void occ_emit_capped_kernel(MlpArgs a, const unsigned long long* __restrict__ mask,
                                                                         const long long* __restrict__ offsets,
                                                                         float* __restrict__ pts, long long* __restrict__ counts,
                                                                         long long C, long long B) {
    const long long ray = (long long)blockIdx.x * MASKED_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long long total = offsets[B];
    const long long kept = min_ll(total, C);
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
    for (long long e = (long long)blockIdx.x * MASKED_THREADS + threadIdx.x; e < n_pad; e += (long long)gridDim.x * MASKED_THREADS)
        pad[e] = pad_point[e % 6];
}

// what the section-14 entry points share: 0 = go on, otherwise the code to return.  1 <= C <= B N, so B >= 1.
int occg_check(const float* rays, const float* u, const float* tbins, uint32_t flags, const uint64_t* mask, const int64_t* offsets,
               int64_t C, int64_t B, int N) {
    if (C < 1) return NERF_AMD_EINVAL;
    const int rc = masked_rays_check(rays, u, tbins, flags, B, N, N > COMPOSITE_BWD_MAX_N);
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
    const long long blocks = (B + MASKED_RAYS_PER_BLOCK - 1) / MASKED_RAYS_PER_BLOCK;
    hipLaunchKernelGGL(occ_emit_capped_kernel, dim3((unsigned)blocks), dim3(MASKED_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a,
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
    const MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    const MaskedBackwardArgs b = capped_head_args(raw_live, mask, offsets, gt, rgb, d_raw_live, capacity, B);
    return nerf_amd_launch_masked_backward(&a, &b, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int nerf_amd_volume_render_masked_mse_backward_pdf(const float* raw_live, const float* rays, const float* u,
                                                              const float* tbins, uint32_t flags, uint64_t seed, int64_t ray_id0,
                                                              const uint64_t* mask, const int64_t* offsets, const float* gt,
                                                              const float* u_f, float* rgb, float* d_raw_live, float* ts_out,
                                                              int64_t capacity, int64_t B, int Nc, int Nf, void* stream) {
    // the rules of the two entry points above, with the sampler's limits
    if (Nf < 0 || capacity < 1) return NERF_AMD_EINVAL;
    if (!(flags & NERF_AMD_DEVICE_RNG) && !u_f && Nf > 0) return NERF_AMD_EINVAL;
    int rc = masked_rays_check(rays, u, tbins, flags, B, Nc, nerf_pdf::unsupported_sizes(Nc, Nf));
    if (!rc) rc = capped_check(mask, offsets, capacity, B, Nc);
    if (rc) return rc;
    if (!raw_live || !gt || !rgb || !d_raw_live || !ts_out || misaligned(raw_live, 16) || misaligned(d_raw_live, 16) ||
        misaligned(gt, 4) || misaligned(rgb, 4) || misaligned(ts_out, 4) || misaligned(u_f, 4))
        return NERF_AMD_EINVAL;
    const MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, Nc);
    MaskedBackwardArgs b = capped_head_args(raw_live, mask, offsets, gt, rgb, d_raw_live, capacity, B);
    b.u_f = u_f; b.ts_out = ts_out; b.Nf = Nf;
    return nerf_amd_launch_masked_backward(&a, &b, reinterpret_cast<hipStream_t>(stream));
}
