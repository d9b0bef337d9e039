// occupancy_hier.hip -- the masked COARSE head of the graphed masked hierarchical training step (include/nerf_amd.h,
// "masked hierarchical pair").  Not in the reference.
//
//   occ_head_capped_pdf_kernel<E> -- what occ_head_capped_kernel (occupancy_graph.hip) does under the capacity clamp -- masked
//       compositor forward -> g_rgb = 2 (rgb - gt) / (3 B) -> masked compositor backward -- and then, in the same wave, the
//       fine pass's sample placement (sample_pdf_device.h) from the weights of its own forward sweep, as composite.hip's
//       dense coarse head does it (the same composite_backward_ray, composite_backward_device.h, with the sampler's LDS slice
//       as its weight sink): wt = mul_rn(alpha, T) goes from registers to the wave's LDS slice beside the positions the
//       kernel has recomputed (a dead or over-capacity sample carries exactly 0), and the sampler reads both there after the
//       backward sweep.  w never reaches HBM.  The fine pass's mark depends on ts_out, so in a captured step both have to come
//       out of one node chain with no host in it; this is that node.
//
// Nc <= 256: four 64-lane chunks, E = keys per lane of the sampler's register sort (1, 2, 4, 8 by Nf).  One wavefront per
// ray, four rays per block; LDS per block 4 * (6 KB + 256 E B): 25 ... 32 KB, the dense head's figures (the positions live in
// the sampler's own ts[] slice, the mask walk is in registers).  No atomics; the kept rows and the pad rows are disjoint
// ranges, so two runs write the same bytes.  The host wrapper below is the C ABI itself (argument rules: api_checks.h).
#include "composite_backward_device.h"
#include "sample_pdf_device.h"
#include "api_checks.h"

namespace {

constexpr int OCCH_RAYS_PER_BLOCK = 4;
constexpr int OCCH_THREADS = 64 * OCCH_RAYS_PER_BLOCK;
constexpr int OCCH_CHUNKS = nerf_pdf::MAXC / 64;

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
    f32x4* rout = reinterpret_cast<f32x4*>(d_raw_live) + first;
    float* rts = s_pdf[wv].ts;                 // the positions: the compositor's and the sampler's
    float* rw = s_pdf_w[wv];
    for (int i = lane; i < N; i += 64) rts[i] = fetch_point_rays<false>(a, ray * N + i, RaySample{ray, i}).t;
    wave_lds_fence();
    if (n_kept <= 0) {
        // nothing kept: every sample is (0, 0, 0, -inf), w = 0 throughout: rgb = 0, no row to write, and the sampler's
        // 1e-5 floor spreads the new samples uniformly
        if (lane == 0) { rgb_out[ray * 3 + 0] = 0.f; rgb_out[ray * 3 + 1] = 0.f; rgb_out[ray * 3 + 2] = 0.f; }
        for (int i = lane; i < N; i += 64) rw[i] = 0.f;
    } else {
        const float* d = a.rays + ray * 6 + 3;
        const float dnorm = nerf_composite::unit_dir_norm(d[0], d[1], d[2], true);
        const nerf_composite::MaskedSamplesBwd src{rts, m, reinterpret_cast<const f32x4*>(raw_live) + first, n_kept};
        // loss = MSELoss(rgb, gt) (train.py:52): only rgb feeds it; the weights go to the sampler, exactly 0 at a dead sample
        nerf_composite::composite_backward_ray<OCCH_CHUNKS>(src, nerf_composite::MseHead{gt, rgb_out, mse_scale},
                                                            nerf_composite::PdfSink{nullptr, rw}, N, lane, dnorm, ray, rout);
    }
    // the fine pass's positions from this ray's weights (nerf_amd_sample_pdf's body, same draws)
    wave_lds_fence();
    nerf_pdf::sample_ray<E>(s_pdf[wv], rw, N, pdf.Nf, lane, pdf.u_f, (a.flags & NERF_FLAG_DEVICE_RNG) != 0, effective_seed(a), a.ray_id0,
                            ray, pdf.ts_out + ray * (long long)(N + pdf.Nf));
}

}  // namespace

extern "C" int nerf_amd_volume_render_masked_mse_backward_pdf(const float* raw_live, const float* rays, const float* u,
                                                              const float* tbins, uint32_t flags, uint64_t seed, int64_t ray_id0,
                                                              const uint64_t* mask, const int64_t* offsets, const float* gt,
                                                              const float* u_f, float* rgb, float* d_raw_live, float* ts_out,
                                                              int64_t capacity, int64_t B, int Nc, int Nf, void* stream) {
    // the rules of the two section-14 entry points (occupancy_graph.hip), with the sampler's limits
    if (Nf < 0 || capacity < 1) return NERF_AMD_EINVAL;
    if (!(flags & NERF_AMD_DEVICE_RNG) && !u_f && Nf > 0) return NERF_AMD_EINVAL;
    int rc = masked_rays_check(rays, u, tbins, flags, B, Nc, nerf_pdf::unsupported_sizes(Nc, Nf));
    if (!rc) rc = capped_check(mask, offsets, capacity, B, Nc);
    if (rc) return rc;
    if (!raw_live || !gt || !rgb || !d_raw_live || !ts_out || misaligned(raw_live, 16) || misaligned(d_raw_live, 16) ||
        misaligned(gt, 4) || misaligned(rgb, 4) || misaligned(ts_out, 4) || misaligned(u_f, 4))
        return NERF_AMD_EINVAL;
    (void)hipGetLastError();
    const MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, Nc);
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
