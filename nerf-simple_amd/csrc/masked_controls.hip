// masked_controls.hip -- the training controls of the dense path (background colour, noise on the raw density, distortion
// loss; composite_bg.hip, composite_dist.hip, composite_head.hip) for the MASKED single-network steps: the noise stage on the
// live rows, and the entry point of the masked training head with any of the three terms in one launch under the capacity
// clamp.  Not in the reference.  include/nerf_amd.h, "masked training controls"; DESIGN.md section 32.
//
//   sigma_noise_masked_kernel<NOISE> -- raw_live[P',4] -> out[P',4].  One wavefront per ray, lane = ORIGINAL sample index,
//       row = offsets[ray] + rank, rank from popcounts of the mask words (as emit_ray_rows, occ_scan_device.h): the colours
//       copied, sigma' = noisy_sigma(sigma, std, key, (ray_id0 + ray) N + i) (sigma_noise_device.h, the one definition).  The
//       counter is the original sample index, so a live sample draws what nerf_amd_sigma_noise gives that sample in the dense
//       raw[B,N,4].  A row is read and written by the same lane: out may be raw_live.  NOISE = false: the copy alone.
//   the head -- masked_backward_kernel<LossHead<BG, DIST, false>, NOISE, 0> (occupancy_train.hip, the one walk of every
//       masked backward and head); this source holds its entry point, which fills the terms' fields of MaskedBackwardArgs.
//
//   the coarse head of the masked pair -- the same walk with the sampler behind it, masked_backward_kernel<LossHead<BG, false,
//       false>, NOISE, E> (occupancy_train.hip likewise); its entry point is the last one below.
//
// No atomics; a row is written by exactly one lane, so two runs write the same bytes.  The three entry points below are the
// C ABI themselves (argument checking included, api_checks.h).
#include "sigma_noise_device.h"
#include "occ_scan_device.h"
#include "api_checks.h"
#include "launchers.h"

namespace {

constexpr int MAX_N = nerf_layout::COMPOSITE_BWD_MAX_N;                    // N <= 512, the masked head's limit

template <bool NOISE>
__global__ __launch_bounds__(MASKED_THREADS) void sigma_noise_masked_kernel(const f32x4* raw, f32x4* out, float std,
                                                                            unsigned long long seed,
                                                                            const unsigned long long* seed_mem, long long ray_id0,
                                                                            const unsigned long long* __restrict__ mask,
                                                                            const long long* __restrict__ offsets, long long B,
                                                                            int N) {
    const long long ray = (long long)blockIdx.x * MASKED_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= B) return;
    const int lane = threadIdx.x & 63;
    long long row0 = offsets[ray];
    const long long end = offsets[ray + 1];
    if (end == row0) return;                   // nothing live on this ray
    const int words = (N + 63) >> 6;
    const unsigned long long* m = mask + ray * words;
    [[maybe_unused]] unsigned long long key = 0;
    if constexpr (NOISE) key = nerf_noise::noise_key(seed, seed_mem);
    const unsigned long long sample0 = (unsigned long long)((ray_id0 + ray) * N);
    for (int q = 0; q < words; ++q) {
        const unsigned long long mw = m[q];
        const int i = q * 64 + lane;
        const long long row = row0 + __popcll(mw & ((1ull << lane) - 1ull));
        // row < end: a mask and offsets that disagree write nothing outside the ray's own rows
        if (((mw >> lane) & 1ull) && i < N && row < end) {
            f32x4 v = raw[row];
            if constexpr (NOISE) v[3] = nerf_noise::noisy_sigma(v[3], std, key, sample0 + (unsigned long long)i);
            out[row] = v;
        }
        row0 += __popcll(mw);
    }
}

}  // namespace

extern "C" int nerf_amd_launch_sigma_noise_masked(const float* raw_live, float* out, float std, unsigned long long seed,
                                                  const unsigned long long* seed_mem, long long ray_id0,
                                                  const unsigned long long* mask, const long long* offsets, long long B, int N,
                                                  hipStream_t stream) {
    (void)hipGetLastError();
    if (B == 0 || (std == 0.f && out == raw_live)) return 0;
    if (N > MAX_N) return -2;
    const dim3 grid((unsigned)((B + MASKED_RAYS_PER_BLOCK - 1) / MASKED_RAYS_PER_BLOCK)), block(MASKED_THREADS);
    const f32x4* in4 = reinterpret_cast<const f32x4*>(raw_live);
    f32x4* out4 = reinterpret_cast<f32x4*>(out);
    if (std == 0.f)      // no noise: no noise code on the path
        hipLaunchKernelGGL(sigma_noise_masked_kernel<false>, grid, block, 0, stream, in4, out4, std, seed, seed_mem, ray_id0, mask,
                           offsets, B, N);
    else
        hipLaunchKernelGGL(sigma_noise_masked_kernel<true>, grid, block, 0, stream, in4, out4, std, seed, seed_mem, ray_id0, mask,
                           offsets, B, N);
    return (int)hipGetLastError();
}

// Order of the rules: sizes; the noise arguments (api_checks.h bad_sigma_noise); the empty problem; the size limit
// (NERF_AMD_EUNSUP); the pointers.  P' is known to the device only: NULL for both raw_live and out says P' == 0.
extern "C" int nerf_amd_sigma_noise_masked(const float* raw_live, float* out, float std, uint32_t flags, uint64_t seed,
                                           const uint64_t* seed_mem, int64_t ray_id0, const uint64_t* mask, const int64_t* offsets,
                                           int64_t B, int N, void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (bad_sigma_noise(std, flags, seed_mem)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (N > COMPOSITE_BWD_MAX_N || B > MASKED_MAX_RAYS) return NERF_AMD_EUNSUP;
    if (!mask || !offsets || misaligned(mask, 8) || misaligned(offsets, 8)) return NERF_AMD_EINVAL;
    if (!raw_live != !out || misaligned(raw_live, 16) || misaligned(out, 16)) return NERF_AMD_EINVAL;
    if (!raw_live) return 0;
    return nerf_amd_launch_sigma_noise_masked(raw_live, out, std, seed, noise_seed_mem(flags, seed_mem), ray_id0,
                                              reinterpret_cast<const unsigned long long*>(mask),
                                              reinterpret_cast<const long long*>(offsets), B, N, reinterpret_cast<hipStream_t>(stream));
}

// Order of the rules: the plain masked head's own (capacity < 1, sizes, the jitter arguments); the noise arguments; the
// background's stride; the distortion term's scalars; B == 0 (no capacity fits: 1 <= C <= B N); the size limit
// (NERF_AMD_EUNSUP); the pointers (rays, C <= B N, mask and offsets, the buffers).
extern "C" int nerf_amd_volume_render_masked_mse_backward_dist(const float* raw_live, const float* rays, const float* u,
                                                               const float* tbins, uint32_t flags, uint64_t seed, int64_t ray_id0,
                                                               const uint64_t* mask, const int64_t* offsets, const float* gt,
                                                               const float* bg, int64_t bg_stride, float std, uint32_t noise_flags,
                                                               uint64_t noise_seed, const uint64_t* seed_mem, float t_far,
                                                               float coef, float* rgb, float* loss_ray, float* d_raw_live,
                                                               int64_t capacity, int64_t B, int N, void* stream) {
    if (capacity < 1 || B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (bad_jitter(flags, u, tbins)) return NERF_AMD_EINVAL;
    if (bad_sigma_noise(std, noise_flags, seed_mem)) return NERF_AMD_EINVAL;
    if (bad_bg_stride(bg_stride)) return NERF_AMD_EINVAL;
    if (bad_distortion(t_far, coef)) return NERF_AMD_EINVAL;
    if (B == 0) return NERF_AMD_EINVAL;
    if (N > COMPOSITE_BWD_MAX_N || B > MASKED_MAX_RAYS) return NERF_AMD_EUNSUP;
    if (!rays) return NERF_AMD_EINVAL;
    const int rc = capped_check(mask, offsets, capacity, B, N);
    if (rc) return rc;
    if (!raw_live || !gt || !rgb || !d_raw_live || misaligned(raw_live, 16) || misaligned(d_raw_live, 16) ||
        misaligned(gt, 4) || misaligned(rgb, 4) || misaligned(bg, 4) || misaligned(loss_ray, 4))
        return NERF_AMD_EINVAL;
    const MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    MaskedBackwardArgs b = capped_head_args(raw_live, mask, offsets, gt, rgb, d_raw_live, capacity, B);
    b.bg = bg; b.bg_stride = bg_stride;
    b.std = std; b.noise_seed = noise_seed;
    b.seed_mem = noise_seed_mem(noise_flags, seed_mem);
    b.t_far = t_far; b.coef = coef; b.loss_ray = loss_ray;
    return nerf_amd_launch_masked_backward(&a, &b, reinterpret_cast<hipStream_t>(stream));
}

// The coarse head of the masked pair behind a background and / or with noise on the live rows: the plain masked coarse head
// (occupancy_graph.hip) with the term block of the head above, the distortion term left out.  Order of
// the rules: the plain coarse head's (Nf and capacity; the sampler's uniforms; sizes; the jitter arguments), then the noise
// arguments and the background's stride, then the plain head's again (the size limit, NERF_AMD_EUNSUP; the rays; C <= B Nc,
// mask and offsets; the buffers).
extern "C" int nerf_amd_volume_render_masked_mse_backward_pdf_bg(const float* raw_live, const float* rays, const float* u,
                                                                 const float* tbins, uint32_t flags, uint64_t seed,
                                                                 int64_t ray_id0, const uint64_t* mask, const int64_t* offsets,
                                                                 const float* gt, const float* bg, int64_t bg_stride, float std,
                                                                 uint32_t noise_flags, uint64_t noise_seed,
                                                                 const uint64_t* seed_mem, const float* u_f, float* rgb,
                                                                 float* d_raw_live, float* ts_out, int64_t capacity, int64_t B,
                                                                 int Nc, int Nf, void* stream) {
    if (Nf < 0 || capacity < 1) return NERF_AMD_EINVAL;
    if (!(flags & NERF_AMD_DEVICE_RNG) && !u_f && Nf > 0) return NERF_AMD_EINVAL;
    if (B < 0 || Nc <= 0) return NERF_AMD_EINVAL;
    if (bad_jitter(flags, u, tbins)) return NERF_AMD_EINVAL;
    if (bad_sigma_noise(std, noise_flags, seed_mem)) return NERF_AMD_EINVAL;
    if (bad_bg_stride(bg_stride)) return NERF_AMD_EINVAL;
    if (nerf_pdf::unsupported_sizes(Nc, Nf) || B > MASKED_MAX_RAYS) return NERF_AMD_EUNSUP;
    if (B > 0 && !rays) return NERF_AMD_EINVAL;
    const int rc = capped_check(mask, offsets, capacity, B, Nc);
    if (rc) return rc;
    if (!raw_live || !gt || !rgb || !d_raw_live || !ts_out || misaligned(raw_live, 16) || misaligned(d_raw_live, 16) ||
        misaligned(gt, 4) || misaligned(rgb, 4) || misaligned(ts_out, 4) || misaligned(u_f, 4) || misaligned(bg, 4))
        return NERF_AMD_EINVAL;
    const MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, Nc);
    MaskedBackwardArgs b = capped_head_args(raw_live, mask, offsets, gt, rgb, d_raw_live, capacity, B);
    b.u_f = u_f; b.ts_out = ts_out; b.Nf = Nf;
    b.bg = bg; b.bg_stride = bg_stride;
    b.std = std; b.noise_seed = noise_seed;
    b.seed_mem = noise_seed_mem(noise_flags, seed_mem);
    return nerf_amd_launch_masked_backward(&a, &b, reinterpret_cast<hipStream_t>(stream));
}
