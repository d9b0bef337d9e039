// guided_sample.hip -- grid-guided fine sampling: the Nf importance samples of a ray placed from a sigma VOLUME instead of a
// coarse network (include/nerf_amd.h, "grid-guided fine sampling").  Not in the reference.
//
// One kernel joins four shared device routines, none of them copied or edited.  One wavefront per ray:
//   positions: the Nc coarse samples as every render forms them (nerf_device.h: fetch_point_rays) -> the wave's WaveLds::ts;
//   look-up:   volume_value (sigma_volume_device.h): the cell of each point by the occupancy rule (occ_grid_device.h:
//              floor(fl(fl(x - lo) inv_step)), outside when !(0 <= c < n - 1) or NaN) and the maximum of the cell's 8 corners
//              of V[nx, ny, nz], from -inf, NaN corners skipped; -inf outside.  No arithmetic on the values: the look-up is
//              exact.  8 plain loads per sample through the read-only path; a 128^3 volume (8 MiB) stays in L2 / MALL;
//   weights:   composite_ray (composite_device.h) over raw = (0, 0, 0, value): its `w` output is pointed at the wave's own LDS
//              slice (ray index 0, every other output NULL), so the bits are composite_ray's and w never reaches HBM;
//   sampler:   nerf_pdf::sample_ray (sample_pdf_device.h) on those positions and weights.
// No atomics, no cross-wave traffic: two runs write the same bytes.  The host wrapper below is the C ABI itself (argument
// rules: api_checks.h).
#include "composite_device.h"
#include "sample_pdf_device.h"
#include "sigma_volume_device.h"
#include "api_checks.h"
#include "launchers.h"

namespace {

constexpr int GUIDED_RAYS_PER_BLOCK = 4;
using nerf_pdf::MAXC;

template <int E>
__global__ __launch_bounds__(64 * GUIDED_RAYS_PER_BLOCK) void guided_sample_kernel(
    MlpArgs a, SigmaVolume g, const float* __restrict__ vol, const float* __restrict__ u_f, float* __restrict__ ts_out,
    float* __restrict__ sigma_c, float* __restrict__ w_c, long long B, int Nf) {
    __shared__ nerf_pdf::WaveLds<E> s_pdf[GUIDED_RAYS_PER_BLOCK];
    __shared__ float s_sigma[GUIDED_RAYS_PER_BLOCK][MAXC];
    __shared__ float s_w[GUIDED_RAYS_PER_BLOCK][MAXC];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * GUIDED_RAYS_PER_BLOCK + wv;
    if (ray >= B) return;                      // whole wave leaves together; only wave-local LDS below, no workgroup barrier
    const int Nc = a.N;
    nerf_pdf::WaveLds<E>& s = s_pdf[wv];
    for (int i = lane; i < Nc; i += 64) {
        const PointIn pt = fetch_point_rays<false>(a, ray * Nc + i, RaySample{ray, i});
        const float v = volume_value(g, vol, pt.x, pt.y, pt.z);
        s.ts[i] = pt.t;
        s_sigma[wv][i] = v;
        if (sigma_c) sigma_c[ray * Nc + i] = v;
    }
    wave_lds_fence();
    const float* d = a.rays + ray * 6 + 3;
    const float dnorm = nerf_composite::unit_dir_norm(d[0], d[1], d[2], true);
    // the compositor's forward sweep; its w goes to this wave's LDS slice (ray index 0 of a [1, Nc] output)
    const nerf_composite::RayOut o{nullptr, nullptr, nullptr, nullptr, s_w[wv], nullptr};
    nerf_composite::composite_ray(VolumeSamples{s.ts, s_sigma[wv]}, Nc, lane, dnorm, 0, o);
    // the sweep's stores went through a generic pointer: wait on both counters before the wave's hand-over
    __builtin_amdgcn_s_waitcnt(0);
    wave_lds_fence();
    if (w_c)
        for (int i = lane; i < Nc; i += 64) w_c[ray * Nc + i] = s_w[wv][i];
    const unsigned long long seed = effective_seed(a);          // with SEED_IN_MEMORY: seed + the 64-bit offset at `u`, for both draws
    nerf_pdf::sample_ray<E>(s, s_w[wv], Nc, Nf, lane, u_f, (a.flags & NERF_FLAG_DEVICE_RNG) != 0, seed, a.ray_id0, ray,
                            ts_out + ray * (Nc + Nf));
}

}  // namespace

extern "C" int nerf_amd_launch_sample_pdf_volume(const MlpArgs* args, const float* volume, long long nx, long long ny, long long nz,
                                                 const float* h_lo, const float* h_inv_step, const float* u_f, float* ts_out,
                                                 float* sigma_c, float* w_c, int Nf, hipStream_t stream) {
    (void)hipGetLastError();
    const int Nc = args->N;
    const long long B = args->P / Nc;
    if (B == 0) return 0;
    if (Nf < 0 || nerf_pdf::unsupported_sizes(Nc, Nf) || nx < 2 || ny < 2 || nz < 2) return -2;
    const SigmaVolume g = sigma_volume_args(nx, ny, nz, h_lo, h_inv_step);
    const dim3 grid((unsigned)((B + GUIDED_RAYS_PER_BLOCK - 1) / GUIDED_RAYS_PER_BLOCK)), block(64 * GUIDED_RAYS_PER_BLOCK);
    // keys per lane of the register sort: ceil_pow2(Nf) / 64
    nerf_pdf::with_keys_per_lane(Nf, [&](auto e) {
        hipLaunchKernelGGL(guided_sample_kernel<e()>, grid, block, 0, stream, *args, g, volume, u_f, ts_out, sigma_c, w_c, B, Nf);
    });
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_sample_pdf_volume(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed,
                                          int64_t ray_id0, const float* sigma_volume, int64_t nx, int64_t ny, int64_t nz,
                                          const float* h_lo, const float* h_inv_step, const float* u_f, float* ts_out,
                                          float* sigma_c, float* w_c, int64_t B, int Nc, int Nf, void* stream) {
    if (Nf < 0) return NERF_AMD_EINVAL;
    // the rays and jitter rules of the masked stages (the kernel forms the coarse positions itself); sizes: the sampler's
    const int rc = masked_rays_check(rays, u, tbins, flags, B, Nc, nerf_pdf::unsupported_sizes(Nc, Nf));
    if (rc) return rc;
    if (nx < 2 || ny < 2 || nz < 2) return NERF_AMD_EINVAL;
    if (!(flags & NERF_AMD_DEVICE_RNG) && !u_f && Nf > 0) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!sigma_volume || !h_lo || !h_inv_step || !ts_out) return NERF_AMD_EINVAL;
    if (misaligned(rays, 4) || misaligned(u, 4) || misaligned(tbins, 4) || misaligned(sigma_volume, 4) || misaligned(u_f, 4) ||
        misaligned(ts_out, 4) || misaligned(sigma_c, 4) || misaligned(w_c, 4))
        return NERF_AMD_EINVAL;
    const MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, Nc);
    return nerf_amd_launch_sample_pdf_volume(&a, sigma_volume, nx, ny, nz, h_lo, h_inv_step, u_f, ts_out, sigma_c, w_c, Nf,
                                             reinterpret_cast<hipStream_t>(stream));
}
