// guided_masked.hip -- grid-guided fine sampling THROUGH an occupancy grid: the masked guided placement (include/nerf_amd.h,
// "masked guided placement").  Not in the reference.
//
// The guided sampler (guided_sample.hip) with the grid looked at twice, in the kernel where the positions already sit in LDS.
// One wavefront per ray, every device routine shared, none copied or edited:
//   positions: the Nc coarse samples as every render forms them (nerf_device.h: fetch_point_rays) -> the wave's WaveLds::ts;
//   look-up:   volume_value (sigma_volume_device.h) of each point, and sample_live (occ_grid_device.h) of the SAME point: a dead
//              coarse sample gets the value -inf in front of the weights -- the rule of the masked pair, "the sampler sees
//              weights that are exactly 0 at a dead sample";
//   weights:   composite_ray (composite_device.h) over raw = (0, 0, 0, value) into the wave's own LDS slice, as guided_sample.hip;
//   sampler:   nerf_pdf::sample_ray (sample_pdf_device.h), which leaves the merged positions in WaveLds::all;
//   mark:      the merged positions once more, through the mark kernel's own body (mark_ray, occ_grid_device.h): the point as
//              fetch_point_rays forms it from a given position (add_rn(o, mul_rn(d, t)) per axis), sample_live, one ballot per 64
//              samples -> mask[B, ceil((Nc + Nf) / 64)] and the ray's live count at the head of the scan workspace (occ_ws_counts).
// The exclusive scan of the counts is occupancy.hip's (nerf_amd_launch_occ_scan).  No atomics, no cross-wave traffic: two runs
// write the same bytes.  The host wrapper below is the C ABI itself (argument rules: api_checks.h).
#include "composite_device.h"
#include "sample_pdf_device.h"
#include "sigma_volume_device.h"
#include "occ_grid_device.h"
#include "occ_scan_device.h"
#include "api_checks.h"
#include "launchers.h"

namespace {

using nerf_pdf::MAXC;

template <int E>
__global__ __launch_bounds__(MASKED_THREADS) void guided_masked_kernel(
    MlpArgs a, SigmaVolume g, const float* __restrict__ vol, OccGrid og, const float* __restrict__ u_f, float* __restrict__ ts_out,
    float* __restrict__ sigma_c, float* __restrict__ w_c, unsigned long long* __restrict__ mask, int* __restrict__ counts,
    long long B, int Nf) {
    __shared__ nerf_pdf::WaveLds<E> s_pdf[MASKED_RAYS_PER_BLOCK];
    __shared__ float s_sigma[MASKED_RAYS_PER_BLOCK][MAXC];
    __shared__ float s_w[MASKED_RAYS_PER_BLOCK][MAXC];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * MASKED_RAYS_PER_BLOCK + wv;
    if (ray >= B) return;                      // whole wave leaves together; only wave-local LDS below, no workgroup barrier
    const int Nc = a.N;
    nerf_pdf::WaveLds<E>& s = s_pdf[wv];
    for (int i = lane; i < Nc; i += 64) {
        const PointIn pt = fetch_point_rays<false>(a, ray * Nc + i, RaySample{ray, i});
        float v = volume_value(g, vol, pt.x, pt.y, pt.z);
        if (!sample_live(og, pt.x, pt.y, pt.z)) v = -__builtin_inff();         // a dead coarse sample weighs exactly 0
        s.ts[i] = pt.t;
        s_sigma[wv][i] = v;
        if (sigma_c) sigma_c[ray * Nc + i] = v;
    }
    wave_lds_fence();
    // the compositor's forward sweep; its w goes to this wave's LDS slice (ray index 0 of a [1, Nc] output)
    const nerf_composite::RayOut o{nullptr, nullptr, nullptr, nullptr, s_w[wv], nullptr};
    nerf_composite::composite_ray(VolumeSamples{s.ts, s_sigma[wv]}, Nc, lane, ray_dnorm(a, ray), 0, o);
    // the sweep's stores went through a generic pointer: wait on both counters before the wave's hand-over
    __builtin_amdgcn_s_waitcnt(0);
    wave_lds_fence();
    if (w_c)
        for (int i = lane; i < Nc; i += 64) w_c[ray * Nc + i] = s_w[wv][i];
    const unsigned long long seed = effective_seed(a);          // with SEED_IN_MEMORY: seed + the 64-bit offset at `u`, for both draws
    const int M = Nc + Nf;
    nerf_pdf::sample_ray<E>(s, s_w[wv], Nc, Nf, lane, u_f, (a.flags & NERF_FLAG_DEVICE_RNG) != 0, seed, a.ray_id0, ray,
                            ts_out + ray * M);
    // the mark of the merged positions (sample_ray fenced WaveLds::all behind its last write): the values ts_out holds
    const float* r6 = a.rays + ray * 6;
    const float ox = r6[0], oy = r6[1], oz = r6[2], dx = r6[3], dy = r6[4], dz = r6[5];
    mark_ray(og, M, lane,
             [&](int i) {
                 const float t = s.all[i];
                 return make_float3(add_rn(ox, mul_rn(dx, t)), add_rn(oy, mul_rn(dy, t)), add_rn(oz, mul_rn(dz, t)));
             },
             mask + ray * ((M + 63) >> 6), counts + ray);
}

}  // namespace

extern "C" int nerf_amd_launch_sample_pdf_volume_masked(const MlpArgs* args, const float* volume, long long vx, long long vy,
                                                        long long vz, const float* v_lo, const float* v_inv_step,
                                                        const unsigned* bits, long long gx, long long gy, long long gz,
                                                        const float* g_lo, const float* g_inv_step, int outside_live,
                                                        const float* u_f, float* ts_out, float* sigma_c, float* w_c,
                                                        unsigned long long* mask, long long* offsets, long long* live, void* ws,
                                                        int Nf, hipStream_t stream) {
    (void)hipGetLastError();
    const int Nc = args->N;
    const long long B = args->P / Nc;
    if (Nf < 0 || nerf_pdf::unsupported_sizes(Nc, Nf) || vx < 2 || vy < 2 || vz < 2 || gx < 2 || gy < 2 || gz < 2) return -2;
    if (B > 0) {
        const SigmaVolume g = sigma_volume_args(vx, vy, vz, v_lo, v_inv_step);
        const OccGrid og = occ_grid_args(bits, gx, gy, gz, g_lo, g_inv_step, outside_live);
        int* counts = occ_ws_counts(ws);
        const dim3 grid((unsigned)((B + MASKED_RAYS_PER_BLOCK - 1) / MASKED_RAYS_PER_BLOCK)), block(MASKED_THREADS);
        // keys per lane of the register sort: ceil_pow2(Nf) / 64
        nerf_pdf::with_keys_per_lane(Nf, [&](auto e) {
            hipLaunchKernelGGL(guided_masked_kernel<e()>, grid, block, 0, stream, *args, g, volume, og, u_f, ts_out, sigma_c, w_c,
                               mask, counts, B, Nf);
        });
    }
    return nerf_amd_launch_occ_scan(ws, offsets, live, B, stream);
}

extern "C" int nerf_amd_sample_pdf_volume_masked(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed,
                                                 int64_t ray_id0, const float* sigma_volume, int64_t vx, int64_t vy, int64_t vz,
                                                 const float* v_lo, const float* v_inv_step, const uint32_t* bits, int64_t gx,
                                                 int64_t gy, int64_t gz, const float* g_lo, const float* g_inv_step,
                                                 const float* u_f, float* ts_out, float* sigma_c, float* w_c, uint64_t* mask,
                                                 int64_t* offsets, int64_t* live, void* workspace, int64_t B, int Nc, int Nf,
                                                 void* stream) {
    const uint32_t jflags = flags & ~NERF_AMD_OUTSIDE_EMPTY;
    // 1. nerf_amd_sample_pdf_volume's rules, in its order
    if (Nf < 0) return NERF_AMD_EINVAL;
    const int rc = masked_rays_check(rays, u, tbins, jflags, B, Nc, nerf_pdf::unsupported_sizes(Nc, Nf));
    if (rc) return rc;
    if (vx < 2 || vy < 2 || vz < 2) return NERF_AMD_EINVAL;
    if (!(jflags & NERF_AMD_DEVICE_RNG) && !u_f && Nf > 0) return NERF_AMD_EINVAL;
    // 2. the grid's axes
    if (gx < 2 || gy < 2 || gz < 2) return NERF_AMD_EINVAL;
    // 3. the empty problem: offsets[0] = 0 (and *live = 0) as nerf_amd_occupancy_mark leaves them, where there is room for them
    if (B == 0) {
        if (!offsets || !workspace || misaligned(offsets, 8) || misaligned(live, 8) || misaligned(workspace, 16)) return 0;
        return nerf_amd_launch_occ_scan(workspace, reinterpret_cast<long long*>(offsets), reinterpret_cast<long long*>(live), 0,
                                        reinterpret_cast<hipStream_t>(stream));
    }
    // 4. the buffers
    if (!sigma_volume || !v_lo || !v_inv_step || !bits || !g_lo || !g_inv_step || !ts_out || !mask || !offsets || !workspace)
        return NERF_AMD_EINVAL;
    if (misaligned(rays, 4) || misaligned(u, 4) || misaligned(tbins, 4) || misaligned(sigma_volume, 4) || misaligned(bits, 4) ||
        misaligned(u_f, 4) || misaligned(ts_out, 4) || misaligned(sigma_c, 4) || misaligned(w_c, 4) || misaligned(mask, 8) ||
        misaligned(offsets, 8) || misaligned(live, 8) || misaligned(workspace, 16))
        return NERF_AMD_EINVAL;
    const MlpArgs a = rays_args(rays, u, tbins, jflags, seed, ray_id0, B, Nc);
    return nerf_amd_launch_sample_pdf_volume_masked(
        &a, sigma_volume, vx, vy, vz, v_lo, v_inv_step, bits, gx, gy, gz, g_lo, g_inv_step, (flags & NERF_AMD_OUTSIDE_EMPTY) ? 0 : 1,
        u_f, ts_out, sigma_c, w_c, reinterpret_cast<unsigned long long*>(mask), reinterpret_cast<long long*>(offsets),
        reinterpret_cast<long long*>(live), workspace, Nf, reinterpret_cast<hipStream_t>(stream));
}
