// sample_pdf.hip -- hierarchical ("fine") sample placement for BASELINE config 4
// (64 coarse + 128 importance samples).  ABSENT from the reference
// (README.md:3, configs/lego.yaml:7, utils/nets.py:45-49): parity UNPINNED; this
// follows the NeRF paper's sample_pdf (inverse-CDF sampling of the coarse
// weights' interior bins) and is checked against oracle/nerf_oracle.sample_pdf.
//
// The per-ray body (bin edges, cdf scan, inverse cdf, register bitonic sort of the new positions, merge
// by rank) is sample_pdf_device.h, shared with the coarse training head (composite.hip); this file is
// the stand-alone launch: positions and weights read from HBM.  The first version sorted all 512 padded
// slots through LDS: 45 stages x 8 exchanges per lane, 26 us per ray; the register sort is ~6x faster.
// Nc <= 256, Nf <= 512, Nc + Nf <= 512.
#include "sample_pdf_device.h"
#include "launchers.h"

namespace {

constexpr int RPB = 4;            // rays (waves) per block
using nerf_pdf::MAXC;
using nerf_pdf::MAXM;

template <int E>
__global__ __launch_bounds__(64 * RPB) void sample_pdf_kernel(
    const float* __restrict__ ts, const float* __restrict__ w, const float* __restrict__ u,
    float* __restrict__ out, long long B, int Nc, int Nf, unsigned long long seed, long long ray_id0,
    int device_rng) {
    __shared__ nerf_pdf::WaveLds<E> s_wave[RPB];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * RPB + wv;
    if (ray >= B) return;                              // wave-uniform; only wave-local LDS is used
    nerf_pdf::WaveLds<E>& s = s_wave[wv];
    const float* rts = ts + ray * Nc;
    for (int i = lane; i < Nc; i += 64) s.ts[i] = rts[i];
    wave_lds_fence();
    nerf_pdf::sample_ray<E>(s, w + ray * Nc, Nc, Nf, lane, u, device_rng != 0, seed, ray_id0, ray, out + ray * (Nc + Nf));
}

}  // namespace

extern "C" int nerf_amd_launch_sample_pdf(const float* ts, const float* w, const float* u, float* out,
                                          long long B, int Nc, int Nf, unsigned long long seed,
                                          long long ray_id0, int device_rng, hipStream_t stream) {
    (void)hipGetLastError();
    if (B == 0) return 0;
    if (Nf < 0 || nerf_pdf::unsupported_sizes(Nc, Nf)) return -2;
    const dim3 grid((unsigned)((B + RPB - 1) / RPB)), block(64 * RPB);
    // keys per lane of the register sort: ceil_pow2(Nf) / 64
    nerf_pdf::with_keys_per_lane(Nf, [&](auto e) {
        hipLaunchKernelGGL(sample_pdf_kernel<e()>, grid, block, 0, stream, ts, w, u, out, B, Nc, Nf, seed, ray_id0, device_rng);
    });
    return (int)hipGetLastError();
}
