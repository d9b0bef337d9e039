// composite_bg.hip -- the two training controls in front of and behind the dense compositor: Gaussian noise on the raw
// density (the NeRF paper's raw_noise_std; the reference's `## TODO add gaussian noise regularizer`, utils/rendering.py:63)
// and a background colour behind the volume (white_bkgd elsewhere):
//   sigma'  = sigma + std z                 in front of the softplus (sigma_noise_device.h)
//   rgb_bg  = rgb + (1 - acc) bg            two rounded ops per channel, no fma: torch's fp32 expression gives the same bits
// Three small stages (noise, blend, the blend's backward).  The training head is BY DEFINITION their composition with the
// compositor, the MSE gradient and the compositor's backward, in one launch: dense_head_kernel<NOISE, BG, .., E>
// (composite_head.hip; E > 0: the coarse head of the pair, the fine pass's sampler behind the same walk).
#include "composite_device.h"
#include "launchers.h"
#include "sigma_noise_device.h"

namespace {

// ---- the stages ----------------------------------------------------------------------------------------------------------
// raw[B,N,4] -> out[B,N,4] (out may be raw: every thread reads its own sample before it writes it): colours copied,
// column 3 = sigma'.  One thread per sample, one 16-byte load and store.
__global__ __launch_bounds__(256) void sigma_noise_kernel(const f32x4* raw, f32x4* out, float std, unsigned long long seed,
                                                          const unsigned long long* seed_mem, unsigned long long sample0,
                                                          long long P) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    f32x4 v = raw[p];
    v[3] = nerf_noise::noisy_sigma(v[3], std, nerf_noise::noise_key(seed, seed_mem), sample0 + (unsigned long long)p);
    out[p] = v;
}

__global__ __launch_bounds__(256) void copy_samples_kernel(const f32x4* raw, f32x4* out, long long P) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p < P) out[p] = raw[p];
}

// one thread per ray: rgb_out[B,3] = rgb_bg and / or pixels[B,4] = [clip(rgb_bg, 0, 1), disp] (the clip behind the blend;
// NaN passes through, as in the compositor)
__global__ __launch_bounds__(256) void background_blend_kernel(const float* __restrict__ rgb, const float* __restrict__ acc,
                                                               const float* __restrict__ disp, const float* __restrict__ bg,
                                                               long long bg_stride, float* __restrict__ rgb_out,
                                                               float* __restrict__ pixels, long long B) {
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    if (ray >= B) return;
    const float* b = bg + ray * bg_stride;
    const float through = sub_rn(1.0f, acc[ray]);
    const float r0 = add_rn(rgb[ray * 3 + 0], mul_rn(through, b[0]));
    const float r1 = add_rn(rgb[ray * 3 + 1], mul_rn(through, b[1]));
    const float r2 = add_rn(rgb[ray * 3 + 2], mul_rn(through, b[2]));
    if (rgb_out) { rgb_out[ray * 3 + 0] = r0; rgb_out[ray * 3 + 1] = r1; rgb_out[ray * 3 + 2] = r2; }
    if (pixels) {
        auto clip01 = [](float v) { return (v != v) ? v : fminf(fmaxf(v, 0.f), 1.f); };
        const f32x4 px = {clip01(r0), clip01(r1), clip01(r2), disp[ray]};
        *reinterpret_cast<f32x4*>(pixels + ray * 4) = px;
    }
}

// g_acc[B] = -((g0 bg0 + g1 bg1) + g2 bg2), WRITTEN (the caller adds its own term); g_rgb passes through untouched
__global__ __launch_bounds__(256) void background_blend_backward_kernel(const float* __restrict__ g, const float* __restrict__ bg,
                                                                        long long bg_stride, float* __restrict__ g_acc,
                                                                        long long B) {
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    if (ray >= B) return;
    const float* b = bg + ray * bg_stride;
    g_acc[ray] = -add_rn(add_rn(mul_rn(g[ray * 3 + 0], b[0]), mul_rn(g[ray * 3 + 1], b[1])), mul_rn(g[ray * 3 + 2], b[2]));
}

inline dim3 per_element(long long n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

extern "C" int nerf_amd_launch_sigma_noise(const float* raw, float* out, float std, unsigned long long seed,
                                           const unsigned long long* seed_mem, long long ray_id0, long long B, int N,
                                           hipStream_t stream) {
    (void)hipGetLastError();
    const long long P = B * N;
    if (P == 0 || (std == 0.f && out == raw)) return 0;
    if (P > (1ll << 39)) return -2;                                  // the grid's x extent
    const f32x4* in4 = reinterpret_cast<const f32x4*>(raw);
    f32x4* out4 = reinterpret_cast<f32x4*>(out);
    if (std == 0.f)      // no noise: no noise code on the path
        hipLaunchKernelGGL(copy_samples_kernel, per_element(P), dim3(256), 0, stream, in4, out4, P);
    else
        hipLaunchKernelGGL(sigma_noise_kernel, per_element(P), dim3(256), 0, stream, in4, out4, std, seed, seed_mem,
                           (unsigned long long)(ray_id0 * N), P);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_background_blend(const float* rgb, const float* acc, const float* disp, const float* bg,
                                                long long bg_stride, float* rgb_out, float* pixels, long long B,
                                                hipStream_t stream) {
    (void)hipGetLastError();
    if (B == 0) return 0;
    hipLaunchKernelGGL(background_blend_kernel, per_element(B), dim3(256), 0, stream, rgb, acc, disp, bg, bg_stride, rgb_out,
                       pixels, B);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_background_blend_backward(const float* g_rgb_bg, const float* bg, long long bg_stride,
                                                         float* g_acc, long long B, hipStream_t stream) {
    (void)hipGetLastError();
    if (B == 0) return 0;
    hipLaunchKernelGGL(background_blend_backward_kernel, per_element(B), dim3(256), 0, stream, g_rgb_bg, bg, bg_stride, g_acc, B);
    return (int)hipGetLastError();
}
