// composite_bg.hip -- the two training controls in front of and behind the dense compositor: Gaussian noise on the raw
// density (the NeRF paper's raw_noise_std; the reference's `## TODO add gaussian noise regularizer`, utils/rendering.py:63)
// and a background colour behind the volume (white_bkgd elsewhere):
//   sigma'  = sigma + std z                 in front of the softplus (sigma_noise_device.h)
//   rgb_bg  = rgb + (1 - acc) bg            two rounded ops per channel, no fma: torch's fp32 expression gives the same bits
// Three small stages (noise, blend, the blend's backward) and the training head, which is BY DEFINITION their composition
// with the compositor, the MSE gradient and the compositor's backward, in one launch on composite_backward_ray.
#include "composite_backward_device.h"
#include "launchers.h"
#include "sigma_noise_device.h"

namespace {

constexpr int RAYS_PER_BLOCK = 4;
constexpr int MAX_CHUNKS = nerf_layout::COMPOSITE_BWD_MAX_CHUNKS;          // N <= 512

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

// ---- the training head (its noisy sample source: sigma_noise_device.h NoisySamples) ---------------------------------------
// NOISE: sigma' in front of the softplus; BG: the loss sits behind the blend.  (false, false) is composite_backward_kernel<0>
// with the MSE head (composite.hip) and is not instantiated here.
template <bool NOISE, bool BG>
__global__ __launch_bounds__(64 * RAYS_PER_BLOCK) void composite_bg_head_kernel(
    const float* __restrict__ raw, const float* __restrict__ ts, const float* __restrict__ rays,
    const float* __restrict__ target, const float* __restrict__ bg, long long bg_stride, float std, unsigned long long seed,
    const unsigned long long* __restrict__ seed_mem, long long ray_id0, float* __restrict__ rgb_out,
    float* __restrict__ d_raw, long long B, int N, float scale) {
    const long long ray = (long long)blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= B) return;                      // whole wave leaves together; no barriers below
    const int lane = threadIdx.x & 63;
    f32x4* rout = reinterpret_cast<f32x4*>(d_raw) + ray * N;
    if (N == 1) {
        // the reference composites an EMPTY sample axis at N == 1 (composite_device.h): rgb = acc = 0, so rgb_bg = bg exactly
        if (lane == 0) {
            rout[0] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (rgb_out) {
                for (int c = 0; c < 3; ++c) rgb_out[ray * 3 + c] = BG ? add_rn(0.f, mul_rn(sub_rn(1.0f, 0.f), bg[ray * bg_stride + c])) : 0.f;
            }
        }
        return;
    }
    const float* d = rays + ray * 6 + 3;
    const float dnorm = nerf_composite::unit_dir_norm(d[0], d[1], d[2], true);
    const nerf_composite::DenseSamples dense{ts + ray * N, reinterpret_cast<const f32x4*>(raw) + ray * N};
    auto run = [&](auto src) {
        if constexpr (BG) {
            nerf_composite::composite_backward_ray<MAX_CHUNKS>(src, nerf_composite::BgMseHead{target, rgb_out, scale, bg, bg_stride},
                                                               nerf_composite::NoSink{}, N, lane, dnorm, ray, rout);
        } else {
            nerf_composite::composite_backward_ray<MAX_CHUNKS>(src, nerf_composite::MseHead{target, rgb_out, scale},
                                                               nerf_composite::NoSink{}, N, lane, dnorm, ray, rout);
        }
    };
    if constexpr (NOISE) {
        run(nerf_noise::NoisySamples{dense, std, nerf_noise::noise_key(seed, seed_mem), (unsigned long long)((ray_id0 + ray) * N)});
    } else {
        run(dense);
    }
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

// bg == NULL and std == 0: the plain head's launch itself (composite.hip)
extern "C" int nerf_amd_launch_composite_mse_backward_bg(const float* raw, const float* ts, const float* rays,
                                                         const float* target, const float* bg, long long bg_stride, float std,
                                                         unsigned long long seed, const unsigned long long* seed_mem,
                                                         long long ray_id0, float* rgb, float* d_raw, long long B, int N,
                                                         hipStream_t stream) {
    if (!bg && std == 0.f) return nerf_amd_launch_composite_mse_backward(raw, ts, rays, target, rgb, d_raw, B, N, stream);
    (void)hipGetLastError();
    if (B == 0) return 0;
    if (N > nerf_layout::COMPOSITE_BWD_MAX_N) return -2;
    const dim3 grid((unsigned)((B + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK)), block(64 * RAYS_PER_BLOCK);
    const float scale = 1.0f / (3.0f * (float)B);
#define NERF_BG_HEAD(NOISE_, BG_)                                                                                          \
    hipLaunchKernelGGL((composite_bg_head_kernel<NOISE_, BG_>), grid, block, 0, stream, raw, ts, rays, target, bg, bg_stride, \
                       std, seed, seed_mem, ray_id0, rgb, d_raw, B, N, scale)
    if (std == 0.f) NERF_BG_HEAD(false, true);
    else if (!bg) NERF_BG_HEAD(true, false);
    else NERF_BG_HEAD(true, true);
#undef NERF_BG_HEAD
    return (int)hipGetLastError();
}
