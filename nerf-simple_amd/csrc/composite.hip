// composite.hip -- sigma -> alpha compositing along each ray: the drop-in body
// of volume_render (reference utils/rendering.py:47-85).
//
// One wavefront per ray, one sample per lane, N walked in chunks of 64 with a
// running transmittance carried between chunks.  The reference's exclusive
// cumulative PRODUCT of (1 - alpha + 1e-10) (utils/rendering.py:68; not
// exp(-cumsum)) is a wave-level inclusive product scan (6 shuffle steps)
// shifted by one lane.  fp32 throughout, literal formulas: softplus(beta=1,
// threshold=20), last delta = 1e10, deltas scaled by ||dirs||, second output is
// DISPARITY 1/max(1e-10, depth/acc) with torch.max's NaN propagation (acc == 0
// gives NaN exactly like the reference).
//
// 20 B read per sample (+8 B written when alpha / w are requested) and 20 B written per ray.
// Not HBM-bound in practice: the exact-fp32 softplus / exp (ocml expf, log1pf) and the two scans
// cost ~400 VALU instructions per 64 samples, which is what sets its 3.4 TB/s.
#include "composite_backward_device.h"
#include "launchers.h"
#include "sample_pdf_device.h"

namespace {

using nerf_composite::wave_sum;

constexpr int RAYS_PER_BLOCK = 4;

struct GlobalSamples {                        // the ray's samples in HBM
    const float* rts;
    const f32x4* rraw;
    __device__ __forceinline__ float t(int i) const { return rts[i]; }
    __device__ __forceinline__ f32x4 c(int i) const { return rraw[i]; }
};

__global__ __launch_bounds__(64 * RAYS_PER_BLOCK) void composite_kernel(
    const float* __restrict__ raw, const float* __restrict__ ts, const float* __restrict__ dirs,
    long long dirs_stride, float* __restrict__ rgb, float* __restrict__ disp,
    float* __restrict__ alpha, float* __restrict__ acc, float* __restrict__ w, long long B, int N,
    int normalize_dirs, float* __restrict__ pixels) {
    const long long ray = (long long)blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= B) return;                      // whole wave leaves together; no barriers below
    const int lane = threadIdx.x & 63;
    const float* d = dirs + ray * dirs_stride;
    const float dnorm = nerf_composite::unit_dir_norm(d[0], d[1], d[2], normalize_dirs != 0);
    const GlobalSamples src{ts + ray * N, reinterpret_cast<const f32x4*>(raw) + ray * N};
    nerf_composite::composite_ray(src, N, lane, dnorm, ray, nerf_composite::RayOut{rgb, disp, alpha, acc, w, pixels});
}

// ---- backward ---------------------------------------------------------------
// d loss / d nerf_outs[B,N,4] given the upstream gradients of the five outputs (NULL = zero), or with the MSE loss
// gradient formed in the kernel: the per-ray walk is composite_backward_ray (composite_backward_device.h).
constexpr int MAX_CHUNKS = nerf_layout::COMPOSITE_BWD_MAX_CHUNKS;          // N <= 512

// The coarse training head (E > 0): the same kernel also places the fine pass's samples from the weights of its
// forward sweep (sample_pdf_device.h sample_behind_walk).  The weights go from registers to the wave's LDS slice with the
// positions; the sampler reads them there after the backward sweep, so neither ts nor w is read from HBM a second time.
// The sampler's arguments (launchers.h) and the ray id of ray 0 are ONE kernel argument: as a scalar argument of its own the
// ray id would be loaded at the kernel's entry, not beside the sampler's fields, and the kernel's text would move.
struct CoarsePdf {
    DensePdfArgs args;
    long long ray_id0;
};

// E = 0: the compositor's backward alone (N <= 512), with the five upstream gradients or (mse_target != NULL) the MSE head.
// E > 0: the coarse training head (MSE head only), N = Nc <= 256 (four chunks) and Nf new samples sorted E keys per lane.
template <int E>
__global__ __launch_bounds__(64 * RAYS_PER_BLOCK) void composite_backward_kernel(
    const float* __restrict__ raw, const float* __restrict__ ts, const float* __restrict__ dirs,
    long long dirs_stride, const float* __restrict__ g_rgb, const float* __restrict__ g_disp,
    const float* __restrict__ g_alpha, const float* __restrict__ g_acc, const float* __restrict__ g_w,
    float* __restrict__ d_raw, long long B, int N, int normalize_dirs,
    const float* __restrict__ mse_target, float* __restrict__ rgb_out, float mse_scale, CoarsePdf pdf) {
    constexpr int CHUNKS = E > 0 ? nerf_pdf::MAXC / 64 : MAX_CHUNKS;
    __shared__ nerf_pdf::WaveLds<(E > 0 ? E : 1)> s_pdf[E > 0 ? RAYS_PER_BLOCK : 1];
    __shared__ float s_pdf_w[E > 0 ? RAYS_PER_BLOCK : 1][nerf_pdf::MAXC];
    const int wv = threadIdx.x >> 6;
    const long long ray = (long long)blockIdx.x * RAYS_PER_BLOCK + wv;
    if (ray >= B) return;
    const int lane = threadIdx.x & 63;
    const float* d = dirs + ray * dirs_stride;
    const float dnorm = nerf_composite::unit_dir_norm(d[0], d[1], d[2], normalize_dirs != 0);
    const nerf_composite::DenseSamples src{ts + ray * N, reinterpret_cast<const f32x4*>(raw) + ray * N};
    f32x4* rout = reinterpret_cast<f32x4*>(d_raw) + ray * N;
    if (N == 1) {
        // the reference composites an EMPTY sample axis at N == 1 (composite_device.h): no output depends on raw
        if (lane == 0) {
            rout[0] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (mse_target && rgb_out) { rgb_out[ray * 3 + 0] = 0.f; rgb_out[ray * 3 + 1] = 0.f; rgb_out[ray * 3 + 2] = 0.f; }
        }
        return;
    }
    const nerf_composite::MseHead mse{mse_target, rgb_out, mse_scale};
    if constexpr (E > 0) {
        nerf_composite::composite_backward_ray<CHUNKS>(src, mse, nerf_composite::PdfSink{s_pdf[wv].ts, s_pdf_w[wv]}, N, lane, dnorm,
                                                       ray, rout);
        nerf_pdf::sample_behind_walk<E>(s_pdf[wv], s_pdf_w[wv], N, lane, pdf.args, pdf.ray_id0, ray);
    } else if (mse_target) {
        nerf_composite::composite_backward_ray<CHUNKS>(src, mse, nerf_composite::NoSink{}, N, lane, dnorm, ray, rout);
    } else {
        nerf_composite::composite_backward_ray<CHUNKS>(src, nerf_composite::FiveGrads{g_rgb, g_disp, g_alpha, g_acc, g_w},
                                                       nerf_composite::NoSink{}, N, lane, dnorm, ray, rout);
    }
}

// ---- MSELoss(pred, target) and its gradient (reference train.py:52: mean over all n elements) ----
// One workgroup, fixed summation order: the loss is bit-reproducible from run to run.
__global__ __launch_bounds__(1024) void mse_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                        float* __restrict__ loss, float* __restrict__ g_pred, long long n) {
    __shared__ float red[16];
    const float inv_n = 1.0f / (float)n;
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += 1024) {
        const float d = pred[i] - target[i];
        s += d * d;
        if (g_pred) g_pred[i] = 2.0f * d * inv_n;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int k = 0; k < 16; ++k) t += red[k];
        *loss = t * inv_n;
    }
}

}  // namespace

extern "C" int nerf_amd_launch_composite_backward(const float* raw, const float* ts, const float* dirs,
                                                  long long dirs_stride, const float* g_rgb,
                                                  const float* g_disp, const float* g_alpha,
                                                  const float* g_acc, const float* g_w, float* d_raw,
                                                  long long B, int N, int normalize_dirs, hipStream_t stream) {
    (void)hipGetLastError();
    if (B == 0) return 0;
    if (N > nerf_layout::COMPOSITE_BWD_MAX_N) return -2;
    const long long blocks = (B + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK;
    hipLaunchKernelGGL(composite_backward_kernel<0>, dim3((unsigned)blocks), dim3(64 * RAYS_PER_BLOCK), 0, stream,
                       raw, ts, dirs, dirs_stride, g_rgb, g_disp, g_alpha, g_acc, g_w, d_raw, B, N,
                       normalize_dirs, nullptr, nullptr, 0.f, CoarsePdf{});
    return (int)hipGetLastError();
}

// training form: compositing forward + MSELoss gradient + compositing backward in one launch
extern "C" int nerf_amd_launch_composite_mse_backward(const float* raw, const float* ts, const float* rays,
                                                      const float* target, float* rgb, float* d_raw, long long B,
                                                      int N, hipStream_t stream) {
    (void)hipGetLastError();
    if (B == 0) return 0;
    if (N > nerf_layout::COMPOSITE_BWD_MAX_N) return -2;
    const long long blocks = (B + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK;
    hipLaunchKernelGGL(composite_backward_kernel<0>, dim3((unsigned)blocks), dim3(64 * RAYS_PER_BLOCK), 0, stream,
                       raw, ts, rays + 3, 6ll, nullptr, nullptr, nullptr, nullptr, nullptr, d_raw, B, N, 1,
                       target, rgb, 1.0f / (3.0f * (float)B), CoarsePdf{});
    return (int)hipGetLastError();
}

// the coarse training head: the launch above + the fine pass's sample placement (sample_pdf) in the same waves
extern "C" int nerf_amd_launch_composite_mse_backward_pdf(const float* raw, const float* ts, const float* rays,
                                                          const float* target, float* rgb, float* d_raw, const float* u,
                                                          float* ts_out, long long B, int Nc, int Nf, unsigned long long seed,
                                                          long long ray_id0, int device_rng, int seed_in_mem,
                                                          hipStream_t stream) {
    (void)hipGetLastError();
    if (B == 0) return 0;
    if (Nf < 0 || nerf_pdf::unsupported_sizes(Nc, Nf)) return -2;
    const dim3 grid((unsigned)((B + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK)), block(64 * RAYS_PER_BLOCK);
    const CoarsePdf pdf{{u, ts_out, Nf, device_rng, seed_in_mem, seed}, ray_id0};
    const float scale = 1.0f / (3.0f * (float)B);
    nerf_pdf::with_keys_per_lane(Nf, [&](auto e) {
        hipLaunchKernelGGL(composite_backward_kernel<e()>, grid, block, 0, stream, raw, ts, rays + 3, 6ll, nullptr, nullptr, nullptr,
                           nullptr, nullptr, d_raw, B, Nc, 1, target, rgb, scale, pdf);
    });
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_composite(const float* raw, const float* ts, const float* dirs,
                                         long long dirs_stride, float* rgb, float* disp, float* alpha,
                                         float* acc, float* w, long long B, int N, int normalize_dirs,
                                         float* pixels, hipStream_t stream) {
    (void)hipGetLastError();   // drop any stale error: the return value is about THIS launch
    if (B == 0) return 0;
    const long long blocks = (B + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK;
    hipLaunchKernelGGL(composite_kernel, dim3((unsigned)blocks), dim3(64 * RAYS_PER_BLOCK), 0, stream,
                       raw, ts, dirs, dirs_stride, rgb, disp, alpha, acc, w, B, N, normalize_dirs, pixels);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_mse_loss(const float* pred, const float* target, float* loss, float* g_pred, long long n,
                                        hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(mse_loss_kernel, dim3(1), dim3(1024), 0, stream, pred, target, loss, g_pred, n);
    return (int)hipGetLastError();
}
