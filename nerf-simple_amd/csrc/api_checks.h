// api_checks.h -- host-side argument rules shared by the sources that implement the C ABI (include/nerf_amd.h): api.hip and
// the self-contained entry points in occupancy_graph.hip and occupancy_terminate.hip.  Host code only.
// Each limit and each rule that more than one entry point applies is stated here once (the limits a kernel's static sizes
// depend on: nerf_layout.h, sample_pdf_device.h); an entry point chooses the ORDER in which it applies them, and that order
// is part of the ABI (tests/test_abi_refusals_cpu.py).
#pragma once
#include "nerf_device.h"
#include "sample_pdf_device.h"
#include "launchers.h"
#include "../../include/nerf_amd.h"

using nerf_layout::align256;
using nerf_layout::COMPOSITE_BWD_MAX_N;          // N of the four compositor backward entry points and the capped heads
using nerf_layout::MASKED_MAX_N;                 // N of the masked render and of ray termination
constexpr int64_t MASKED_MAX_RAYS = 1ll << 32;   // B of every masked, capped and terminated entry point
// the sampler's merged positions feed the fine pass: its fused render and its compositor backward
static_assert(nerf_pdf::MAXM <= nerf_layout::FUSED_RENDER_MAX_N && nerf_pdf::MAXM <= COMPOSITE_BWD_MAX_N, "fine pass sizes");

inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// the jitter arguments of every rays-mode entry point: explicit u / ts, the counter RNG, or the counter RNG with its seed
// offset in device memory (then `u` is that address).  With TS_GIVEN the kernels read the positions through `u` whatever
// the other flags say, so `u` is required then.
// (`used`: emitted whether or not every call is inlined, so the library's symbol table does not depend on the inliner)
__attribute__((used)) inline bool bad_jitter(uint32_t flags, const float* u, const float* tbins) {
    if (flags & ~(NERF_AMD_TS_GIVEN | NERF_AMD_DEVICE_RNG | NERF_AMD_SEED_IN_MEMORY)) return true;     // unknown bits
    if (flags & NERF_AMD_SEED_IN_MEMORY) {
        if (!(flags & NERF_AMD_DEVICE_RNG) || (flags & NERF_AMD_TS_GIVEN) || !u) return true;
        if (misaligned(u, 8)) return true;                                     // the kernels load it as one 64-bit word
    } else if ((!(flags & NERF_AMD_DEVICE_RNG) || (flags & NERF_AMD_TS_GIVEN)) && !u) {
        return true;
    }
    return !(flags & NERF_AMD_TS_GIVEN) && !tbins;
}

// the sigma-noise arguments (nerf_amd_sigma_noise, nerf_amd_volume_render_mse_backward_bg): std finite and >= 0; the only flag
// is NERF_AMD_SEED_IN_MEMORY, and with it `seed_mem` is the 8-byte aligned device address of the step offset (without it
// `seed_mem` is not looked at).  Applied whatever std is: std == 0 launches no noise code but the call is still checked.
inline bool bad_sigma_noise(float std, uint32_t flags, const uint64_t* seed_mem) {
    if (!(std >= 0.f) || std > 3.402823466e38f) return true;                   // negative, NaN, inf
    if (flags & ~NERF_AMD_SEED_IN_MEMORY) return true;
    return (flags & NERF_AMD_SEED_IN_MEMORY) && (!seed_mem || misaligned(seed_mem, 8));
}
// the step offset a noise launch reads: `seed_mem` with NERF_AMD_SEED_IN_MEMORY, nothing without it
inline const unsigned long long* noise_seed_mem(uint32_t flags, const uint64_t* seed_mem) {
    return (flags & NERF_AMD_SEED_IN_MEMORY) ? reinterpret_cast<const unsigned long long*>(seed_mem) : nullptr;
}
// the jitter arguments of the dense coarse heads' sampler (nerf_amd_volume_render_mse_backward_pdf, .._pdf_bg): the uniforms
// u[B, Nf], the counter RNG, or the counter RNG with its seed offset in device memory (then `u` is that 8-byte aligned address,
// the graphed step's hyper vector).  No positions are given and no bins are needed, unlike bad_jitter.
inline bool bad_pdf_jitter(uint32_t flags, const float* u, int Nf) {
    if (flags & ~(NERF_AMD_DEVICE_RNG | NERF_AMD_SEED_IN_MEMORY)) return true;
    if (flags & NERF_AMD_SEED_IN_MEMORY) return !(flags & NERF_AMD_DEVICE_RNG) || !u || misaligned(u, 8);
    return !(flags & NERF_AMD_DEVICE_RNG) && !u && Nf > 0;
}
// the distortion term's scalars (nerf_amd_distortion_loss, nerf_amd_volume_render_mse_backward_dist): the far plane finite,
// the coefficient finite and >= 0 (0 switches the term off: its gradient and loss values are zeros)
inline bool bad_distortion(float t_far, float coef) {
    if (!(coef >= 0.f) || coef > 3.402823466e38f) return true;                 // negative, NaN, inf
    return !(t_far >= -3.402823466e38f && t_far <= 3.402823466e38f);
}
// a background: one colour (stride 0) or one per ray (stride 3), in floats; looked at whether or not `bg` is given
inline bool bad_bg_stride(int64_t bg_stride) { return bg_stride != 0 && bg_stride != 3; }

// a scene box (nerf_amd_box_positions): two HOST vectors of three floats, finite, lo < hi on every axis
inline bool bad_box(const float* h_lo, const float* h_hi) {
    if (!h_lo || !h_hi) return true;
    for (int i = 0; i < 3; ++i) {
        if (!(h_lo[i] >= -3.402823466e38f) || !(h_hi[i] <= 3.402823466e38f)) return true;       // -inf / +inf / NaN
        if (!(h_lo[i] < h_hi[i])) return true;                                                   // also the other infinity
    }
    return false;
}

// the segments of a grid span (nerf_amd_span_positions) over a grid of (nx, ny, nz) >= 2 points: K a multiple of 64, at least
// 64 and at least twice the cells of the longest axis -- what makes 8 cells per segment enough
constexpr int SPAN_MAX_PROBES = 1024;
inline bool bad_span_probes(int probes, int64_t nx, int64_t ny, int64_t nz) {
    const int64_t cells = (nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz)) - 1;
    return probes < 64 || probes % 64 != 0 || probes < 2 * cells;
}
// three HOST floats, each finite
inline bool bad_f32x3(const float* h) {
    if (!h) return true;
    for (int i = 0; i < 3; ++i)
        if (!(h[i] >= -3.402823466e38f && h[i] <= 3.402823466e38f)) return true;                 // -inf / +inf / NaN
    return false;
}

// the gradient guard (nerf_amd_grad_guard, nerf_amd_adam_step_guarded): the record is eight 32-bit words in device memory,
// 16-byte aligned; the workspace holds one double per workgroup of the reduction's fixed partition, whatever n is
inline bool bad_guard_record(const void* guard) { return !guard || misaligned(guard, 16); }
inline int64_t grad_guard_ws_bytes() { return align256((int64_t)GRAD_GUARD_BLOCKS * 8); }

// the rays and jitter of a rays-mode launch whose kernels form the sample positions themselves
inline MlpArgs rays_args(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed, int64_t ray_id0,
                         int64_t B, int N) {
    MlpArgs a{};
    a.rays = rays; a.u = u; a.tbins = tbins;
    a.P = B * (int64_t)N; a.N = N; a.flags = flags; a.seed = seed; a.ray_id0 = ray_id0;
    return a;
}

// the rays, jitter and sizes every stage of the masked render takes (the kernels form the sample positions themselves):
// 0 = go on, otherwise the code to return.  `unsupported_n` is the entry point's own size rule (N > MASKED_MAX_N,
// N > COMPOSITE_BWD_MAX_N, nerf_pdf::unsupported_sizes): NERF_AMD_EUNSUP comes after the jitter rule and before the rays.
inline int masked_rays_check(const float* rays, const float* u, const float* tbins, uint32_t flags, int64_t B, int N,
                             bool unsupported_n) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (bad_jitter(flags, u, tbins)) return NERF_AMD_EINVAL;
    if (unsupported_n || B > MASKED_MAX_RAYS) return NERF_AMD_EUNSUP;
    if (B > 0 && !rays) return NERF_AMD_EINVAL;
    return 0;
}

// a capped entry point (fixed capacity of C live points): 1 <= C <= B N, so B >= 1; the mask and its offsets
inline int capped_check(const uint64_t* mask, const int64_t* offsets, int64_t C, int64_t B, int N) {
    if (C > B * (int64_t)N) return NERF_AMD_EINVAL;
    if (!mask || !offsets || misaligned(mask, 8) || misaligned(offsets, 8)) return NERF_AMD_EINVAL;
    return 0;
}

// the camera set every camera entry point takes (M images of H x W pixels, focal length f in pixels): the sizes, then --
// behind the entry point's own empty problem -- the limits the kernels' 32-bit pixel arithmetic and grids set
constexpr int64_t CAMERA_MAX = 0x7fffffffll;     // of M, of B and of H W
inline bool bad_camera_sizes(int64_t B, int64_t M, int H, int W, float f) {
    return B < 0 || M < 0 || H <= 0 || W <= 0 || !(f > 0.f) || f > 3.402823466e38f;      // f: negative, zero, NaN, inf
}
inline bool unsupported_camera_sizes(int64_t B, int64_t M, int H, int W) {
    return B > CAMERA_MAX || M > CAMERA_MAX || (int64_t)H * W > CAMERA_MAX;
}

// the per-image colour correction (M images of HW pixels each, rows of six floats): the sizes, then -- behind the entry point's
// own empty problem -- the limits of the grids and of the product M HW; a row per ray (stride 6) or one row for all rays (0)
inline bool bad_appearance_sizes(int64_t B, int64_t M, int64_t HW) { return B < 0 || M <= 0 || HW <= 0; }
inline bool unsupported_appearance_sizes(int64_t B, int64_t M, int64_t HW) {
    return B > CAMERA_MAX || M > CAMERA_MAX || HW > CAMERA_MAX;
}
inline bool bad_theta_stride(int64_t theta_stride) { return theta_stride != 0 && theta_stride != 6; }

// the image metrics (M image pairs of H x W pixels, rows of at least 3 floats): the sizes, then -- behind the empty problem --
// the limit of the kernels' 32-bit pixel arithmetic, and the smallest image that holds one 11 x 11 SSIM window
constexpr int SSIM_WINDOW = 11;
inline bool bad_metrics_sizes(int64_t M, int H, int W, int64_t pred_stride, int64_t gt_stride) {
    return M < 0 || H <= 0 || W <= 0 || pred_stride < 3 || gt_stride < 3;
}
inline bool unsupported_metrics_sizes(int H, int W) { return (int64_t)H * W > CAMERA_MAX; }
inline bool unsupported_ssim_sizes(int H, int W) { return H < SSIM_WINDOW || W < SSIM_WINDOW; }
