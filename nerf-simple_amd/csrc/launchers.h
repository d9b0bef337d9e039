// launchers.h -- every function one source of this directory defines and another calls: the kernel launchers
// (nerf_amd_launch_*) and the few host helpers beside them.  api.hip calls them; the source that defines one includes this
// header too, so a definition whose parameter list drifts from the declaration its callers see is a compile error
// (C linkage would otherwise link it and pass garbage to a launch).  No .hip file declares a function of another file.
// A launcher returns 0, a hipError_t, or -2 for a size its kernel does not serve (api.hip refuses those first).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

struct MlpArgs;          // nerf_device.h
struct DensityArgs;

// What the dense training head reads (composite_head.hip), filled by api.hip's three entry points.  A term's fields are
// looked at only where the term is on: std != 0 (noise), bg != NULL, dist, theta != NULL (the affine map; with no other term).
struct DenseHeadArgs {
    const float *raw, *ts, *rays, *target;
    float *rgb, *d_raw;                                // rgb [B,3] = the loss's prediction, or NULL
    long long B;
    int N;
    float scale;                                       // 1 / (3 B): the launcher's
    const float* bg;                                   // one colour (bg_stride 0) or one per ray (bg_stride 3)
    long long bg_stride;
    float std;                                         // noise on sigma: keyed by seed (+ *seed_mem), ray ids from ray_id0
    unsigned long long seed;
    const unsigned long long* seed_mem;
    long long ray_id0;
    bool dist;                                         // the distortion term (coef may be 0): t_far, coef, loss_ray [B] or NULL
    float t_far, coef;
    float* loss_ray;
    const float* theta;                                // the affine map: rows [B,6] (theta_stride 6) or one row (theta_stride 0),
    long long theta_stride;
    float* g_theta;                                    // and every ray's row of d loss / d theta [B,6]
};

// The fine pass's sampler behind a dense walk (sample_pdf_device.h sample_behind_walk): what both dense coarse heads read beside
// their own arguments -- composite_backward_kernel<E> (composite.hip), which takes the ray id of ray 0 beside it, and
// dense_head_kernel<.., E> (composite_head.hip), where the ray ids start at DenseHeadArgs::ray_id0 as the noise's do.
struct DensePdfArgs {
    const float* u;                                    // u[B,Nf]; with seed_in_mem the DEVICE ADDRESS of the 64-bit seed offset
    float* ts_out;                                     // [B, Nc+Nf]
    int Nf;
    int device_rng;
    int seed_in_mem;
    unsigned long long seed;
};

// What the masked compositor backward reads beside the rays (occupancy_train.hip), filled by the entry points that reach it
// (api.hip: the eager backward; occupancy_graph.hip and masked_controls.hip: the three capped heads, through
// capped_head_args below).  The upstream gradients are the MSE head's where target != NULL and the five pointers otherwise.
// Behind the MSE head the fine pass's sampler may run (ts_out != NULL) and any of the head's terms may be on, its fields as
// DenseHeadArgs has them: std != 0 (noise; the ray ids are the jitter's, MlpArgs::ray_id0), bg != NULL, coef != 0 (not with
// the sampler).  A term's fields are looked at only where the term is on.
struct MaskedBackwardArgs {
    const unsigned long long* mask;                    // [B, ceil(N / 64)]
    const long long* offsets;                          // [B + 1]
    const float* raw_live;
    float* d_raw_live;
    long long B;
    long long capacity;                                // rows of raw_live / d_raw_live, the clamp of every row index and
                                                       // the end of the zero fill; MASKED_NO_CLAMP: the rows are offsets[B]
    const float *g_rgb, *g_disp, *g_alpha, *g_acc, *g_w;   // each may be NULL
    const float* target;                               // the MSE head: [B,3]
    float* rgb;                                        // [B,3] = the loss's prediction
    float scale;                                       // 1 / (3 B): the launcher's
    const float* u_f;                                  // the sampler: u_f[B, Nf] (unused with the counter RNG)
    float* ts_out;                                     // [B, N + Nf]
    int Nf;
    const float* bg;                                   // one colour (bg_stride 0) or one per ray (bg_stride 3)
    long long bg_stride;
    float std;                                         // noise on sigma: keyed by noise_seed (+ *seed_mem)
    unsigned long long noise_seed;
    const unsigned long long* seed_mem;
    float t_far, coef;                                 // the distortion term; coef == 0: off, loss_ray gets zeros
    float* loss_ray;                                   // [B] or NULL
};
constexpr long long MASKED_NO_CLAMP = 0x7fffffffffffffffll;
// the gradient guard's fixed number of workgroups = the doubles of its workspace (adam.hip, nerf_amd_grad_guard_workspace_bytes)
constexpr int GRAD_GUARD_BLOCKS = 256;

// the plain MSE head under the clamp `capacity`: what the three capped heads share; the sampler's and the terms' fields zero
inline MaskedBackwardArgs capped_head_args(const float* raw_live, const uint64_t* mask, const int64_t* offsets, const float* gt,
                                           float* rgb, float* d_raw_live, int64_t capacity, int64_t B) {
    MaskedBackwardArgs b{};
    b.mask = reinterpret_cast<const unsigned long long*>(mask);
    b.offsets = reinterpret_cast<const long long*>(offsets);
    b.raw_live = raw_live; b.d_raw_live = d_raw_live;
    b.B = B; b.capacity = capacity;
    b.target = gt; b.rgb = rgb;
    return b;
}

// The (NOISE, BG) ladder of the training heads' launchers (composite_head.hip, occupancy_train.hip), one of the two terms being
// on: f is called once with the pair as std::bool_constant, e.g. with_noise_bg(noise, bg, [&](auto n, auto b) { ..<n(), b()>.. }).
template <class F>
inline void with_noise_bg(bool noise, bool bg, F&& f) {
    if (!noise) f(std::false_type{}, std::true_type{});
    else if (!bg) f(std::true_type{}, std::false_type{});
    else f(std::true_type{}, std::true_type{});
}

extern "C" {
int nerf_amd_launch_pack(const float*, void*, int, hipStream_t);
int nerf_amd_launch_pack_train(const float*, void*, void*, hipStream_t);
int nerf_amd_launch_composite_mse_backward(const float*, const float*, const float*, const float*, float*, float*, long long,
                                           int, hipStream_t);
int nerf_amd_launch_composite_mse_backward_pdf(const float*, const float*, const float*, const float*, float*, float*,
                                               const float*, float*, long long, int, int, unsigned long long, long long, int,
                                               int, hipStream_t);
int nerf_amd_launch_param_gradients_begin(const float*, void*, float*, long long, hipStream_t);
int nerf_amd_launch_param_gradients_finish(const void*, const void*, const void*, const void*, const void*, float*, long long,
                                           int, hipStream_t);
int nerf_amd_launch_query_points(const MlpArgs*, float*, hipStream_t);
int nerf_amd_launch_gamma(const float*, long long, float*, long long, int, hipStream_t);
int nerf_amd_launch_posenc(const float*, float*, float*, long long, int, int, hipStream_t);
int nerf_amd_launch_composite(const float*, const float*, const float*, long long, float*, float*,
                              float*, float*, float*, long long, int, int, float*, hipStream_t);
int nerf_amd_launch_sample_pdf(const float*, const float*, const float*, float*, long long, int, int,
                               unsigned long long, long long, int, hipStream_t);
int nerf_amd_launch_sample_pdf_volume(const MlpArgs*, const float*, long long, long long, long long, const float*, const float*,
                                      const float*, float*, float*, float*, int, hipStream_t);
int nerf_amd_launch_sample_pdf_volume_masked(const MlpArgs*, const float*, long long, long long, long long, const float*,
                                             const float*, const unsigned*, long long, long long, long long, const float*,
                                             const float*, int, const float*, float*, float*, float*, unsigned long long*,
                                             long long*, long long*, void*, int, hipStream_t);
int nerf_amd_launch_generate_rays(const float*, int, int, float, long long, long long, float*, hipStream_t);
int nerf_amd_launch_composite_backward(const float*, const float*, const float*, long long, const float*,
                                       const float*, const float*, const float*, const float*, float*,
                                       long long, int, int, hipStream_t);
int nerf_amd_launch_mse_loss(const float*, const float*, float*, float*, long long, hipStream_t);
int nerf_amd_launch_sample_encode(const MlpArgs*, float*, float*, hipStream_t);
int nerf_amd_launch_mlp_f32(const MlpArgs*, int, hipStream_t);
int nerf_amd_launch_mlp_bf16_16(const MlpArgs*, int, hipStream_t);
int nerf_amd_launch_mlp_f16_16(const MlpArgs*, int, hipStream_t);
int nerf_amd_launch_mlp_backward(const float*, const void*, const void*, void*, long long, int, hipStream_t);
int nerf_amd_launch_param_gradients_finish_e4m3(const void*, const void*, const void*, float*, long long, int, hipStream_t);
int nerf_amd_launch_param_gradients_convert_e4m3(const void*, const void*, const void*, void*, long long, int, hipStream_t);
long long nerf_amd_f8_scratch_bytes(long long);
int nerf_amd_launch_mt19937_uniform(const uint32_t*, int, float*, long long, uint32_t*, hipStream_t);
int nerf_amd_launch_mt19937_uniform_par(const uint32_t*, int, float*, long long, uint32_t*, const uint32_t*, int, long long,
                                        uint32_t*, hipStream_t);
int nerf_amd_launch_range_check(const MlpArgs*, long long, unsigned*, hipStream_t);
int nerf_amd_launch_mt19937_raw(const uint32_t*, int, uint32_t*, long long, uint32_t*, hipStream_t);
int nerf_amd_launch_mt19937_uniform_after(const uint32_t*, const uint32_t*, int, int, float*, long long, uint32_t*, long long, uint32_t*,
                                          hipStream_t);
int nerf_amd_launch_mt19937_advance(const uint32_t*, const uint32_t*, uint32_t*, hipStream_t);
int nerf_amd_launch_select_rays(const uint32_t*, unsigned long long, const unsigned long long*, long long, long long, const float*,
                                const float*, float*, float*, long long*, void*, hipStream_t);
int nerf_amd_host_mt19937_jump_poly(long long, const uint32_t*, uint32_t*);
int nerf_amd_launch_adam_hyper(float*, const float*, float*, float*, long long, const float*, hipStream_t);
int nerf_amd_launch_hyper_fetch(const float*, int, float*, unsigned*, hipStream_t);
// the gradient guard (adam.hip): `partial` holds GRAD_GUARD_BLOCKS doubles, `guard` is the 8-word record
int nerf_amd_launch_grad_guard(const float*, long long, double*, unsigned*, hipStream_t);
int nerf_amd_launch_adam_guarded(float*, const float*, float*, float*, long long, const float*, const unsigned*, hipStream_t);
int nerf_amd_launch_linear_f32(const float*, long long, long long, const float*, const float*, long long, long long, const float*,
                               float*, long long, long long, long long, long long, int, hipStream_t);
int nerf_amd_launch_adam(float*, const float*, float*, float*, long long, float, float, float, float, float, float,
                         hipStream_t);
int nerf_amd_launch_sample_encode_bf16(const MlpArgs*, void*, void*, hipStream_t);
int nerf_amd_launch_param_gradients(const float*, const void*, const void*, const void*, const void*, void*, float*,
                                    long long, hipStream_t);
int nerf_amd_launch_input_gradients(const void*, const float*, const float*, const float*, const float*, float*, float*,
                                    long long, int, hipStream_t);
int nerf_amd_launch_query_points_backward(const float*, const float*, const float*, float*, long long, int, hipStream_t);
int nerf_amd_launch_gamma_backward(const float*, long long, const float*, float*, long long, int, hipStream_t);
int nerf_amd_launch_posenc_backward(const float*, const float*, const float*, float*, long long, int, int, hipStream_t);
int nerf_amd_launch_density_bf16(const DensityArgs*, hipStream_t);
int nerf_amd_launch_density_f16(const DensityArgs*, hipStream_t);
int nerf_amd_launch_grid_points(const DensityArgs*, long long, long long, float*, hipStream_t);
long long nerf_amd_mc_workspace_bytes(long long);
int nerf_amd_launch_mc_count(const float*, long long, long long, long long, float, void*, long long*, hipStream_t);
int nerf_amd_launch_mc_emit(const float*, long long, long long, long long, float, const float*, const float*, void*, float*, float*,
                            int*, long long, long long, hipStream_t);
int nerf_amd_occ_max_n(void);
int nerf_amd_occ_max_dilate(void);
long long nerf_amd_occ_workspace_bytes(long long);
int nerf_amd_launch_occ_bits(const float*, long long, long long, long long, float, int, unsigned*, hipStream_t);
int nerf_amd_launch_occ_pack(const unsigned char*, long long, long long, long long, unsigned*, hipStream_t);
int nerf_amd_launch_occ_mark(const MlpArgs*, const unsigned*, long long, long long, long long, const float*, const float*, int,
                             unsigned long long*, long long*, long long*, void*, long long, hipStream_t);
int nerf_amd_launch_occ_scan(void*, long long*, long long*, long long, hipStream_t);
int nerf_amd_launch_occ_emit(const MlpArgs*, const unsigned long long*, const long long*, float*, long long, long long, hipStream_t);
int nerf_amd_launch_occ_composite(const MlpArgs*, const unsigned long long*, const long long*, const float*, long long, hipStream_t);
int nerf_amd_occ_train_max_n(void);
int nerf_amd_launch_masked_backward(const MlpArgs*, const MaskedBackwardArgs*, hipStream_t);
int nerf_amd_launch_occ_decay_max(float*, const float*, float, long long, hipStream_t);
int nerf_amd_launch_sigma_noise(const float*, float*, float, unsigned long long, const unsigned long long*, long long, long long,
                                int, hipStream_t);
int nerf_amd_launch_background_blend(const float*, const float*, const float*, const float*, long long, float*, float*,
                                     long long, hipStream_t);
int nerf_amd_launch_background_blend_backward(const float*, const float*, long long, float*, long long, hipStream_t);
int nerf_amd_launch_dense_head(const DenseHeadArgs*, hipStream_t);
int nerf_amd_launch_dense_head_pdf(const DenseHeadArgs*, const DensePdfArgs*, hipStream_t);
int nerf_amd_launch_distortion_loss(const float*, const float*, float, float, float*, float*, long long, int, hipStream_t);
int nerf_amd_launch_sum_f32(const float*, float*, long long, hipStream_t);
int nerf_amd_launch_sigma_noise_masked(const float*, float*, float, unsigned long long, const unsigned long long*, long long,
                                       const unsigned long long*, const long long*, long long, int, hipStream_t);
int nerf_amd_launch_camera_rays(const float*, const float*, const long long*, long long*, int, int, float, float*, long long,
                                long long, hipStream_t);
int nerf_amd_launch_camera_rays_backward(const float*, const float*, const long long*, const float*, int, int, float, float*,
                                         long long, long long, hipStream_t);
int nerf_amd_launch_camera_poses(const float*, const float*, float*, long long, hipStream_t);
long long nerf_amd_image_metrics_ws_bytes(long long, int, int);
int nerf_amd_launch_image_metrics(const float*, long long, const float*, long long, double*, double*, float*, void*, long long, int,
                                  int, hipStream_t);
int nerf_amd_launch_appearance_gather(const float*, const long long*, long long*, long long, float*, long long, long long,
                                      hipStream_t);
int nerf_amd_launch_appearance_apply(const float*, const float*, long long, float*, long long, hipStream_t);
int nerf_amd_launch_appearance_apply_backward(const float*, const float*, const float*, long long, float*, float*, long long,
                                              hipStream_t);
int nerf_amd_launch_appearance_reduce(const float*, const long long*, long long, const float*, float, const int*, float*,
                                      long long, long long, hipStream_t);
int nerf_amd_launch_box_positions(const MlpArgs*, const float*, const float*, float, float, float*, float*, int*, long long,
                                  hipStream_t);
int nerf_amd_launch_span_positions(const MlpArgs*, const unsigned*, long long, long long, long long, const float*, const float*,
                                   const float*, int, float, float, float*, float*, int*, long long, hipStream_t);
}
