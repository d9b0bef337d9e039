/* nerf_amd.h -- C ABI of libnerf_amd.so: the MI355X (gfx950) NeRF render hot path.
 *
 * Drop-in boundary for the hot path of UCSD-Comp-Imaging/Nerf-Simple.  The
 * reference has no FFI; its boundary is plain Python call signatures in
 * package `utils`.  Each entry point below names the
 * reference function (file:line, relative to the reference repo) whose body it
 * replaces; the Python host side (nerf-simple_amd/utils/) keeps the reference's
 * names, argument order, defaults and return order and calls these through
 * ctypes (binding shown in INTEGRATION.md).
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer unless its name starts with `h_`;
 *     fp32, row-major, contiguous; never written unless documented as output
 *     (one exception, which is why `packed` is not const where a 16-bit MLP kernel may run: the
 *     sticky status word behind a packed 16-bit image, see nerf_amd_packed_status_offset);
 *   - the library allocates nothing, frees nothing and keeps no pointer after
 *     return; workspaces are caller-provided;
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on it,
 *     do no host synchronisation and are safe to capture into a hipGraph;
 *   - return value: 0 = launched, otherwise a negative NERF_AMD_E* code or a
 *     positive hipError_t; nothing throws or exits across the ABI.
 */
#ifndef NERF_AMD_H
#define NERF_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NERF_AMD_ABI_VERSION 5

/* error codes */
#define NERF_AMD_EINVAL   (-1)   /* bad argument (null pointer, negative size, ...) */
#define NERF_AMD_EUNSUP   (-2)   /* unsupported configuration */

/* precision of the fused MLP */
#define NERF_AMD_F32   0   /* exact-f32 MFMA (v_mfma_f32_16x16x4_f32), fp32 end to end */
#define NERF_AMD_BF16  1   /* bf16 operands on v_mfma_f32_16x16x32_bf16, fp32 accumulate (the flagship) */
#define NERF_AMD_BF16_BWD 3 /* nerf_amd_pack_weights / nerf_amd_packed_bytes only: the transposed image of nerf_amd_mlp_backward */
#define NERF_AMD_FP16  2   /* fp16 operands on v_mfma_f32_16x16x32_f16: same rate, 11-bit mantissa; range 65504 */
/* The NERF_AMD_FP16 image is FOLDED: layers_2 (a linear layer with no activation behind it, feeding color_fc.0 alone) is
 * multiplied into the colour layer by the packer.  Same byte size and the same offsets of every layer, of the bias table
 * and of the status block as the NERF_AMD_BF16 image; the colour layer's first 256 k positions hold
 * Wc[:, :256] W2 (fp32 fma chain, ascending k, then rounded to fp16) in the k order they held Wc[:, :256] in, its bias rows
 * hold bc + Wc[:, :256] b2, and the 16 layers_2 tiles (128 KiB) stay filled with layers_2 but are read by no fp16 kernel:
 * the fp16 inference kernels run 65,536 of the 600,064 padded multiply-accumulates per point less than the bf16 ones.
 * A folded element that does not fit fp16 sets NERF_AMD_STATUS_WORD_WEIGHT_RANGE like any weight that does not.  An fp16
 * image must therefore come from nerf_amd_pack_weights(..., NERF_AMD_FP16), never from converting a bf16 one. */

/* flags of nerf_amd_render_forward / nerf_amd_mlp_forward_rays */
#define NERF_AMD_TS_GIVEN   1u  /* `u` holds sample positions ts[B,N], not jitter */
/* With NERF_AMD_TS_GIVEN `u` is required whatever the other flags are: every rays-mode entry point returns NERF_AMD_EINVAL
 * for u == NULL then. */
#define NERF_AMD_DEVICE_RNG 2u  /* `u` ignored (may be NULL): jitter from the counter RNG */
#define NERF_AMD_SEED_IN_MEMORY 4u /* with NERF_AMD_DEVICE_RNG: `u` is the DEVICE ADDRESS of a uint64 that is added to
                                    * `seed` when the kernel runs -- a launch captured into a hipGraph is replayed with
                                    * frozen arguments, and this is how every replay of a training step draws fresh
                                    * jitter (the reference draws torch.rand(B,N) anew per call, utils/rendering.py:28) */

/* ---- introspection (host only, no GPU needed) ------------------------------ */
int      nerf_amd_abi_version(void);
/* 595844 = parameters of Nerf(Lp=10, Ld=4, H=256), reference utils/nets.py:9-32 */
int64_t  nerf_amd_param_count(void);
/* bytes of the packed weight image for a precision (the caller allocates it) */
int64_t  nerf_amd_packed_bytes(int precision);
/* Range guard of the 16-bit images.  The reference is fp32 with no range limit (utils/nets.py:16-32); fp16
 * operands overflow beyond 65504.  A packed NERF_AMD_FP16 / NERF_AMD_BF16 image ends with a 256-byte status
 * block of sticky uint32 flags (0 / 1), zeroed by nerf_amd_pack_weights:
 *   word NERF_AMD_STATUS_WORD_NONFINITE     set by every 16-bit MLP forward kernel when a point's (rgb, sigma) output
 *                                           is inf or NaN (where an overflowed hidden activation ends up);
 *   word NERF_AMD_STATUS_WORD_WEIGHT_RANGE  set by the packer if a weight is not finite in the operand type (beyond its
 *                                           range, or NaN / inf to begin with).
 * Returns the byte offset of word 0 inside the image, -1 for images without a status block (NERF_AMD_F32,
 * NERF_AMD_BF16_BWD).  The host wrapper (utils/nets.py) reads it after the first fp16 render of a weight set and
 * falls back to bf16 operands with a warning instead of returning NaN pixels. */
#define NERF_AMD_STATUS_WORD_NONFINITE     0
#define NERF_AMD_STATUS_WORD_WEIGHT_RANGE  1
int64_t  nerf_amd_packed_status_offset(int precision);
/* bytes of workspace nerf_amd_render_forward / _pixels_forward need for B rays x N samples.
 * 0 up to 768 samples per ray: those renders run as ONE launch (sampling + encoding + MLP +
 * compositing, samples composited out of LDS) and `workspace` may be NULL; longer rays take the
 * two-launch path through raw[B,N,4] + ts[B,N]. */
int64_t  nerf_amd_render_workspace_bytes(int precision, int64_t B, int N);
/* host-side self-check of the packed-weight index math (bijectivity of the
 * k-permutations, offsets, sizes); 0 = consistent.  Used by the CPU tests. */
int      nerf_amd_layout_selfcheck(void);
/* host-side: source column (or -1 = padding) that the packed image holds at
 * (layer, k-step, lane group 0..3, element 0..7 [16-bit images] / 0 [f32]); -2 = out of range.
 * Lets tests audit the packing. */
int      nerf_amd_layout_src_col(int precision, int layer, int kstep, int group, int elem);

/* ---- weights ---------------------------------------------------------------- */
/* Pack the 24 state-dict tensors of the reference Nerf (utils/nets.py:16-32),
 * given flattened in state_dict order as one fp32 vector `params`[595844], into
 * the MFMA-fragment-ordered image the fused kernels stream.  Derived cache:
 * re-run after any parameter update.  */
int nerf_amd_pack_weights(const float* params, void* packed, int precision, void* stream);
/* The two images a training step needs (NERF_AMD_BF16 and NERF_AMD_BF16_BWD) in one launch.  Clears the status block of
 * the forward image except NERF_AMD_STATUS_WORD_WEIGHT_RANGE, which it only ever sets (a non-finite weight stays
 * non-finite under Adam; nerf_amd_pack_weights clears the word): `packed_bf16` is an image that nerf_amd_pack_weights
 * has filled before (any weights), re-packed in place from then on. */
int nerf_amd_pack_weights_train(const float* params, void* packed_bf16, void* packed_bwd, void* stream);

/* ---- positional encoding: utils/xyz.py:6-36 --------------------------------- */
/* gamma(x, L): x[n] -> out[n, 2L] = [sin(2^0 x), cos(2^0 x), ..., sin(2^(L-1) x), cos(2^(L-1) x)]
 * (utils/xyz.py:6-14).  `x_stride` in floats lets x be a column of a wider table. */
int nerf_amd_gamma(const float* x, int64_t x_stride, float* out, int64_t n, int L, void* stream);
/* positional_encoder(vec, Lp, Ld): vec[P,6] -> posx[P,3+6Lp], posd[P,3+6Ld]
 * (utils/xyz.py:16-36), columns grouped per coordinate. */
int nerf_amd_positional_encoder(const float* vec, float* posx, float* posd,
                                int64_t P, int Lp, int Ld, void* stream);

/* ---- the MLP: Nerf.forward, utils/nets.py:34-43 ------------------------------ */
/* pts[P,6] = [x,y,z,d1,d2,d3] -> out[P,4] = [r,g,b,sigma] (raw: no sigmoid, no
 * softplus).  Encoding + 12 dense layers fused in one kernel; activations never
 * leave the CU.  `packed` from nerf_amd_pack_weights with the same precision.
 * The encoder inside: NERF_AMD_F32 evaluates sinf / cosf on the exactly scaled argument 2^l x (5e-7 of float64).  The 16-bit
 * kernels (this one, the rays-mode and render entry points, nerf_amd_density_forward, the bf16 training forward and the
 * stored rows of nerf_amd_sample_encode_bf16 / nerf_amd_encode_points_bf16) use the hardware sine on x / (2 pi) carried as
 * an fp32 pair; every feature, before it is rounded to the operand type, is within 2e-6 of float64 sin / cos (2^l x) --
 * measured 5.6e-7, the stored rows 3.8e-7 -- VERIFIED FOR |x| <= 4096 at every level 0..9 (tests/test_gpu_encoder_probe.py;
 * the scene range is 4.5).  Beyond that no accuracy is claimed; every sin / cos feature stays finite with |f| <= 1 for every
 * finite x, FLT_MAX included.  A raw coordinate beyond the operand type's range (65504 in fp16; FLT_MAX rounds to inf in
 * bf16) becomes inf, makes the point's outputs NaN and sets NERF_AMD_STATUS_WORD_NONFINITE. */
int nerf_amd_mlp_forward(const float* pts, void* packed, float* out,
                         int64_t P, int precision, void* stream);

/* ---- sampling + query points on their own: utils/rendering.py:24-40 ------------ */
/* rays[B,6] (+ u / ts / device RNG and tbins as in nerf_amd_render_forward) -> query_pts[B*N,6] =
 * [origin + direction * t, direction / ||direction||] ray-major / sample-minor, and ts[B,N] (may be NULL).
 * For a caller whose network is not the fused one (render_nerf with a foreign `net`): that net's own forward
 * runs on query_pts, nerf_amd_volume_render_rays composites. */
int nerf_amd_query_points(const float* rays, const float* u, const float* tbins,
                          uint32_t flags, uint64_t seed, int64_t ray_id0,
                          float* query_pts, float* ts, int64_t B, int N, void* stream);

/* ---- compositing: volume_render, utils/rendering.py:47-85 -------------------- */
/* raw[B,N,4], ts[B,N], dirs[B] (3 floats at stride `dirs_stride` floats) ->
 * rgb[B,3], disp[B], alpha[B,N], acc[B], w[B,N].  alpha and w may be NULL.
 * One wavefront per ray; transmittance by a wave-level product scan.
 * N == 1 reproduces the reference's degenerate result (every compositing entry point and the fused renders):
 * its delta construction (utils/rendering.py:60-61) leaves the sample axis EMPTY there, so rgb = acc = 0,
 * disparity = NaN, alpha / w (shape [B,0] in the reference) are not written and d_raw is zero. */
int nerf_amd_volume_render(const float* raw, const float* ts,
                           const float* dirs, int64_t dirs_stride,
                           float* rgb, float* disp, float* alpha, float* acc, float* w,
                           int64_t B, int N, void* stream);

/* Image-driver form of the compositor (stage 2 of nerf_amd_render_image_forward
 * on its own): raw[B,N,4], ts[B,N] from nerf_amd_mlp_forward_rays and the same
 * rays[B,6] -> pixels[B,4] = [clip(rgb,0,1), disparity]  (utils/rendering.py:102-105). */
int nerf_amd_volume_render_pixels(const float* raw, const float* ts, const float* rays,
                                  float* pixels, int64_t B, int N, void* stream);

/* Backward of the above: d loss / d raw [B,N,4] from the upstream gradients of
 * the five outputs (any of g_* may be NULL = zero).  Autograd through
 * volume_render in the training step, reference train.py:51-54.  ts and dirs
 * get no gradient (they carry none in the reference either).  N <= 512.
 * Per element (tests/test_gpu_ray_routines.py): d alpha / d sigma is e delta softplus'(sigma) with e = exp(-softplus(sigma)
 * delta) itself and softplus' = exp(sigma) / (1 + exp(sigma)) as autograd forms them, so a nearly opaque sample (e -> 0)
 * and a hugely negative sigma keep their relative precision.
 * Where the disparity has no slope: on its clamp branch (depth / acc <= 1e-10) g_disp contributes zero, as in autograd; on an
 * EMPTY ray (acc == 0: disparity = 1 / max(1e-10, 0/0) = NaN) g_disp contributes ZERO as well, where autograd writes NaN
 * into the whole sigma column (NaN x softplus', even where softplus' is 0) -- the forward's NaN disparity already reports
 * the empty ray, and a NaN here would reach every weight.
 * Non-finite raw values: d_raw has NaN exactly where the reference's fp32 autograd has it (g_rgb upstream: the whole sigma
 * column of a ray that holds a NaN sigma, the colours from that sample on, 0 x inf products), and every other ray is
 * bit for bit what it is when run alone. */
int nerf_amd_volume_render_backward(const float* raw, const float* ts,
                                    const float* dirs, int64_t dirs_stride,
                                    const float* g_rgb, const float* g_disp, const float* g_alpha,
                                    const float* g_acc, const float* g_w,
                                    float* d_raw, int64_t B, int N, void* stream);

/* Both with the directions taken from rays[B,6] and normalised inside the kernel,
 * dirs = rays[:,3:] / ||rays[:,3:]|| as render_nerf does (utils/rendering.py:37,43):
 * no [B,3] temporary, no extra launch (the training step uses these). */
int nerf_amd_volume_render_rays(const float* raw, const float* ts, const float* rays,
                                float* rgb, float* disp, float* alpha, float* acc, float* w,
                                int64_t B, int N, void* stream);
int nerf_amd_volume_render_rays_backward(const float* raw, const float* ts, const float* rays,
                                         const float* g_rgb, const float* g_disp, const float* g_alpha,
                                         const float* g_acc, const float* g_w,
                                         float* d_raw, int64_t B, int N, void* stream);

/* Training form (reference train.py:51-54 between the MLP forward and its backward): compositing
 * forward, loss = MSELoss(rgb, target) (mean over 3B elements), and the backward of both in ONE launch:
 * raw, ts, rays, target[B,3] -> rgb[B,3] (may be NULL; feed it to nerf_amd_mse_loss for the loss value)
 * and d_raw[B,N,4] = d loss / d raw.  N <= 512. */
int nerf_amd_volume_render_mse_backward(const float* raw, const float* ts, const float* rays,
                                        const float* target, float* rgb, float* d_raw,
                                        int64_t B, int N, void* stream);

/* Coarse head of the hierarchical training step (BASELINE config 4; the NeRF paper's objective
 * MSE(rgb_c, gt) + MSE(rgb_f, gt)).  ONE launch, one wavefront per ray, doing what
 *   nerf_amd_volume_render_mse_backward(raw, ts, rays, target, rgb, d_raw)         (train.py:51-54 on the coarse pass)
 *   + nerf_amd_volume_render_rays(...) for w                                      (utils/rendering.py:69, w = alpha * T)
 *   + nerf_amd_sample_pdf(ts, w, u, ...) -> ts_out                                 (no reference counterpart)
 * would, bit for bit: raw[B,Nc,4], ts[B,Nc], rays[B,6], target[B,3] -> rgb[B,3] (may be NULL), d_raw[B,Nc,4] and
 * ts_out[B,Nc+Nf] (the fine pass's merged, sorted positions).  The weights go from registers to LDS and never reach
 * HBM; they carry no gradient (the coarse net learns from its own loss only: w.detach()).
 * Jitter of the Nf new samples: u[B,Nf]; or NERF_AMD_DEVICE_RNG with nerf_amd_sample_pdf's key (seed, ray_id0);
 * or NERF_AMD_DEVICE_RNG | NERF_AMD_SEED_IN_MEMORY, `u` then the DEVICE ADDRESS of the 64-bit seed offset (a node
 * of a replayed graph).  3 <= Nc <= 256, Nc + Nf <= 512, otherwise NERF_AMD_EUNSUP.  Parity unpinned like
 * nerf_amd_sample_pdf (the reference has no hierarchical path). */
int nerf_amd_volume_render_mse_backward_pdf(const float* raw, const float* ts, const float* rays,
                                            const float* target, const float* u, uint32_t flags,
                                            uint64_t seed, int64_t ray_id0, float* rgb, float* d_raw,
                                            float* ts_out, int64_t B, int Nc, int Nf, void* stream);

/* ---- the whole path: render_nerf, utils/rendering.py:13-45 ------------------- */
/* rays[B,6] = [origin, direction] -> (rgb[B,3], disp[B], alpha[B,N], acc[B], w[B,N]).
 *   u        jitter in [0,1) [B,N] exactly as the reference draws it with
 *            torch.rand(B,N) (utils/rendering.py:28); or ts[B,N] with
 *            NERF_AMD_TS_GIVEN; or unused with NERF_AMD_DEVICE_RNG (counter RNG
 *            keyed by (seed, ray_id0 + ray, sample) so results do not depend on
 *            batching or sharding).
 *   tbins    linspace(tn, tf, N+1) computed by the caller [N+1] (device), so
 *            bin edges are bit-identical to torch.linspace (utils/rendering.py:25)
 *   alpha,w  optional (NULL to skip the 8 B/sample of output traffic)
 *   workspace  nerf_amd_render_workspace_bytes(precision,B,N) bytes, 256-B aligned (NULL if 0) */
int nerf_amd_render_forward(const float* rays, const float* u, const float* tbins,
                            void* packed, int precision, uint32_t flags,
                            uint64_t seed, int64_t ray_id0,
                            float* rgb, float* disp, float* alpha, float* acc, float* w,
                            void* workspace, int64_t B, int N, void* stream);

/* Image-driver form (the body of utils/rendering.py:102-105 for one batch): the same render, output
 * pixels[B,4] = [clip(rgb,0,1), disparity]; rgb is clipped AFTER compositing, disparity is not. */
int nerf_amd_render_pixels_forward(const float* rays, const float* u, const float* tbins,
                                   void* packed, int precision, uint32_t flags,
                                   uint64_t seed, int64_t ray_id0,
                                   float* pixels, void* workspace, int64_t B, int N, void* stream);

/* Stage 1 of the above on its own (sampling + encoding + MLP): writes
 * raw[B,N,4] and ts[B,N].  Exposed for the importance-sampling caller, which
 * needs explicit ts. */
int nerf_amd_mlp_forward_rays(const float* rays, const float* u, const float* tbins,
                              void* packed, int precision, uint32_t flags,
                              uint64_t seed, int64_t ray_id0,
                              float* raw, float* ts, int64_t B, int N, void* stream);

/* ---- image drivers: render_poses / render_image, utils/rendering.py:88-153 ---- */
/* Pinhole rays on the device (utils/xyz.py:38-52 + utils/rendering.py:129-134):
 * rays[i] = [pose[:3,3], pose[:3,:3] @ ((w-W//2)/f, -(h-H//2)/f, -1)] for pixel
 * p = ray0 + i = h*W + w.  h_pose: HOST pointer to a row-major 3x4 / 4x4 pose. */
int nerf_amd_generate_rays(const float* h_pose, int H, int W, float f,
                           int64_t ray0, int64_t n_rays, float* rays, void* stream);
int64_t nerf_amd_render_image_workspace_bytes(int precision, int64_t n_rays, int N);
/* One call = the body of the reference's per-image loop (utils/rendering.py:139-151)
 * for pixels [ray0, ray0+n_rays) of an HxW view: ray generation, render_nerf,
 * clip(rgb,0,1) after compositing, disparity un-clipped ->
 * pixels[n_rays,4] = [r,g,b,disparity].  Two launches (three on the two-launch path), no host sync; the
 * multi-GPU driver calls it per rank and all-gathers `pixels`.  u / tbins /
 * flags / seed as in nerf_amd_render_forward (u indexed from ray0). */
int nerf_amd_render_image_forward(const float* h_pose, int H, int W, float f,
                                  int64_t ray0, int64_t n_rays,
                                  const float* u, const float* tbins,
                                  void* packed, int precision, uint32_t flags, uint64_t seed,
                                  float* pixels, void* workspace, int N, void* stream);

/* ---- hierarchical sampling (BASELINE config 4) -------------------------------- */
/* ABSENT from the reference (README.md:3, configs/lego.yaml:7): parity unpinned.
 * Inverse-CDF placement of Nf new samples from the coarse pass's weights (the
 * NeRF paper's sample_pdf over interior bins), merged and sorted with the Nc
 * coarse positions: ts[B,Nc], w[B,Nc], u[B,Nf] in [0,1) (or NERF_AMD_DEVICE_RNG)
 * -> ts_out[B,Nc+Nf] ascending.  Feed ts_out to nerf_amd_render_forward with
 * NERF_AMD_TS_GIVEN for the fine pass.  3 <= Nc <= 256, Nc+Nf <= 512.
 * Per ray (tests/test_gpu_ray_routines.py): ts_out is ascending and holds the Nc coarse positions bit for bit.  A new
 * position is z = b0 + (u - c0) / denom (b1 - b0) between the mids b0, b1 of its bin, accurate to a few
 * 2^-24 [(b1 - b0) (1 + (c1 + u) / denom) + |z|]: the cdf's rounding divided by the bin's mass.  denom = c1 - c0 is replaced
 * by 1 below 1e-5 (the paper's guard), so a bin whose mass is within fp32 rounding of 1e-5 -- every empty bin (weight 0
 * + the 1e-5 floor) of an opaque ray, whose weights sum to 1 -- may place its sample at either end of the bin. */
int nerf_amd_sample_pdf(const float* ts, const float* w, const float* u,
                        uint32_t flags, uint64_t seed, int64_t ray_id0,
                        float* ts_out, int64_t B, int Nc, int Nf, void* stream);

/* BASELINE config 4 as ONE call for pixels [ray0, ray0+n_rays) of an HxW view: device ray generation ->
 * coarse render (Nc stratified samples, network `packed_c`; only its positions and weights are kept)
 * -> nerf_amd_sample_pdf -> fine render of `packed_f` on the Nc+Nf merged positions ->
 * pixels[n_rays,4] = [clip(rgb,0,1), disparity].  Four launches, no host sync, nothing per-sample but
 * ts / w of the coarse pass and ts of the fine pass touches HBM.  u_c[n,Nc] / u_f[n,Nf] explicit
 * uniforms, or NERF_AMD_DEVICE_RNG (both keyed by the global pixel id: sharding-invariant).
 * 3 <= Nc <= 256, Nc+Nf <= 512; otherwise NERF_AMD_EUNSUP (compose the three stages instead).
 * Parity unpinned like nerf_amd_sample_pdf (the reference has no hierarchical sampling). */
int64_t nerf_amd_render_hierarchical_workspace_bytes(int64_t n_rays, int Nc, int Nf);
int nerf_amd_render_hierarchical_forward(const float* h_pose, int H, int W, float f,
                                         int64_t ray0, int64_t n_rays,
                                         const float* u_c, const float* u_f, const float* tbins_c,
                                         void* packed_c, void* packed_f, int precision,
                                         uint32_t flags, uint64_t seed,
                                         float* pixels, void* workspace, int Nc, int Nf, void* stream);

/* Training-side front end: sampling + point assembly + encoding in one launch
 * (utils/rendering.py:24-40 + utils/xyz.py:16-36): rays[B,6] (+ u / ts / device
 * RNG as in nerf_amd_render_forward) -> posx[B*N,63], posd[B*N,27], ts[B,N]
 * (Lp = 10, Ld = 4), fp32, reference column order. */
int nerf_amd_sample_encode(const float* rays, const float* u, const float* tbins,
                           uint32_t flags, uint64_t seed, int64_t ray_id0,
                           float* posx, float* posd, float* ts, int64_t B, int N, void* stream);

/* ---- fused training path of the dense layers (reference train.py:51-54) --------
 * bf16 ONLY: the fused training kernels exist in bf16; a caller asking them for another precision gets
 * NERF_AMD_EUNSUP from its host wrapper.  (Exact fp32 training is the layer-by-layer composition of
 * nerf_amd_positional_encoder, nerf_amd_linear_f32 and the compositor's backward: at the end of this header.)
 * Forward as nerf_amd_mlp_forward_rays (bf16) that ALSO saves every layer's output for the
 * weight gradients (bf16; L0..L7 post-ReLU 256 features, L8 = the linear 256->256, L9 = colour
 * hidden 128; P = B*N points) in the point-blocked layout the kernels write and read with
 * contiguous 256-byte runs: layer L at L * ceil(P/256) * 128 KiB, inside it tile t (256 points)
 * at t * 128 KiB as [feature/8 (32)][point in tile (256)][8 bf16].  Then, at
 * 10 * ceil(P/256) * 128 KiB, the ReLU masks for the dX chain: one bit per feature,
 * 10 * ceil(P/256) * 8 KiB, in the kernels' register order.  (Both layouts: csrc/nerf_layout.h;
 * decoded in tests/test_gpu_training.py.) */
int64_t nerf_amd_train_activation_bytes(int64_t P);
int nerf_amd_mlp_forward_train(const float* rays, const float* u, const float* tbins,
                               void* packed_bf16, uint32_t flags, uint64_t seed, int64_t ray_id0,
                               float* raw, float* ts, void* acts, int64_t B, int N, void* stream);
/* The same for explicit points, i.e. Nerf.forward(v) under autograd (utils/nets.py:34-43):
 * pts[P,6] -> out[P,4], activations saved as above; and the matching bf16 encoder rows. */
int nerf_amd_mlp_forward_train_points(const float* pts, void* packed_bf16, float* out,
                                      void* acts, int64_t P, void* stream);
int nerf_amd_encode_points_bf16(const float* pts, void* posx64, void* posd32, int64_t P, void* stream);
/* Backward dX chain: d_raw[P,4] (from nerf_amd_volume_render_backward) + the ReLU
 * mask bits inside `acts` (the bf16 activations themselves are not read here) ->
 * dys: every layer's pre-activation gradient, bf16, point-blocked like the bf16 part
 * of `acts`.  The gradient w.r.t. activations stays on-chip between
 * layers.  `bwd_image` from nerf_amd_pack_weights(..., NERF_AMD_BF16_BWD).  Weight
 * gradients are then dW_L = dys[L]^T @ input_L: nerf_amd_param_gradients. */
int nerf_amd_mlp_backward(const float* d_raw, const void* bwd_image, const void* acts,
                          void* dys, int64_t P, void* stream);

/* Encoder outputs as the dW GEMM wants them: bf16, posx64[P,64] (col 63 zero),
 * posd32[P,32] (cols 27..31 zero); otherwise as nerf_amd_sample_encode. */
int nerf_amd_sample_encode_bf16(const float* rays, const float* u, const float* tbins,
                                uint32_t flags, uint64_t seed, int64_t ray_id0,
                                void* posx64, void* posd32, float* ts, int64_t B, int N, void* stream);
/* All 24 parameter gradients of the step in ONE flat fp32 vector `grads`[595844]
 * (state_dict order; zeroed by the call): dW_L = dys[L]^T @ input_L as split-K
 * GEMMs over the points, db_L = column sums.  The vector is also the bucket of the
 * data-parallel all-reduce.  scratch: nerf_amd_param_gradients_scratch_bytes(P). */
int64_t nerf_amd_param_gradients_scratch_bytes(int64_t P);
int nerf_amd_param_gradients(const float* d_raw, const void* acts, const void* dys,
                             const void* posx64, const void* posd32, void* scratch,
                             float* grads, int64_t P, void* stream);

/* The same in two parts, so a captured step can overlap the first with the dX chain (both need only
 * d_raw): _begin zeroes `grads`, packs d_raw into `scratch` and adds the two head bias gradients;
 * _finish runs the 14 products and the other bias sums. */
int nerf_amd_param_gradients_begin(const float* d_raw, void* scratch, float* grads, int64_t P, void* stream);
int nerf_amd_param_gradients_finish(const void* acts, const void* dys, const void* posx64, const void* posd32,
                                    const void* scratch, float* grads, int64_t P, void* stream);
/* Data-parallel training reduces `grads` in two buckets so the exchange overlaps the arithmetic: bucket 1 =
 * skip_conn_layer ... color_fc.2 (the tail of the vector, whose products run first), bucket 2 = layers_0.* (its
 * head); bucket 0 = everything (= nerf_amd_param_gradients_finish).  nerf_amd_grad_bucket_range gives a bucket's
 * [first, first + count) inside the flat vector.  The caller all-reduces bucket 1 while bucket 2 is computed. */
int nerf_amd_grad_bucket_range(int bucket, int64_t* h_first, int64_t* h_count);
int nerf_amd_param_gradients_finish_bucket(const void* acts, const void* dys, const void* posx64, const void* posd32,
                                           const void* scratch, float* grads, int64_t P, int bucket, void* stream);

/* ---- the same three steps with the saved tensors in the 8-bit storage form ---------------------------------------
 * What the forward saves and the dX chain writes is read by the weight gradients only: sums over all P points
 * (reference train.py:54, loss.backward()).  With NERF_AMD_STORE_E4M3 both buffers hold OCP e4m3 bytes plus one
 * power-of-two exponent per (32 features x 32 points) instead of bf16 -- half the bytes of the step's three
 * HBM-bound kernels; the chain itself still runs on bf16 values in registers, so raw / d_raw / the masks are bit for
 * bit those of the bf16 form, and the gradients differ by the operand rounding of the products only (bounded in
 * tests/test_gpu_storage.py against the reference's minibatch deviation).
 * Layout (csrc/nerf_layout.h): layer L at L * ceil(P/256) * 64 KiB, tile t at t * 64 KiB as
 * [feature/16 (16)][point in tile (256)][16 x e4m3]; behind the 10 layers, per layer and 32-point block 8 exponent
 * bytes (byte Q: features 32Q .. 32Q+31; value = e4m3 * 2^(byte - 127); the producers choose one exponent per 128
 * features, so bytes 4k .. 4k+3 are equal -- a consumer need not rely on it); `acts` then carries the ReLU masks.
 * What no point or feature owns -- the data of points >= P in the last tile and of features past a layer's width, the
 * exponent bytes of 32-point blocks with no point and of fragments past the width -- is written by no producer and looked
 * at by no consumer: the buffers may be allocated uninitialised (the exponent byte 0xFF is e8m0's NaN, and the scaled MFMA
 * returns NaN for it even over zero data, so the products mask the exponents of a slab's absent second block).
 *   nerf_amd_mlp_forward_train(..., flags | NERF_AMD_STORE_E4M3, ...)  with acts of nerf_amd_train_activation_bytes_e4m3(P)
 *   nerf_amd_mlp_backward_e4m3: dys of nerf_amd_train_gradient_bytes_e4m3(P)
 *   nerf_amd_param_gradients_begin (unchanged: packs d_raw into `scratch`);
 *   nerf_amd_param_gradients_convert_e4m3: the narrow operands of the products into `scratch_e4m3`
 *   (nerf_amd_param_gradients_scratch_e4m3_bytes(P)) -- which & 1: the bf16 encoder rows posx64 / posd32 (needs only
 *   nerf_amd_sample_encode_bf16: a captured step runs it beside the forward), which & 2: the packed d_raw of `scratch`
 *   (needs ..._begin: beside the dX chain);
 *   nerf_amd_param_gradients_finish_e4m3: the 14 products on the block-scaled 8-bit MFMA and the bias sums (buckets as in
 *   nerf_amd_param_gradients_finish_bucket). */
#define NERF_AMD_STORE_E4M3 8u /* nerf_amd_mlp_forward_train only */
int64_t nerf_amd_train_activation_bytes_e4m3(int64_t P);
int64_t nerf_amd_train_gradient_bytes_e4m3(int64_t P);
int64_t nerf_amd_param_gradients_scratch_e4m3_bytes(int64_t P);
int nerf_amd_mlp_backward_e4m3(const float* d_raw, const void* bwd_image, const void* acts_e4m3,
                               void* dys_e4m3, int64_t P, void* stream);
int nerf_amd_param_gradients_convert_e4m3(const void* posx64, const void* posd32, const void* scratch,
                                          void* scratch_e4m3, int64_t P, int which, void* stream);
int nerf_amd_param_gradients_finish_e4m3(const void* acts_e4m3, const void* dys_e4m3, const void* scratch_e4m3,
                                         float* grads, int64_t P, int bucket, void* stream);

/* ---- loss: nn.MSELoss(), reference train.py:42,52 -------------------------------- */
/* loss[0] = mean((pred - target)^2) over n elements; g_pred[n] (may be NULL) =
 * d loss / d pred = 2 (pred - target) / n.  One workgroup, fixed summation order. */
int nerf_amd_mse_loss(const float* pred, const float* target, float* loss, float* g_pred,
                      int64_t n, void* stream);

/* ---- optimizer: torch.optim.Adam defaults, reference train.py:43,55 ------------- */
/* One launch over the flat fp32 parameter vector (state_dict order; the 24 tensors are
 * views of it): params, exp_avg, exp_avg_sq updated in place from grads; `step` >= 1 is
 * the 1-based step count used for the bias corrections.  No amsgrad / weight decay, as
 * in the reference.  Follow with nerf_amd_pack_weights on `params`. */
int nerf_amd_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                       int64_t n, float lr, float beta1, float beta2, float eps, int64_t step,
                       void* stream);

/* The reference's jitter draw `torch.rand(B, N)` on torch's CPU default generator
 * (utils/rendering.py:28-30), continued on the GPU with identical values: MT19937, one 32-bit
 * output per float32, u = (tempered & 0xFFFFFF) * 2^-24.  state624: the generator's 624 state
 * words (device memory); next: index of the first unread word of the current block, 0..624
 * (624 = the block is used up); out[n] receives the next n draws; state_out624 the state words
 * afterwards (equal to state624 if no new block was needed).  The host side keeps the
 * generator's counters (utils/host_rng.py reference_rand).  One workgroup; ~1 barrier per 624
 * draws; see nerf_amd_mt19937_uniform_par for long draws. */
int nerf_amd_mt19937_uniform(const uint32_t* state624, int next, float* out, int64_t n,
                             uint32_t* state_out624, void* stream);

/* The same stream produced by several workgroups: after the generator's unread words the stream is
 * cut into segments of seg_words words (a multiple of 624); segment b starts from the state
 * advanced by b * seg_words words, obtained by MT19937 jump-ahead -- polys[m][624] holds
 * x^(seg_words * 2^m) mod the characteristic polynomial (utils/mt19937_jump.npz, made and verified by
 * tools/make_mt_jump.py), m < levels, and the start states follow from the first by a doubling
 * tree of GF(2) convolutions.  levels < 0 selects the one-launch form for short draws instead:
 * polys[j-1][624] holds x^(seg_words * j), j = 1 .. -levels, and every start state is formed from the
 * first directly (up to 1 - levels segments; utils/mt19937_jump.npz holds 63 of them for 39,936-word segments).  seg_states: workspace of nerf_amd_mt19937_segments(next, n,
 * seg_words) * 624 words.  Values and final state identical to nerf_amd_mt19937_uniform. */
int64_t nerf_amd_mt19937_segments(int next, int64_t n, int64_t seg_words);
int nerf_amd_mt19937_uniform_par(const uint32_t* state624, int next, float* out, int64_t n,
                                 uint32_t* state_out624, const uint32_t* polys, int levels,
                                 int64_t seg_words, uint32_t* seg_states, void* stream);

/* The reference's range warning, utils/xyz.py:8-9 (`input not in range -1,1, check rescaling`, raised by every gamma call
 * of positional_encoder when any of the six query-point columns leaves [-1, 1]) without its two device->host syncs:
 * *word |= 1 (uint32 in DEVICE memory, an atomic OR; the caller zeroes and reads it when it likes) if any query point of
 * this call would trigger it.  rays != NULL: the points render_nerf would form from (rays[B,6], u, tbins, flags, seed,
 * ray_id0, N) exactly as the render kernels form them; only the first and the last sample of each ray are looked at (a
 * coordinate is monotone along its ray; with NERF_AMD_TS_GIVEN, whose positions need not be sorted, all N), so the cost is
 * that of 2 B points.  pts != NULL (rays NULL): B FLOATS to test -- the 6 P values of explicit points [P,6], or any
 * gamma() argument.  NaN coordinates do not warn (comparisons with NaN are false), as in the reference. */
int nerf_amd_range_check(const float* rays, const float* pts, const float* u, const float* tbins, uint32_t flags,
                         uint64_t seed, int64_t ray_id0, uint32_t* word, int64_t B, int N, void* stream);

/* ---- ray selection: RayGenerator.select + the ground-truth gather, reference utils/dataload.py:141-153, train.py:47-49 ---- */
/* The raw 32-bit outputs of the same generator (at::mt19937's random()): what `torch.randperm(n)` (dataload.py:151) draws
 * its swap positions from.  Arguments as nerf_amd_mt19937_uniform; state_out624 may be NULL. */
int nerf_amd_mt19937_raw(const uint32_t* state624, int next, uint32_t* out, int64_t n,
                         uint32_t* state_out624, void* stream);
/* HOST function (no GPU): h_poly624 = x^(624 * blocks) mod phi over GF(2), phi = the characteristic polynomial of MT19937's
 * one-word step (h_phi624: 624 little-endian words, `phi` of utils/mt19937_jump.npz).  ~0.1 s; one per table size. */
int nerf_amd_mt19937_jump_poly(int64_t blocks, const uint32_t* h_phi624, uint32_t* h_poly624);
/* state_out624 = the generator's state words (1 + q) blocks after state624's block, poly624 = x^(624 q) mod phi on the
 * device: where torch.randperm(n) leaves the generator after its n - 1 draws, of which nerf_amd_select_rays looks at the
 * first B only.  All 32 bits of all 624 words are torch's.  One launch of 16 workgroups (~85 us). */
int nerf_amd_mt19937_advance(const uint32_t* state624, const uint32_t* poly624, uint32_t* state_out624, void* stream);
/* The jitter draw that FOLLOWS the shuffle in the reference's iteration (train.py:47-51: rg.select, then render_nerf's
 * torch.rand(B, N) from the same generator) without a second dependent jump: out[n] = the n uniforms drawn from the state
 * (1 + q) blocks after state624's block, read from word next_after on -- i.e. from where nerf_amd_mt19937_advance(q) would
 * leave the generator -- with the start states of all `segments` = nerf_amd_mt19937_segments(next_after, n, seg_words) segments
 * formed from state624 in ONE launch: polys[b][624] = x^(624 (q + b * seg_words / 624)) mod phi, b < segments
 * (nerf_amd_mt19937_jump_poly).  state_out624: the state words after the draw; seg_states: workspace, segments * 624 words
 * (seg_states[0] ends up holding the state after the shuffle). */
int nerf_amd_mt19937_uniform_after(const uint32_t* state624, const uint32_t* polys, int segments, int next_after, float* out,
                                   int64_t n, uint32_t* state_out624, int64_t seg_words, uint32_t* seg_states, void* stream);
/* ray_ids = torch.randperm(n)[:B]; rays = table[ray_ids]; gt = colours[ray_ids]   (dataload.py:150-153, train.py:49) with
 * table[n,6] and colours[n,3] resident in HBM.  ids_out[B] (int64, as torch's), rays_out[B,6], gt_out[B,3]: any may be NULL.
 * The permutation prefix is the exact forward Fisher-Yates prefix of torch's CPU randperm (csrc/select.hip), from
 *   draws != NULL: draws[i], i < min(B, n-1): the generator's next 32-bit outputs (nerf_amd_mt19937_raw) -- the
 *                  reference's own ray_ids for the generator's state; seed / seed_mem ignored;
 *   draws == NULL: the counter RNG keyed by seed (+ *seed_mem if seed_mem != NULL: a uint64 in DEVICE memory read when the
 *                  kernel runs, so a launch captured into a hipGraph selects a fresh batch at every replay).
 * B <= n < 2^32 / 20 (beyond, torch.randperm is another algorithm: NERF_AMD_EUNSUP).  workspace: nerf_amd_select_workspace_bytes(B).
 * workspace 16-byte aligned.  Three launches, no atomics on global memory, deterministic. */
int64_t nerf_amd_select_workspace_bytes(int64_t B);
int nerf_amd_select_rays(const uint32_t* draws, uint64_t seed, const uint64_t* seed_mem, int64_t n, int64_t B,
                         const float* table, const float* colours, float* rays_out, float* gt_out, int64_t* ids_out,
                         void* workspace, void* stream);

/* The same update with the step-dependent scalars in DEVICE memory: hyper[6] = {lr, beta1,
 * beta2, eps, 1 - beta1^step, sqrt(1 - beta2^step)} (fp32).  The launch carries no per-step
 * argument, so it can sit inside a captured hipGraph replayed every iteration while the host
 * rewrites `hyper` (training.GraphedTrainStep). */
int nerf_amd_adam_step_hyper(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                             int64_t n, const float* hyper, void* stream);
/* The scalars of a captured step without a copy between graph launches: a ring of slots x 8 floats in PINNED HOST memory
 * (one slot per step, written by the host before it launches the step: the 6 floats of `hyper` above, then whatever the
 * caller keeps in floats 6..7 -- the training step's jitter seed offset as an int64).  nerf_amd_pinned_device_address
 * returns the address under which the device reads such a buffer (hipHostGetDevicePointer; < 0: not pinned / not
 * mapped) -- query it once, outside any capture; nerf_amd_hyper_fetch(ring_dev = that address, ...) copies slot
 * (*counter % slots) into hyper[0..7] on the device and increments *counter (device memory, uint32).  The caller reuses
 * a slot only after the step that read it has been passed by an event. */
int64_t nerf_amd_pinned_device_address(const void* host);
int nerf_amd_hyper_fetch(const float* ring_dev, int slots, float* hyper, uint32_t* counter, void* stream);

/* ---- gradient guard: global-norm clipping and the non-finite step guard, all in device memory -------------------------
 * Between the gradients (behind a data-parallel exchange, so every rank decides alike) and Adam.  `guard` is a record of
 * eight 32-bit words in device memory, 16-byte aligned, allocated and zeroed (but for word 0) by the caller:
 *   0  f32  INPUT max_norm: > 0; +inf = guard only (never clips); may be overwritten in place between launches / replays
 *   1  f32  norm of this step, before clipping, as computed (NaN / inf on a skipped step)
 *   2  f32  coef (0 on a skipped step)
 *   3  u32  skip, 0 / 1
 *   4  u32  steps seen     5  u32  steps skipped     6  u32  steps clipped (coef < 1)     7  0
 * Words 4..6 are running totals kept by one thread with ordinary loads and stores.  Definition, for g = grads[0..n):
 *   S    = sum g_i^2, every square and the sum in double, in a fixed order (a fixed partition of g over a fixed number of
 *          workgroups; per-thread, then wave / block tree, then the block sums in index order; no atomics): two runs
 *          write the same bytes, and a finite fp32 gradient neither overflows nor underflows S
 *   norm = fl32(sqrt(S));   skip <=> norm is not finite (some g_i is NaN or +-inf, or the norm exceeds the fp32 range)
 *   coef = min(1, max_norm / (norm + 1e-6)), three fp32 operations each rounded on its own (torch's clip_grad_norm_);
 *          max_norm = +inf gives exactly 1.  n == 0: norm 0, coef 1, no skip.
 * nerf_amd_grad_guard fills the record (two launches); workspace: nerf_amd_grad_guard_workspace_bytes(n) bytes, 8-byte
 * aligned, contents irrelevant.  grads may be NULL when n == 0. */
int64_t nerf_amd_grad_guard_workspace_bytes(int64_t n);
int nerf_amd_grad_guard(const float* grads, int64_t n, void* workspace, void* guard, void* stream);
/* nerf_amd_adam_step_hyper behind the guard: by definition, bit for bit, nerf_amd_adam_step_hyper on g' = fl32(coef g_i)
 * (one rounded product per element; where coef == 1 the gradient is read as it is) -- and nothing at all where the
 * record's skip word is set: params, exp_avg and exp_avg_sq keep their bits.  The bias corrections in `hyper` stay the
 * caller's, those of the ATTEMPTED step: time passes on a skipped step, so after k skips they are those of step t, not
 * t - k (a relative difference of beta^(t-k) - beta^t, nothing beyond the first few hundred steps).  `guard`: the record
 * nerf_amd_grad_guard filled on the same stream (required whatever n is). */
int nerf_amd_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                               int64_t n, const float* hyper, const void* guard, void* stream);

/* ---- networks of other sizes: Nerf(Lp, Ld, H), reference utils/nets.py:9-32 ---------------- */
/* The fused kernels implement the one configuration the reference constructs (Nerf() = (10, 4, 256): train.py:41,
 * test.py:27).  Every nn.Linear (+ nn.ReLU) of any other size, and its backward (dX = dY W, dW = dY^T X, db = dY^T 1),
 * is this strided fp32 GEMM on the exact-f32 MFMA:
 *     C[i*ldc + j] (+)= sum_k A(i,k) * B(k,j) (+ bias[j]) (ReLU),   i < M, j < N, k < K
 *     A(i,k) = A[i*sa_i + k*sa_k], taken as 0 where A_mask[i*sa_i + k*sa_k] <= 0 (A_mask may be NULL: the ReLU
 *              derivative of a saved activation applied to the incoming gradient);
 *     B(k,j) = B[k*sb_k + j*sb_j] (a weight matrix or a column slice of one, an activation, or one 1.0f with both
 *              strides 0 for column sums).
 * flags: NERF_AMD_LINEAR_RELU, NERF_AMD_LINEAR_ACCUMULATE (C += ; with a long K and few output tiles the reduction is
 * split and summed with float atomics: summation order then varies from run to run).  bias may be NULL. */
#define NERF_AMD_LINEAR_RELU       1u
#define NERF_AMD_LINEAR_ACCUMULATE 2u
int nerf_amd_linear_f32(const float* A, int64_t sa_i, int64_t sa_k, const float* A_mask,
                        const float* B, int64_t sb_k, int64_t sb_j, const float* bias,
                        float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, uint32_t flags, void* stream);

/* ---- gradients with respect to the inputs: query points and rays (pose refinement) ------------------------------ */
/* The reference's render_nerf (utils/rendering.py:13-45), Nerf.forward (utils/nets.py:34-43) and positional_encoder /
 * gamma (utils/xyz.py:6-36) are differentiable in their inputs; these entries give the same gradients.
 *
 * nerf_amd_input_gradients: after nerf_amd_mlp_backward, its dys (bf16, P points) and the flat fp32 parameters (state_dict
 * order; the three weight slices that touch the encoder are rounded to bf16 as the packers round them) ->
 *   points mode (pts [P,6] given, rays == ts == d_rays == NULL): dv [P,6] = d loss / d pts     (utils/nets.py:34-43);
 *   rays mode   (pts == NULL; rays [B,6], ts [B,N] = the sample positions of the forward, P = B*N):
 *               dv [P,6] = d loss / d query points (written, also a workspace), d_rays [B,6] = d loss / d rays
 *               (utils/rendering.py:24-40: x = o + t d, d_hat = d / |d|; t carries no gradient).
 * bf16 MFMA products into the encoder features, fp32 encoder Jacobian on the point recomputed in fp32, rays reduced in
 * sample order; no atomics: bit-identical results run to run. */
int nerf_amd_input_gradients(const void* dys, const float* params, const float* pts, const float* rays, const float* ts,
                             float* dv, float* d_rays, int64_t P, int N, void* stream);
/* d_q [B*N,6] (gradient w.r.t. nerf_amd_query_points' output) -> d_rays [B,6] (utils/rendering.py:24-40), with the
 * ray reduction of nerf_amd_input_gradients.  ts [B,N]: the sample positions the query points were formed with. */
int nerf_amd_query_points_backward(const float* rays, const float* ts, const float* d_q, float* d_rays, int64_t B, int N,
                                   void* stream);
/* backward of nerf_amd_gamma (utils/xyz.py:6-14): d_out [n, 2L] (contiguous) -> d_x [n] */
int nerf_amd_gamma_backward(const float* x, int64_t x_stride, const float* d_out, float* d_x, int64_t n, int L, void* stream);
/* backward of nerf_amd_positional_encoder (utils/xyz.py:16-36): d_posx [P,3+6Lp], d_posd [P,3+6Ld] -> d_vec [P,6] */
int nerf_amd_positional_encoder_backward(const float* vec, const float* d_posx, const float* d_posd, float* d_vec,
                                         int64_t P, int Lp, int Ld, void* stream);

/* ---- camera optimiser: per-image pose corrections (not in the reference) -----------------------------------------------
 * M training images of H x W pixels share the focal length f; image m has the stored pose poses[m] (DEVICE, row-major
 * 3x4 [R0 | t0]) and the learnable correction xi[m] = (w, tau): an axis-angle and a translation, fp32.  The pose the
 * rays are formed from is R = exp([w]x) R0, t = t0 + tau.  xi == NULL is xi == 0.
 *
 * nerf_amd_camera_rays: rays[i] = [t, R dir_cam(h, w)] of the global ray id ids[i] = m H W + h W + w (the row of the
 * table nerf_amd_generate_rays builds image by image), dir_cam as nerf_amd_generate_rays forms it, in its operation
 * order.  With xi[m] == 0 (or xi == NULL) the row equals nerf_amd_generate_rays(poses[m]) bit for bit.  An id outside
 * [0, M H W) writes a row of NaN and reads no pose.  ids_copy (or NULL) receives ids: a captured step keeps the ids it
 * ran on without a launch of its own.  rays, ids and ids_copy 8-byte aligned.
 *
 * nerf_amd_camera_rays_backward: d_rays [B,6] = d loss / d rays -> g_xi [M,6] = d loss / d xi, WRITTEN (not accumulated):
 * g_tau[m] = sum of the origin gradients, g_w[m] = J^T sum (y x g_d) over the batch rows of image m, y the row's world
 * direction and J = I + b K + c K^2 the left Jacobian of the exponential map at w.  Rows in any order, with duplicates;
 * an image without a row gets zeros (B == 0: all of them), an id outside [0, M H W) contributes nothing.  No atomics and
 * a fixed summation order: two runs write the same bytes.  workspace: nerf_amd_camera_workspace_bytes(B, M) bytes (0 in
 * this version: one launch, a block per image; NULL is accepted).  d_rays and g_xi 8-byte aligned.
 *
 * nerf_amd_camera_poses: out[m] = [R | t] (row-major 3x4, 16-byte aligned), the bits the rays kernel uses.
 *
 * Limits: M, B and H W below 2^31 (NERF_AMD_EUNSUP). */
int nerf_amd_camera_rays(const float* poses, const float* xi, const int64_t* ids, int64_t* ids_copy, int H, int W, float f,
                         float* rays, int64_t B, int64_t M, void* stream);
int64_t nerf_amd_camera_workspace_bytes(int64_t B, int64_t M);
int nerf_amd_camera_rays_backward(const float* poses, const float* xi, const int64_t* ids, const float* d_rays, int H, int W,
                                  float f, float* g_xi, void* workspace, int64_t B, int64_t M, void* stream);
int nerf_amd_camera_poses(const float* poses, const float* xi, float* out, int64_t M, void* stream);

/* ---- appearance: a per-image colour correction (gain and bias) trained beside the network (not in the reference) --------
 * M training images of HW pixels each; image m holds theta[m] = (a[3], b[3]) in fp32 (DEVICE, [M,6], zeros = the identity).
 * A ray of image m is compared with its pixel behind
 *     c'_k = (1 + a_k) c_k + b_k,   k = r, g, b,   c = the compositor's rgb (before any clip),
 * evaluated as fl(fl(fl(1 + a) c) + b): three separately rounded fp32 operations per channel, no fma -- torch's eager fp32
 * expression (1 + a) * c + b has the same bits.  The image of a ray is m = id / HW of its global ray id (the row of the table
 * nerf_amd_generate_rays builds image by image, as nerf_amd_camera_rays reads it).
 *
 * nerf_amd_appearance_gather: theta_ray[i] = theta[ids[i] / HW], one row per ray; an id outside [0, M HW) writes a row of NaN
 * and reads no theta -- that ray's colour, loss and d_raw are NaN, no image receives anything from it, and every other ray is
 * what it is alone.  ids_copy (or NULL) receives ids: a captured step keeps the ids it ran on without a launch of its own.
 *
 * nerf_amd_appearance_apply: out[i] = c' of rgb[i] under the row theta_ray + i theta_stride: theta_stride = 6 for one row per
 * ray, 0 for one row for all rays.  out may be rgb.
 *
 * nerf_amd_appearance_apply_backward: g_out [B,3] = d loss / d c' -> g_rgb = g_out fl(1 + a) (may be g_out) and the ray's own
 * row g_theta_ray[i] = (g_out rgb, g_out), each one rounded product.  rgb is the UNCORRECTED colour.
 *
 * nerf_amd_appearance_reduce: g_theta[m] = sum of the rows g_theta_ray[i] with ids[i] / HW == m, WRITTEN (not accumulated), then
 * the gauge: g_theta[m] += reg theta[m] for EVERY image, with or without a row in the batch (the gradient of the ridge
 * (reg / 2) sum ||theta||^2; reg finite and >= 0; an image without a row gets reg theta[m]), or, where frozen (int32 [M], or
 * NULL) is non-zero, exactly zero and no ridge.  An id outside [0, M HW) contributes nothing.  One launch, a block per image,
 * no atomics, no workspace, a fixed summation order: two runs write the same bytes.
 *
 * nerf_amd_volume_render_mse_backward_affine: the training head in one launch -- BY DEFINITION, and bit for bit, the chain
 * nerf_amd_volume_render_rays (rgb) -> nerf_amd_appearance_apply -> g' = 2 (c' - target) / (3 B) as
 * nerf_amd_volume_render_mse_backward forms it -> nerf_amd_appearance_apply_backward -> nerf_amd_volume_render_rays_backward
 * (g_rgb only).  rgb (or NULL) receives c': nerf_amd_mse_loss(rgb, target) is the loss.  g_theta_ray [B,6] and d_raw [B,N,4]
 * are written.  N == 1 is the reference's empty sample axis: rgb = 0, c' = fl(fl(fl(1 + a) 0) + b), d_raw = 0, g_theta_ray =
 * (g' 0, g').  theta == 0 gives nerf_amd_volume_render_mse_backward's d_raw bit for bit.
 *
 * Rules, in this order: NERF_AMD_EINVAL for B < 0, M <= 0, HW <= 0, N <= 0, a theta_stride other than 0 or 6, a reg that is
 * negative or not finite;  B == 0 launches nothing, looks at nothing else and returns 0;  NERF_AMD_EUNSUP for B, M or HW >= 2^31
 * and, for the head, N > 512;  NERF_AMD_EINVAL for a missing pointer (ids_copy, frozen and the head's rgb may be NULL);
 * NERF_AMD_EINVAL for alignment: theta, theta_ray, g_theta_ray, g_theta, ids and ids_copy 8 bytes, raw and d_raw 16, the
 * rest 4. */
int nerf_amd_appearance_gather(const float* theta, const int64_t* ids, int64_t* ids_copy, int64_t HW, float* theta_ray, int64_t B,
                               int64_t M, void* stream);
int nerf_amd_appearance_apply(const float* rgb, const float* theta_ray, int64_t theta_stride, float* out, int64_t B, void* stream);
int nerf_amd_appearance_apply_backward(const float* g_out, const float* rgb, const float* theta_ray, int64_t theta_stride,
                                       float* g_rgb, float* g_theta_ray, int64_t B, void* stream);
int nerf_amd_appearance_reduce(const float* g_theta_ray, const int64_t* ids, int64_t HW, const float* theta, float reg,
                               const int32_t* frozen, float* g_theta, int64_t B, int64_t M, void* stream);
int nerf_amd_volume_render_mse_backward_affine(const float* raw, const float* ts, const float* rays, const float* target,
                                               const float* theta_ray, int64_t theta_stride, float* rgb, float* g_theta_ray,
                                               float* d_raw, int64_t B, int N, void* stream);

/* ---- image metrics: squared error, the reference's PSNR and SSIM on the device (SSIM is not in the reference) -----------
 * pred and gt hold M images of H x W pixels as rows of floats: image m starts at row m H W, a row is `pred_stride`
 * (`gt_stride`) floats apart and its first three floats are r, g, b -- whatever lies behind them (the disparity column of
 * the [H W, 4] pixels a view render returns) is never read.  fp32, data range 1.
 *
 *   sums [M,4] (double):  sse_c = sum over all H W pixels of (pred - gt)^2 per channel -- the difference and its square
 *                         formed in fp32, accumulated in double -- and max_gt = max(gt) over the three channels.
 *                         mse = (sse_r + sse_g + sse_b) / (3 H W);  psnr = -10 log10(mse);  the reference's img_psnr
 *                         (train.py:21-26, peak max(gt)) = 20 log10(max_gt) - 10 log10(mse): left to the caller, in double.
 *   ssim [M,3] (double, or NULL):  per channel the mean over the (H-10)(W-10) window positions of
 *   ssim_map [M, H-10, W-10, 3] (float, or NULL):
 *       (2 mu_a mu_b + C1)(2 s_ab + C2) / ((mu_a^2 + mu_b^2 + C1)(s_aa + s_bb + C2)),  C1 = 0.01^2, C2 = 0.03^2,
 *       mu = sum G x,  s_xy = sum G (x - mu_x)(y - mu_y) over the 11 x 11 window at the position ("valid": no padding),
 *       G_ij = g_i g_j,  g_k = exp(-(k-5)^2 / (2 1.5^2)) normalised to sum 1 in double and rounded once to fp32.
 *       This is tf.image.ssim(max_val = 1) per channel (the image's SSIM is the mean of the three) and skimage's
 *       structural_similarity(gaussian_weights=True, use_sample_covariance=False, data_range=1).  The second moments are
 *       evaluated CENTRED, in a second pass behind the means, every operation rounded on its own: each map value lies
 *       within a few units of 2^-24 of the float64 value where E[x^2] - mu^2 loses 5e-4 on a white background
 *       (DESIGN.md section 27), and pred == gt gives exactly 1.
 *   ssim == NULL and ssim_map == NULL: squared error and max_gt only, for any H, W >= 1.
 *
 * A NaN pixel makes sse and -- through every window that contains it -- the SSIM of its own channel of its own image
 * NaN and touches nothing else; a NaN in gt makes max_gt NaN.  Two launches (tiles, then one block per image adds the
 * tiles' partial sums in a fixed order), no atomics: two runs write the same bytes, and M images in one call give what M
 * calls give.  workspace: nerf_amd_image_metrics_workspace_bytes(M, H, W) bytes, 8-byte aligned.
 *
 * Rules, in this order: NERF_AMD_EINVAL for M < 0, H <= 0, W <= 0 or a stride below 3;  M == 0 launches nothing and
 * returns 0 (the size query: 0);  NERF_AMD_EUNSUP for H W >= 2^31 (or a workspace size that leaves an int64);
 * NERF_AMD_EUNSUP for H < 11 or W < 11 when ssim or ssim_map is given;  NERF_AMD_EINVAL for a missing pred, gt, sums or
 * workspace;  NERF_AMD_EINVAL for alignment: sums, ssim and workspace 8 bytes, pred, gt and ssim_map 4.  The size query
 * applies the first three. */
int64_t nerf_amd_image_metrics_workspace_bytes(int64_t M, int H, int W);
int nerf_amd_image_metrics(const float* pred, int64_t pred_stride, const float* gt, int64_t gt_stride, double* sums, double* ssim,
                           float* ssim_map, void* workspace, int64_t M, int H, int W, void* stream);

/* ---- density grid and surface extraction (not in the reference) ------------------------------------------------------
 * The reference can only evaluate sigma through the whole Nerf.forward (utils/nets.py:34-43) and has no mesh export.
 *
 * nerf_amd_density_forward: sigma[P] = raw sigma (pre-softplus, column 3 of nerf_amd_mlp_forward's output) of the points
 * pts[P, stride >= 3] (their first three columns).  Not in the reference.  sigma does not depend on the view direction
 * (sigma_fc reads h8 before the direction concat, utils/nets.py:36-40): the kernel runs layers 0..7 and the sigma row of
 * layers_2 only (82.6 % of the MFMAs of the bf16 forward, 92.7 % of the folded fp16 one's) with the arithmetic of nerf_amd_mlp_forward, and equals its column 3 bit for bit.
 * precision: NERF_AMD_BF16 or NERF_AMD_FP16 on the image of nerf_amd_pack_weights (NERF_AMD_F32: NERF_AMD_EUNSUP -- run
 * nerf_amd_grid_points + nerf_amd_mlp_forward instead).  The range guard of the 16-bit kernels applies: status word 0 is
 * set on a non-finite accumulator in layers 1..7 or a non-finite sigma (nerf_amd_packed_status_offset).
 *
 * nerf_amd_density_grid: the same on the grid points of an [nx, ny, nz] volume, formed in the kernel (no input buffer):
 * sigma[(i ny + j) nz + k] (C order, z fastest) at (x(i), y(j), z(k)), x_a(i) = fl(lo_a + fl(i step_a)) with two separately
 * rounded float32 operations -- torch's float32 `lo + i * step` is the same number.  h_lo[3], h_step[3]: HOST floats
 * (the conventional step is fl32((hi - lo) / (n - 1))).  Each extent in [2, 2^24], at most 2^40 points (64-bit indices).
 *
 * nerf_amd_grid_points: pts6[count, 6] = (x(i), y(j), z(k), 0, 0, 1) of grid points first .. first + count - 1, the same
 * coordinates: the input of the fp32 forward (or of another network size) on a chunk of the grid.  Not in the reference. */
int nerf_amd_density_forward(const float* pts, int64_t stride, void* packed, int precision, float* sigma, int64_t P,
                             void* stream);
int nerf_amd_density_grid(const float* h_lo, const float* h_step, int64_t nx, int64_t ny, int64_t nz, void* packed,
                          int precision, float* sigma, void* stream);
int nerf_amd_grid_points(const float* h_lo, const float* h_step, int64_t nx, int64_t ny, int64_t nz, int64_t first,
                         int64_t count, float* pts6, void* stream);

/* Marching cubes on an fp32 volume sigma[nx, ny, nz] (C order, z fastest; any device volume, e.g. nerf_amd_density_grid's).
 * Not in the reference.  Semantics (tests/mesh_model.py restates them in numpy, bit for bit):
 *   - a corner is inside iff sigma > level (a tie is outside); an edge crosses iff exactly one endpoint is inside and both
 *     are finite; a cell with a non-finite corner emits no face;
 *   - one vertex per crossing edge.  On edge a -> b (a = the endpoint with the lower linear index):
 *     t = fl(fl(level - sa) / fl(sb - sa)); on the edge's axis x = fl(xa + fl(t fl(xb - xa))), the other two coordinates
 *     are exact grid coordinates x_a(i) = fl(lo_a + fl(i step_a));
 *   - normal: -grad sigma by central differences on the grid (one-sided on the grid's faces: (s[hi] - s[lo]) /
 *     (x(hi) - x(lo))), interpolated with t between the endpoints and normalised: it points outward, towards lower sigma;
 *     a zero or non-finite one is (0, 0, 0);
 *   - vertices are numbered by (linear index of the lower endpoint, axis x < y < z), faces by (linear cell index, table
 *     order); faces are int32 vertex triples, oriented outward;
 *   - the case tables are generated by rule (tools/make_mc_tables.py): on each cube face the crossing edges are joined by
 *     a rule that depends on that face's four corners only (an ambiguous face separates its inside corners), the segments
 *     chain into loops and each loop is fanned.  A surface that stays inside the grid gives a closed, consistently
 *     oriented mesh: every edge belongs to two faces, once in each direction.
 * Deterministic: fixed partitions and hand-written scans, no atomics -- every run writes the same bytes.
 *
 * nerf_amd_marching_cubes_workspace_bytes: bytes of the workspace both passes share (about 5 per grid point).
 * nerf_amd_marching_cubes_count: counts[2] (DEVICE int64) = (vertices, faces).  Also fills the workspace for _emit.
 * nerf_amd_marching_cubes_emit: after _count on the same sigma, extents, level and workspace: verts[V,3], normals[V,3]
 *   (may be NULL), faces[F,3].  Writes vertex v only if v < max_verts and face f only if f < max_faces -- never past the
 *   capacities; the mesh is complete when max_verts >= counts[0] and max_faces >= counts[1].  max_verts < 2^31 (vertex
 *   numbers are int32: a vertex count of 2^31 or more cannot be emitted). */
int64_t nerf_amd_marching_cubes_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
int nerf_amd_marching_cubes_count(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float level, void* workspace,
                                  int64_t* counts, void* stream);
int nerf_amd_marching_cubes_emit(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float level, const float* h_lo,
                                 const float* h_step, void* workspace, float* verts, float* normals, int32_t* faces,
                                 int64_t max_verts, int64_t max_faces, void* stream);

/* ---- occupancy grid and the masked render: skip the samples that lie in empty space (inference; not in the reference) ---
 * Grid: [nx, ny, nz] grid points (the axes of nerf_amd_density_grid: x_a(i) = fl(lo_a + fl(i step_a))) make
 * C = (nx - 1, ny - 1, nz - 1) cells; cell (i, j, k) spans points i .. i + 1, j .. j + 1, k .. k + 1.  Semantics
 * (tests/occupancy_model.py restates them in numpy, bit for bit):
 *   - packing: one bit per cell, z fastest, 32 cells per uint32: cell (i, j, k) is bit (k & 31) of word
 *     (i Cy + j) Wz + (k >> 5), Wz = ceil(Cz / 32); every z row is padded to a whole word and the padding bits are zero.
 *     nerf_amd_occupancy_grid_words = Cx Cy Wz.  A set bit means live.
 *   - from a sigma volume: a cell is DEAD iff every corner of every cell within `dilate` cells of it (Chebyshev distance,
 *     clipped at the grid's edge) has sigma <= level; a NaN corner therefore makes it live.  0 <= dilate <= 15.
 *   - cell of a point, per axis, in float32 with separately rounded operations: c = floor(fl(fl(x - lo) * inv_step)), where
 *     h_inv_step is fl32(1 / step) formed on the host.  c < 0, c >= C or a NaN coordinate on any axis: the point is
 *     OUTSIDE, and is live unless NERF_AMD_OUTSIDE_EMPTY is given.  Otherwise it is live iff its cell's bit is set.
 *   - the sample positions ts[B,N] and points o + d t of a ray are exactly those of nerf_amd_query_points /
 *     nerf_amd_render_forward for the same (u, tbins, flags, seed, ray_id0); no stage reads or writes them in memory.
 *   - mask[B, ceil(N / 64)] uint64: bit (i & 63) of word i >> 6 of a ray is set iff sample i is live (bits >= N are zero).
 *     offsets[B + 1] int64: exclusive scan of the rays' live counts; offsets[B] = the live count P'.
 *   - the masked render is volume_render over all N samples with the network's output replaced by (0, 0, 0, -inf) at a dead
 *     sample: alpha = w = 0 exactly there, the delta of a live sample is still the distance to the NEXT SAMPLE, dead or not.
 *     It equals nerf_amd_query_points -> nerf_amd_mlp_forward on all B N points -> dead rows overwritten ->
 *     nerf_amd_volume_render_rays (_pixels) bit for bit.  A ray with no live sample: rgb = acc = 0, disparity NaN.
 * N <= 768 and B <= 2^32 (NERF_AMD_EUNSUP beyond).  No atomics: fixed partitions, hand-written scans, same bytes every run.
 *
 * nerf_amd_occupancy_from_density: bits <- sigma[nx, ny, nz] (fp32, C order), level, dilate.
 * nerf_amd_occupancy_from_mask:    bits <- cells[Cx, Cy, Cz], one byte per cell (non-zero = live).
 * nerf_amd_occupancy_mark: stages mark + scan.  flags: the jitter flags, plus NERF_AMD_OUTSIDE_EMPTY.  h_lo[3], h_inv_step[3]:
 *   HOST floats.  Writes mask, offsets[B + 1] and, if not NULL, *live = P' (DEVICE int64: the host reads it to size the next
 *   two buffers -- the one synchronisation of a masked render).  workspace: nerf_amd_occupancy_workspace_bytes(B), 16-aligned.
 * nerf_amd_occupancy_points: pts[P', 6] = the rows of nerf_amd_query_points of the live samples, ray-major, sample order
 *   inside a ray: the input of nerf_amd_mlp_forward.  Writes row r only if r < max_points.
 * nerf_amd_volume_render_masked(_pixels): raw_live[P', 4] = the network's output on those points (NULL allowed when P' = 0);
 *   outputs as nerf_amd_volume_render_rays (alpha / w [B, N] or NULL) / nerf_amd_volume_render_pixels. */
#define NERF_AMD_OUTSIDE_EMPTY 16u /* nerf_amd_occupancy_mark only: a sample outside the grid is dead (default: live) */
int64_t nerf_amd_occupancy_grid_words(int64_t nx, int64_t ny, int64_t nz);
int nerf_amd_occupancy_from_density(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float level, int dilate,
                                    uint32_t* bits, void* stream);
int nerf_amd_occupancy_from_mask(const uint8_t* cells, int64_t nx, int64_t ny, int64_t nz, uint32_t* bits, void* stream);
int64_t nerf_amd_occupancy_mask_words(int64_t B, int N);
int64_t nerf_amd_occupancy_workspace_bytes(int64_t B);
int nerf_amd_occupancy_mark(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed,
                            int64_t ray_id0, const uint32_t* bits, int64_t nx, int64_t ny, int64_t nz, const float* h_lo,
                            const float* h_inv_step, uint64_t* mask, int64_t* offsets, int64_t* live, void* workspace,
                            int64_t B, int N, void* stream);
int nerf_amd_occupancy_points(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed,
                              int64_t ray_id0, const uint64_t* mask, const int64_t* offsets, float* pts, int64_t max_points,
                              int64_t B, int N, void* stream);
int nerf_amd_volume_render_masked(const float* raw_live, const float* rays, const float* u, const float* tbins, uint32_t flags,
                                  uint64_t seed, int64_t ray_id0, const uint64_t* mask, const int64_t* offsets, float* rgb,
                                  float* disp, float* alpha, float* acc, float* w, int64_t B, int N, void* stream);
int nerf_amd_volume_render_masked_pixels(const float* raw_live, const float* rays, const float* u, const float* tbins,
                                         uint32_t flags, uint64_t seed, int64_t ray_id0, const uint64_t* mask,
                                         const int64_t* offsets, float* pixels, int64_t B, int N, void* stream);

/* ---- training with the occupancy grid: the masked compositor's backward and the running density volume ------------------
 * Not in the reference.  tests/occupancy_train_model.py restates both in torch / numpy.
 *
 * nerf_amd_volume_render_masked_backward: d loss / d raw_live[P', 4] of nerf_amd_volume_render_masked, for the same
 *   (raw_live, rays, u, tbins, flags, seed, ray_id0, mask, offsets), given the upstream gradients of its five outputs:
 *   g_rgb[B,3], g_disp[B], g_alpha[B,N], g_acc[B], g_w[B,N] (dense [B,N], whatever the mask; any of them NULL = zero).
 *   Semantics: d_raw_live is the rows at the live samples of nerf_amd_volume_render_rays_backward run on the dense
 *   raw[B,N,4] whose dead rows hold (0, 0, 0, -inf), with the sample positions of nerf_amd_query_points.  A dead sample has
 *   softplus' = 0, alpha = 0 and w = 0 in that kernel: it receives nothing and contributes exact zeros to the suffix sums.
 *   One wavefront per ray, no atomics: row offsets[ray] + rank is written by exactly one lane, nothing outside [0, P') is
 *   written, and every run writes the same bytes.  A ray with no live sample writes nothing.  At N = 1 (the reference's
 *   empty sample axis) every live row gets zeros.  N <= 512 like the dense backward (NERF_AMD_EUNSUP beyond; N <= 0 is
 *   NERF_AMD_EINVAL).  With P' = 0 raw_live and d_raw_live may both be NULL; otherwise both are given, 16-byte aligned.
 *   Arguments are checked on the host before any launch.
 *
 * nerf_amd_occupancy_decay_max: state[i] = max(fl(state[i] * decay), softplus(sigma_now[i])), i < n, in place.
 *   sigma_now: raw sigma on the grid points (nerf_amd_density_grid); softplus is the compositor's (beta = 1, identity
 *   above 20), so state is a density, >= 0, fp32.  A NaN on either side gives NaN, which
 *   nerf_amd_occupancy_from_density treats as live.  The bits of a training grid are
 *   nerf_amd_occupancy_from_density(state, softplus(level), dilate).  0 <= decay <= 1 (NERF_AMD_EINVAL otherwise). */
int nerf_amd_volume_render_masked_backward(const float* raw_live, const float* rays, const float* u, const float* tbins,
                                           uint32_t flags, uint64_t seed, int64_t ray_id0, const uint64_t* mask,
                                           const int64_t* offsets, const float* g_rgb, const float* g_disp,
                                           const float* g_alpha, const float* g_acc, const float* g_w, float* d_raw_live,
                                           int64_t B, int N, void* stream);
int nerf_amd_occupancy_decay_max(float* state, const float* sigma_now, float decay, int64_t n, void* stream);

/* ---- graphed masked training step: device-side live count, fixed capacity (csrc/occupancy_graph.hip) -------------------
 * Not in the reference.  tests/occupancy_graphed_model.py restates the semantics in numpy.
 *
 * A masked step captured into a graph has no host in it, so the live count P' = offsets[B] of a batch can size nothing.
 * Such a step is captured for a fixed point CAPACITY C, 1 <= C <= B N: every network kernel (nerf_amd_mlp_forward_train_points,
 * nerf_amd_encode_points_bf16, nerf_amd_mlp_backward, nerf_amd_param_gradients_begin, nerf_amd_param_gradients_finish_bucket)
 * runs with P = C on every replay, P' comes from nerf_amd_occupancy_mark and stays on the device, and the two entry points
 * below make the rows that no live sample owns inert:
 *   - kept samples: sample i of ray b is KEPT iff its mask bit is set and its global rank
 *     r = offsets[b] + (set bits of the ray below i) is < C.  mask_C is the mask with every other bit cleared,
 *     offsets_C = min(offsets, C) its scan.  The step IS the masked step above with mask_C / offsets_C in place of
 *     mask / offsets.  With P' <= C nothing changes; with P' > C (an OVERFLOW) the tail of the live samples in ray-major
 *     order is dead -- (0, 0, 0, -inf), contributing exactly nothing and receiving no gradient: a well-defined,
 *     deterministic step under a stricter mask, never an out-of-bounds access.  It is reported through `counts`.
 *   - surplus rows r in [min(P', C), C): pts[r] = NERF_AMD_OCCUPANCY_PAD_POINT (inside the network's input range),
 *     d_raw_live[r] = 0, so the dX chain and the dW / db products add exact zeros for them.  Every byte of pts[C, 6] and
 *     d_raw_live[C, 4] is written on every launch: nothing of an earlier replay survives.
 *   - counts: DEVICE int64[2] = {P', min(P', C)}, written on every launch.
 * Both: one wavefront per ray for the kept rows, a grid-stride tail for the surplus rows, no atomics (the two row ranges
 * are disjoint; every run writes the same bytes).  Jitter flags as the other masked stages, NERF_AMD_DEVICE_RNG |
 * NERF_AMD_SEED_IN_MEMORY included (a node of a replayed graph).  Arguments are checked on the host before any launch:
 * NULL or misaligned buffers (mask, offsets, counts 8 bytes; raw_live, d_raw_live 16), B < 0, N <= 0, capacity < 1 or
 * > B N (so B = 0 as well), unknown flags: NERF_AMD_EINVAL; N > 512 (the masked backward's limit) or B > 2^32:
 * NERF_AMD_EUNSUP.
 *
 * nerf_amd_occupancy_points_capped: pts[C, 6]; rows r < min(P', C) bit for bit the rows of nerf_amd_occupancy_points.
 * nerf_amd_volume_render_masked_mse_backward: the training head of the masked step in one launch, nerf_amd_volume_render_masked
 *   (rgb only) -> g_rgb = 2 (rgb - gt) / (3 B), formed in the kernel as nerf_amd_volume_render_mse_backward forms it ->
 *   nerf_amd_volume_render_masked_backward, all under mask_C / offsets_C.  raw_live[C, 4]: the network's output on pts
 *   (rows >= min(P', C) are never read).  Writes rgb[B, 3] (bit for bit the masked compositor's; 0 for a ray with nothing
 *   kept) and all of d_raw_live[C, 4].  At N = 1 (the reference's empty sample axis) every row gets zeros. */
#define NERF_AMD_OCCUPANCY_PAD_POINT {0.f, 0.f, 0.f, 0.f, 0.f, -1.f}   /* (x, y, z, d1, d2, d3): the origin, looking down -z */
int nerf_amd_occupancy_points_capped(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed,
                                     int64_t ray_id0, const uint64_t* mask, const int64_t* offsets, float* pts,
                                     int64_t* counts, int64_t capacity, int64_t B, int N, void* stream);
int nerf_amd_volume_render_masked_mse_backward(const float* raw_live, const float* rays, const float* u, const float* tbins,
                                               uint32_t flags, uint64_t seed, int64_t ray_id0, const uint64_t* mask,
                                               const int64_t* offsets, const float* gt, float* rgb, float* d_raw_live,
                                               int64_t capacity, int64_t B, int N, void* stream);

/* ---- masked hierarchical pair: one occupancy grid for the coarse and the fine pass (csrc/occupancy_graph.hip) ----------
 * Not in the reference.  tests/occupancy_hierarchical_model.py restates the semantics in numpy; DESIGN.md section 15.
 *
 * ONE grid masks both passes (while training it follows the FINE network).  The masked hierarchical render is BY DEFINITION
 * this composition of existing entry points:
 *   1. coarse pass: the masked render above on the Nc stratified samples (mark -> emit -> network on the live points ->
 *      masked compositor): rgb_c and w_c[B, Nc], w_c = 0 exactly at a dead sample; the coarse positions ts_c are those of
 *      nerf_amd_query_points for the same jitter.
 *   2. sampler: ts_f = nerf_amd_sample_pdf(ts_c, w_c (detached), Nf, u_f | counter RNG); the coarse samples are kept and
 *      merged, as in the dense pair.  A ray with no live coarse sample has w_c == 0 and the sampler's 1e-5 floor makes its
 *      fine samples uniform: the defined result, not an error.
 *   3. fine pass: the masked render with NERF_AMD_TS_GIVEN on ts_f[B, Nc + Nf] through the SAME grid, by the fine network.
 *   Training loss: MSE(rgb_c, gt) + MSE(rgb_f, gt); the coarse network learns from its own term only.
 * Limits (the intersection of the parts'): the default network, bf16 training kernels, 3 <= Nc <= 256, Nc + Nf <= 512, no
 * gradients to the rays.
 *
 * nerf_amd_volume_render_masked_mse_backward_pdf: the masked COARSE head of a captured pair step, one launch, one wavefront per
 *   ray: nerf_amd_volume_render_masked (rgb and w) -> g_rgb = 2 (rgb - gt) / (3 B) -> nerf_amd_volume_render_masked_backward ->
 *   nerf_amd_sample_pdf(ts_c, w, ...), every stage under mask_C / offsets_C of the graphed masked step above.  rgb[B, 3] and
 *   ts_out[B, Nc + Nf] are bit for bit that composition's; d_raw_live[C, 4] is the fused masked head's (kept rows from the
 *   sweep, rows behind min(P', C) exact zeros, every byte written on every launch).  w never reaches HBM.
 *   u / tbins / flags / seed / ray_id0: the COARSE jitter, as the other masked stages (NERF_AMD_TS_GIVEN: u = ts_c[B, Nc]).
 *   The Nf new samples: u_f[B, Nf], or with NERF_AMD_DEVICE_RNG the counter RNG under nerf_amd_sample_pdf's key (seed,
 *   ray_id0) -- with NERF_AMD_SEED_IN_MEMORY the same 64-bit offset at `u` is added to the seed of both draws, exactly as
 *   nerf_amd_volume_render_mse_backward_pdf honours it (a node of a replayed graph).
 *   Checked on the host before any launch: the rules of the two entry points above (NULL or misaligned buffers, B < 0,
 *   Nc <= 0, Nf < 0, capacity < 1 or > B Nc, unknown flags, NERF_AMD_TS_GIVEN without u, no u_f without the counter RNG when
 *   Nf > 0: NERF_AMD_EINVAL) and the sampler's limits (Nc < 3, Nc > 256, Nc + Nf > 512, B > 2^32: NERF_AMD_EUNSUP). */
int nerf_amd_volume_render_masked_mse_backward_pdf(const float* raw_live, const float* rays, const float* u, const float* tbins,
                                                   uint32_t flags, uint64_t seed, int64_t ray_id0, const uint64_t* mask,
                                                   const int64_t* offsets, const float* gt, const float* u_f, float* rgb,
                                                   float* d_raw_live, float* ts_out, int64_t capacity, int64_t B, int Nc,
                                                   int Nf, void* stream);

/* ---- terminated render: early ray termination for the masked and dense inference renders (csrc/occupancy_terminate.hip) --
 * Not in the reference.  tests/termination_model.py restates the semantics in numpy; DESIGN.md section 16.
 *
 * An occupancy grid removes the samples in front of a surface; termination removes those behind an opaque one.  Semantics:
 *   - slabs: a ray's N samples are cut into slabs of S consecutive sample indices, S in {16, 32, 64} (a slab never straddles
 *     a 64-sample chunk of the compositor); the last slab may be short; K = ceil(N / S).
 *   - threshold: 0 < eps < 1.
 *   - M0: the occupancy mask of the masked render above (every sample when there is no grid).
 *   - before slab k the ray's transmittance T_k is formed: the transmittance entering the first sample of slab k over the
 *     rows evaluated so far, in the compositor's arithmetic (the product scan of fl(fl(1 - alpha) + 1e-10) over the 64-chunk,
 *     times the carry of the earlier chunks: bit for bit the T the masked compositor forms for that sample from the same
 *     rows).  T_0 = 1.  The ray is TERMINATED from slab k on iff T_k < eps.  A NaN T_k is not terminated: termination never
 *     hides a NaN.  Every factor is <= 1 in fp32, so T does not grow and termination is permanent; it is also permanent by
 *     construction: a terminated ray evaluates nothing more and its T is frozen, T_j = T_k for j > k (the scan's product
 *     tree is not associative to the last bit, so a re-formed T could differ from T_k in an ulp).
 *   - evaluated mask: M* = M0 & (the slab of sample i is not terminated).
 *   - result: the terminated render is BY DEFINITION the masked render above under M*: volume_render over all N samples with
 *     the network's output replaced by (0, 0, 0, -inf) at every sample outside M*.  Nothing else about the arithmetic changes.
 *   Consequences: each rgb channel differs from the un-terminated masked render by less than eps max|c| over the dropped
 *   samples (their weights sum to less than the transmittance that reached them, < eps), acc by less than eps;
 *   alpha = w = 0 exactly at a dropped sample; a ray that never terminates is bit for bit what it was.
 *
 * nerf_amd_termination_advance: one step of the slab loop, for the slab [s0, s1) just evaluated and the next slab [s1, s2).
 *   The first call is (s0, s1, s2) = (0, 0, min(S, N)) with raw_slab = NULL; then (k S, min((k + 1) S, N), min((k + 2) S, N));
 *   the call with s1 = s2 = N only retires the last slab.  Per ray (one wavefront):
 *   1. retire: row offsets_slab[ray] + popcount(mask_slab bits below i) of raw_slab[rows_slab, 4] -- the network's output on
 *      the slab's compacted points (nerf_amd_occupancy_points under mask_slab / offsets_slab, an earlier call's mask_next /
 *      offsets_next) -- goes to row offsets0[ray] + popcount(M0 bits below i) of raw0[rows0, 4], the M0 layout.  The caller
 *      pre-fills raw0 with (0, 0, 0, -inf); a row never written IS a dead sample, so after the last call
 *      nerf_amd_volume_render_masked(_pixels)(raw0, mask0, offsets0) yields the defined result.  raw_slab = NULL (with
 *      rows_slab = 0): nothing to retire (the first call, or a slab no ray had a live sample in).  No row is read or written
 *      at or past rows_slab / rows0.
 *   2. transmittance: T entering sample s1 from the rows of the current 64-chunk in raw0 (chunk start to s1) and the carry of
 *      the earlier chunks (kept in `workspace` between calls); positions recomputed from (u, tbins, flags, seed, ray_id0) as the
 *      masked compositor recomputes them, or read under NERF_AMD_TS_GIVEN.  T -> trans[B, K], column s1 / S (s1 < N).
 *   3. select: mask_next[B, ceil(N / 64)] = M0 & [s1, s2) & !(T < eps), offsets_next[B + 1] its exclusive scan, and
 *      totals (DEVICE int64[2]): [0] the live count of the next slab, [1] the live samples of M0 at or beyond s1 on rays
 *      still alive.  The host stops when totals[1] is 0.
 *   workspace: nerf_amd_termination_workspace_bytes(B) bytes, 16-aligned, ONE buffer kept through all calls of a render (the
 *   first call initialises it).  mask_next / offsets_next must not be the buffers given as mask_slab / offsets_slab.
 *   Checked on the host before any launch -- NERF_AMD_EINVAL: NULL or misaligned buffers, B < 0, N <= 0, negative row counts,
 *   unknown flags or a jitter tensor missing, eps outside (0, 1) or NaN, S not 16, 32 or 64, slab bounds that are not the
 *   multiples of S stated above (clipped at N) or are out of order, raw_slab with s0 = s1 or without its mask and offsets,
 *   rows_slab > 0 without raw_slab; NERF_AMD_EUNSUP: N > 768 or B > 2^32.  B = 0: nothing is launched or written.
 *   No atomics, fixed partitions: two runs write the same bytes. */
int64_t nerf_amd_termination_workspace_bytes(int64_t B);
int nerf_amd_termination_advance(const float* raw_slab, const uint64_t* mask_slab, const int64_t* offsets_slab, int64_t rows_slab,
                                 const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed,
                                 int64_t ray_id0, const uint64_t* mask0, const int64_t* offsets0, float* raw0, int64_t rows0,
                                 float eps, int slab, int s0, int s1, int s2, float* trans, uint64_t* mask_next,
                                 int64_t* offsets_next, int64_t* totals, void* workspace, int64_t B, int N, void* stream);

/* ---- grid-guided fine sampling: importance samples from a sigma volume (csrc/guided_sample.hip) --------------------------
 * Not in the reference.  tests/guided_model.py restates the look-up and the composition in numpy; DESIGN.md section 21.
 *
 * The hierarchical path places its Nf fine samples from the weights of a coarse NETWORK.  Here the weights come from a sigma
 * VOLUME on a grid instead (nerf_amd_density_grid's output): Nc table look-ups per ray in place of Nc network evaluations.
 * The guided sample placement is BY DEFINITION this composition of existing entry points plus one exact table look-up:
 *   1. coarse positions: ts_c[B, Nc] and the points o + d t are those of nerf_amd_query_points for (u, tbins, flags, seed,
 *      ray_id0).  Every jitter mode is accepted: explicit u, NERF_AMD_TS_GIVEN, NERF_AMD_DEVICE_RNG, and
 *      NERF_AMD_DEVICE_RNG | NERF_AMD_SEED_IN_MEMORY.
 *   2. look-up: V[nx, ny, nz] is fp32 in C order (z fastest) and holds raw sigma at the grid points of the density grid's
 *      axes, exactly what nerf_amd_density_grid writes.  The cell of a point is the occupancy rule above, op for op: per axis
 *      c = floor(fl(fl(x - lo) * inv_step)), h_lo[3] and h_inv_step[3] HOST floats.  A point is OUTSIDE when !(0 <= c < n - 1)
 *      on any axis; a NaN coordinate is outside.  The value inside is the maximum over the cell's 8 corners V[cx + a, cy + b,
 *      cz + c], a, b, c in {0, 1}; the maximum starts from -inf and skips NaN corners.  The value outside, or in a cell whose
 *      8 corners are all NaN, is -inf.  There is no rounding anywhere in the look-up, and a NaN in the volume never reaches
 *      the sampler.
 *   3. weights: w_c[B, Nc] is the `w` output of nerf_amd_volume_render_rays on raw = (0, 0, 0, value), ts_c and rays.  The
 *      compositor's softplus applies, so a value of -inf gives alpha = w = 0 exactly.
 *   4. sampler: ts_out[B, Nc + Nf] = nerf_amd_sample_pdf(ts_c, w_c, u_f, ...): u_f[B, Nf], or with NERF_AMD_DEVICE_RNG that
 *      entry point's own key (seed, ray_id0).  With NERF_AMD_SEED_IN_MEMORY the 64-bit offset at `u` is added to the seed of
 *      both draws, exactly as nerf_amd_volume_render_mse_backward_pdf does.  A ray with all-zero weights gets the sampler's
 *      uniform placement: that is the defined result, not an error.
 * The guided render is the existing render with NERF_AMD_TS_GIVEN on ts_out; the guided training loss is MSE(rgb, gt) of ONE
 * network on those positions, and ts_out carries no gradient.
 *
 * nerf_amd_sample_pdf_volume: one launch, one wavefront per ray; w_c stays in LDS unless asked for.  sigma_c[B, Nc] (the
 *   look-up's values) and w_c[B, Nc] are optional outputs (NULL: not written); ts_out does not depend on them.
 *   Checked on the host before any launch, in this order -- NERF_AMD_EINVAL: Nf < 0, B < 0, Nc <= 0, unknown flags or a jitter
 *   tensor missing; NERF_AMD_EUNSUP: Nc < 3, Nc > 256, Nc + Nf > 512, B > 2^32; NERF_AMD_EINVAL: an axis < 2, no u_f without
 *   the counter RNG when Nf > 0; B = 0: nothing is launched or written; NERF_AMD_EINVAL: a NULL rays, sigma_volume, h_lo,
 *   h_inv_step or ts_out, or a device buffer not aligned to 4 bytes.  No atomics: two runs write the same bytes. */
int nerf_amd_sample_pdf_volume(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed,
                               int64_t ray_id0, const float* sigma_volume, int64_t nx, int64_t ny, int64_t nz,
                               const float* h_lo, const float* h_inv_step, const float* u_f, float* ts_out, float* sigma_c,
                               float* w_c, int64_t B, int Nc, int Nf, void* stream);

/* ---- masked guided placement: guided sampling through an occupancy grid (csrc/guided_masked.hip) -------------------------
 * Not in the reference.  tests/guided_masked_model.py restates it in numpy; DESIGN.md section 24.
 *
 * The guided sampler does not know the occupancy grid: left alone it places fine samples in cells the masked render then
 * discards.  The masked guided placement looks at the grid twice -- at the coarse samples in front of the weights, and at the
 * merged positions.  For (rays, u, tbins, flags, seed, ray_id0), a sigma volume V, an occupancy grid G with its outside policy
 * and u_f it is BY DEFINITION, bit for bit, this chain of existing entry points:
 *   1. ts_c[B, Nc] and the points: nerf_amd_query_points.
 *   2. value_i: the look-up of the guided placement above (maximum over the 8 corners of the point's cell in V, NaN corners
 *      skipped, -inf outside).
 *   3. mask_c: nerf_amd_occupancy_mark on the same coarse jitter through G (the jitter flags, plus NERF_AMD_OUTSIDE_EMPTY when
 *      given); value_i := -inf where the bit is clear -- the rule of the masked pair: the sampler sees weights that are exactly
 *      0 at a dead sample.
 *   4. w_c: the `w` output of nerf_amd_volume_render_rays on raw = (0, 0, 0, value).
 *   5. ts_out[B, Nc + Nf] = nerf_amd_sample_pdf(ts_c, w_c, u_f, ...) under the sampler's key; with NERF_AMD_SEED_IN_MEMORY the
 *      64-bit offset at `u` is added to the seed of both draws, as in the guided placement.
 *   6. mask[B, ceil((Nc + Nf) / 64)], offsets[B + 1], live = offsets[B]: nerf_amd_occupancy_mark with NERF_AMD_TS_GIVEN on
 *      ts_out, through the same G and policy.
 * Hence: an all-live grid gives nerf_amd_sample_pdf_volume's ts_out and a full mask; a ray with no live coarse sample gets the
 * sampler's uniform placement; a new sample may still land in a dead cell (the sampler's 1e-5 floor, a bin that straddles a
 * boundary) and is then simply masked; V and G may differ in resolution and bounds.  The masked guided render and training
 * step are the existing masked render / masked step with NERF_AMD_TS_GIVEN on ts_out under this mask and these offsets.
 *
 * nerf_amd_sample_pdf_volume_masked: the placement kernel (one wavefront per ray) followed by the mark's three scan kernels.
 *   flags: the jitter flags (NERF_AMD_DEVICE_RNG | NERF_AMD_SEED_IN_MEMORY included), plus NERF_AMD_OUTSIDE_EMPTY.
 *   sigma_volume[vx, vy, vz] with v_lo[3], v_inv_step[3]; bits of the grid of (gx, gy, gz) grid points with g_lo[3],
 *   g_inv_step[3]: the four axis arrays are HOST floats.  Optional outputs (NULL: not written): sigma_c[B, Nc], the value AFTER
 *   step 3; w_c[B, Nc]; live, a DEVICE int64.  workspace: nerf_amd_occupancy_workspace_bytes(B) bytes, 16-byte aligned.
 *   Checked on the host before any launch, in this order -- nerf_amd_sample_pdf_volume's rules (NERF_AMD_EINVAL: Nf < 0, B < 0,
 *   Nc <= 0, unknown flags or a jitter tensor missing; NERF_AMD_EUNSUP: Nc < 3, Nc > 256, Nc + Nf > 512, B > 2^32;
 *   NERF_AMD_EINVAL: a volume axis < 2, no u_f without the counter RNG when Nf > 0); NERF_AMD_EINVAL: a grid axis < 2; B = 0:
 *   returns 0, and offsets[0] = 0 (*live = 0) is written as nerf_amd_occupancy_mark writes it at B = 0 when offsets and
 *   workspace are given and aligned; NERF_AMD_EINVAL: a NULL rays, sigma_volume, v_lo, v_inv_step, bits, g_lo, g_inv_step,
 *   ts_out, mask, offsets or workspace, or a buffer not aligned (mask, offsets, live: 8 bytes; workspace: 16; the rest: 4).
 *   No atomics: two runs write the same bytes. */
int nerf_amd_sample_pdf_volume_masked(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed,
                                      int64_t ray_id0, const float* sigma_volume, int64_t vx, int64_t vy, int64_t vz,
                                      const float* v_lo, const float* v_inv_step, const uint32_t* bits, int64_t gx, int64_t gy,
                                      int64_t gz, const float* g_lo, const float* g_inv_step, const float* u_f, float* ts_out,
                                      float* sigma_c, float* w_c, uint64_t* mask, int64_t* offsets, int64_t* live,
                                      void* workspace, int64_t B, int Nc, int Nf, void* stream);

/* ---- background colour and sigma noise for the dense training path ----------------------------------------------------
 * Two controls every NeRF trainer offers and the reference does not (white_bkgd and raw_noise_std elsewhere; the noise is the
 * reference's own `## TODO add gaussian noise regularizer`, utils/rendering.py:63).  Dense single-network path only.
 *
 * nerf_amd_sigma_noise: raw[B,N,4] -> out[B,N,4] (out may be raw): the colours are copied, sigma' = sigma + std z goes in
 *   column 3 (two rounded ops; it replaces sigma in front of the softplus, utils/rendering.py:63-64, d sigma' / d sigma = 1).
 *   z = sqrt(-2 ln u1) cos(2 pi u2) is a standard normal from the counter RNG whatever the jitter source is: key =
 *   (seed + offset) ^ NOISE_KEY -- a key of its own, apart from the jitter's, the sampler's and the ray selection's --
 *   where offset is 0, or with flags = NERF_AMD_SEED_IN_MEMORY the uint64 at the DEVICE ADDRESS seed_mem (8-byte aligned;
 *   a node of a replayed graph: step k draws what seed + k draws); sample (ray_id0 + ray) N + i owns the counters
 *   2 s and 2 s + 1, so the noise does not depend on how the rays are batched or sharded.  u1 in (0, 1] from the top 24
 *   bits of the first word plus one, u2 in [0, 1) from the second.  std == 0: out = raw, no noise code runs.
 *   NERF_AMD_EINVAL: B < 0, N <= 0; std < 0 or not finite; any other flag; NERF_AMD_SEED_IN_MEMORY with a NULL or
 *   misaligned seed_mem -- in this order, all before the empty problem (B == 0: nothing is launched) and the pointers.
 *   A training control: the inference renders do not take it. */
int nerf_amd_sigma_noise(const float* raw, float* out, float std, uint32_t flags, uint64_t seed, const uint64_t* seed_mem,
                         int64_t ray_id0, int64_t B, int N, void* stream);

/* nerf_amd_background_blend: a background colour behind the volume, applied to a ray's composited rgb[B,3] and acc[B]:
 *   rgb_bg[c] = rgb[c] + (1 - acc) bg[c], the subtraction, the product and the sum each rounded on its own (no fma), so the
 *   torch fp32 expression rgb + (1 - acc) * bg has the same bits.  bg: one colour [3] (bg_stride = 0) or one per ray [B,3]
 *   (bg_stride = 3, in floats); it carries no gradient.  Outputs, either may be NULL (not both): rgb_out[B,3] = rgb_bg and
 *   pixels[B,4] = [clip(rgb_bg, 0, 1), disp] -- the clip comes after the blend and passes NaN through, as the compositor's
 *   does (utils/rendering.py:103-105); disp[B] is read for pixels only.  disp, alpha, acc and w are what they were.  At
 *   N == 1 (rgb = acc = 0) rgb_bg = bg exactly.
 * nerf_amd_background_blend_backward: g_rgb passes through; g_acc[B] = -((g0 bg0 + g1 bg1) + g2 bg2) from g = g_rgb_bg[B,3],
 *   every product and sum rounded on its own, in that order.  g_acc is WRITTEN, not accumulated: the caller adds its own
 *   term and hands the sum to nerf_amd_volume_render_rays_backward.
 * Both: NERF_AMD_EINVAL for B < 0, then for bg_stride not in {0, 3}; B == 0 launches nothing; then NERF_AMD_EINVAL for a
 *   missing pointer. */
int nerf_amd_background_blend(const float* rgb, const float* acc, const float* disp, const float* bg, int64_t bg_stride,
                              float* rgb_out, float* pixels, int64_t B, void* stream);
int nerf_amd_background_blend_backward(const float* g_rgb_bg, const float* bg, int64_t bg_stride, float* g_acc, int64_t B,
                                       void* stream);

/* nerf_amd_volume_render_mse_backward_bg: the training head with both controls, ONE launch.  By definition, bit for bit
 *   (tests/test_gpu_background.py), it is the composition
 *     nerf_amd_sigma_noise (std, flags, seed, seed_mem, ray_id0)          (the regulariser of utils/rendering.py:63)
 *     -> nerf_amd_volume_render_rays (rgb, acc) -> nerf_amd_background_blend
 *     -> g = 2 (rgb_bg - target) / (3 B), as nerf_amd_volume_render_mse_backward forms it
 *     -> nerf_amd_background_blend_backward -> nerf_amd_volume_render_rays_backward (g_rgb = g, g_acc)
 *   raw, ts, rays, target[B,3] -> rgb[B,3] = rgb_bg (may be NULL; nerf_amd_mse_loss on it is the step's loss) and
 *   d_raw[B,N,4].  Each sample's noise is generated once, as its chunk is loaded.  bg == NULL: no background (bg_stride is
 *   still checked); std == 0: no noise; with both it IS nerf_amd_volume_render_mse_backward.  N <= 512 (NERF_AMD_EUNSUP
 *   beyond); at N == 1 rgb = bg (0 without one) and d_raw = 0.  Rules in order: sizes; the noise arguments as in
 *   nerf_amd_sigma_noise; bg_stride; B == 0; the size limit; the pointers. */
int nerf_amd_volume_render_mse_backward_bg(const float* raw, const float* ts, const float* rays, const float* target,
                                           const float* bg, int64_t bg_stride, float std, uint32_t flags, uint64_t seed,
                                           const uint64_t* seed_mem, int64_t ray_id0, float* rgb, float* d_raw, int64_t B, int N,
                                           void* stream);

/* nerf_amd_volume_render_mse_backward_pdf_bg: the COARSE head of the coarse + fine pair with both controls, ONE launch:
 *   nerf_amd_volume_render_mse_backward_pdf with the term block (bg, bg_stride, std, noise_flags, noise_seed, seed_mem) of
 *   nerf_amd_volume_render_mse_backward_bg in front of the sampler's arguments.  By definition, bit for bit
 *   (tests/test_gpu_pair_controls.py), rgb[B,3] = rgb_bg and d_raw[B,Nc,4] are the chain of that entry point at N = Nc, and
 *   ts_out[B,Nc+Nf] is nerf_amd_sample_pdf (u, flags, seed, ray_id0) on the w of that chain's compositor: the sampler sees
 *   the weights of the NOISY compositor, the background never touches them, and w never reaches HBM.  ray_id0 is shared by
 *   the sampler and the noise; the noise has flags, seed and seed_mem of its own (a pair's fine pass draws its noise under
 *   noise_seed + 2^63: two streams, since the counter (ray_id0 + ray) N + i of two passes with different N would share words
 *   across rays under one key).  The distortion term is not offered here: it belongs on the final weights.
 *   bg == NULL: no background (bg_stride is still checked); std == 0: no noise; with both it IS
 *   nerf_amd_volume_render_mse_backward_pdf (the same launch).  3 <= Nc <= 256, Nc + Nf <= 512 (NERF_AMD_EUNSUP beyond).
 *   Rules in order: sizes and the sampler's jitter arguments as nerf_amd_volume_render_mse_backward_pdf; the noise arguments
 *   as in nerf_amd_sigma_noise; bg_stride; B == 0; the size limit; the pointers. */
int nerf_amd_volume_render_mse_backward_pdf_bg(const float* raw, const float* ts, const float* rays, const float* target,
                                               const float* bg, int64_t bg_stride, float std, uint32_t noise_flags,
                                               uint64_t noise_seed, const uint64_t* seed_mem, const float* u, uint32_t flags,
                                               uint64_t seed, int64_t ray_id0, float* rgb, float* d_raw, float* ts_out, int64_t B,
                                               int Nc, int Nf, void* stream);

/* ---- distortion loss for the dense training path -------------------------------------------------------------------------
 * mip-NeRF 360's regulariser on a ray's compositing weights (the w of utils/rendering.py:68), which pulls them together into
 * one compact interval.  For one ray with positions t_0 <= ... <= t_{N-1} and the far plane t_far:
 *     delta_i = t_{i+1} - t_i (i < N - 1), delta_{N-1} = max(t_far - t_{N-1}, 0)     (the compositor's 1e10, clipped)
 *     m_i     = t_i + delta_i / 2
 *     D       = 2 sum_i w_i sum_{j<i} w_j (m_i - m_j) + (1/3) sum_i w_i^2 delta_i
 *     dD/dw_i = 2 [ sum_{j<i} w_j (m_i - m_j) + sum_{j>i} w_j (m_j - m_i) ] + (2/3) w_i delta_i
 * This ORDERED form is the definition; it equals sum_ij w_i w_j |m_i - m_j| + (1/3) sum w_i^2 delta_i on nondecreasing
 * positions, which every sampler here produces and nothing checks.  Positions carry no gradient.  O(N) per ray: one
 * wavefront per ray, prefix and suffix sums of w and w m (m centred on t_0), every operation rounded on its own; no atomics:
 * every run writes the same bytes.  A sample with w_i == 0 contributes exact zeros; a NaN weight stays inside its ray.
 *
 * nerf_amd_distortion_loss: ts[B,N], w[B,N] -> loss_ray[B] = coef D and g_w[B,N] = coef dD/dw; either output may be NULL (not
 *   both).  A training step's term is lambda / (B (tf - tn)) sum_rays D: coef = lambda / (B (tf - tn)) formed in double and
 *   rounded once, t_far = tf (mip-NeRF 360's normalised distance: D is homogeneous of degree 1 in t).  N == 1 is the
 *   reference's empty sample axis: loss_ray = 0, g_w = 0.  N <= 512.
 *   Rules in order: NERF_AMD_EINVAL for B < 0 or N <= 0; for t_far or coef not finite or coef < 0; B == 0 launches nothing;
 *   NERF_AMD_EUNSUP for N > 512 (or B > 2^32); NERF_AMD_EINVAL for a missing pointer. */
int nerf_amd_distortion_loss(const float* ts, const float* w, float t_far, float coef, float* loss_ray, float* g_w, int64_t B,
                             int N, void* stream);

/* nerf_amd_sum_f32: out[0] = the sum of x[n], one workgroup and a fixed summation order (as nerf_amd_mse_loss): the same bits
 *   from run to run.  The step's distortion term from loss_ray.  NERF_AMD_EINVAL for n <= 0 or a missing pointer. */
int nerf_amd_sum_f32(const float* x, float* out, int64_t n, void* stream);

/* nerf_amd_volume_render_mse_backward_dist: the training head with the distortion term, ONE launch.  By definition, bit for
 *   bit (tests/test_gpu_distortion.py), it is the composition
 *     nerf_amd_sigma_noise (std, flags, seed, seed_mem, ray_id0)
 *     -> nerf_amd_volume_render_rays (rgb, acc, w) -> nerf_amd_distortion_loss (t_far, coef) on that w: loss_ray, g_w
 *     -> nerf_amd_background_blend -> g = 2 (rgb_bg - target) / (3 B) -> nerf_amd_background_blend_backward
 *     -> nerf_amd_volume_render_rays_backward (g_rgb = g, g_acc, g_w)
 *   so d_raw[B,N,4] is the gradient of MSELoss(rgb_bg, target) + sum_rays coef D.  rgb[B,3] = rgb_bg and loss_ray[B] may be
 *   NULL.  bg == NULL: no background (bg_stride is still checked); std == 0: no noise; with both it is the plain chain.
 *   coef == 0: rgb and d_raw are nerf_amd_volume_render_mse_backward_bg's and loss_ray is all zeros.  N <= 512; at N == 1
 *   rgb = bg (0 without one), loss_ray = 0 and d_raw = 0.  Rules in order: sizes; the noise arguments as in
 *   nerf_amd_sigma_noise; bg_stride; t_far and coef as in nerf_amd_distortion_loss; B == 0; the size limit; the pointers. */
int nerf_amd_volume_render_mse_backward_dist(const float* raw, const float* ts, const float* rays, const float* target,
                                             const float* bg, int64_t bg_stride, float std, uint32_t flags, uint64_t seed,
                                             const uint64_t* seed_mem, int64_t ray_id0, float t_far, float coef, float* rgb,
                                             float* loss_ray, float* d_raw, int64_t B, int N, void* stream);

/* ---- masked training controls: background, sigma noise and distortion loss for the masked steps (csrc/masked_controls.hip) --
 * The three terms of the dense training path for the masked single-network steps (one network behind an occupancy grid,
 * plain or on guided positions), and the background and the noise for the coarse head of the masked pair.  Definitions of mask, offsets, the live rows raw_live[P',4]
 * and the capacity clamp: "training with the occupancy grid" and "graphed masked training step" above.
 *
 * nerf_amd_sigma_noise_masked: the noise stage on live rows, raw_live[P',4] -> out[P',4] (out may be raw_live).  Row
 *   offsets[b] + rank of the live sample i of ray b (rank = live samples of the ray in front of it) gets its colours copied
 *   and sigma' = sigma + std z, z the standard normal nerf_amd_sigma_noise draws for sample (ray_id0 + b) N + i: the counter is
 *   the ORIGINAL sample index, so an all-live grid reproduces nerf_amd_sigma_noise bit for bit.  std == 0: out = raw_live, no
 *   noise code runs.  flags / seed / seed_mem as in nerf_amd_sigma_noise.  N <= 512.  P' = offsets[B] is known to the device
 *   only: raw_live == out == NULL says P' == 0, launches nothing and returns 0.
 *   Rules in order: NERF_AMD_EINVAL for B < 0 or N <= 0; the noise arguments as in nerf_amd_sigma_noise; B == 0 launches
 *   nothing; NERF_AMD_EUNSUP for N > 512 (or B > 2^32); NERF_AMD_EINVAL for a missing or misaligned mask / offsets (8 bytes), for
 *   exactly one of raw_live / out missing, or either off 16 bytes. */
int nerf_amd_sigma_noise_masked(const float* raw_live, float* out, float std, uint32_t flags, uint64_t seed,
                                const uint64_t* seed_mem, int64_t ray_id0, const uint64_t* mask, const int64_t* offsets, int64_t B,
                                int N, void* stream);

/* nerf_amd_volume_render_masked_mse_backward_dist: the masked training head with the three terms, ONE launch under the capacity
 *   clamp.  By definition, bit for bit (tests/test_gpu_masked_controls.py), it is the composition under mask_C / offsets_C --
 *   the stricter mask nerf_amd_volume_render_masked_mse_backward defines: kept iff live and global rank < capacity --
 *     nerf_amd_sigma_noise_masked (std, noise_flags, noise_seed, seed_mem, ray_id0)
 *     -> nerf_amd_volume_render_masked (rgb, acc, w) -> nerf_amd_distortion_loss (ts, w, t_far, coef): loss_ray, g_w
 *     -> nerf_amd_background_blend -> g = 2 (rgb_bg - gt) / (3 B) -> nerf_amd_background_blend_backward
 *     -> nerf_amd_volume_render_masked_backward (g_rgb = g, g_acc, g_w)
 *   so the kept rows of d_raw_live[capacity,4] are the gradient of MSELoss(rgb_bg, gt) + sum_rays coef D, and the surplus rows
 *   [min(P', capacity), capacity) are zero-filled on every launch: every row is written by exactly one lane, no atomics, two
 *   runs write the same bytes.  rgb[B,3] = rgb_bg.  ray_id0 is shared by the jitter and the noise; the noise has flags, seed
 *   and seed_mem of its own.  A dead or over-capacity sample is dead whatever the noise: it is (0, 0, 0, -inf), never noised,
 *   alpha = w = 0 exactly.  A ray with nothing kept, or N == 1: rgb = bg through the blend's own rounded ops (0 without a
 *   background), loss_ray = 0, a kept row gets zeros.
 *   bg == NULL: no background (bg_stride is still checked); std == 0: no noise; coef == 0: no distortion term -- rgb and
 *   d_raw_live are the chain without it and loss_ray (may be NULL) is all zeros.  With none of the three it IS
 *   nerf_amd_volume_render_masked_mse_backward (the same launch; a loss_ray that is given is cleared by a memset in front of
 *   it).  N <= 512.
 *   Rules in order: NERF_AMD_EINVAL for capacity < 1, B < 0, N <= 0 or the jitter arguments, as the plain masked head; the noise
 *   arguments as in nerf_amd_sigma_noise; bg_stride; t_far and coef as in nerf_amd_distortion_loss; B == 0 (NERF_AMD_EINVAL:
 *   1 <= capacity <= B N leaves B >= 1); NERF_AMD_EUNSUP for N > 512 (or B > 2^32); NERF_AMD_EINVAL for missing rays,
 *   capacity > B N, a missing or misaligned mask / offsets, a missing raw_live / gt / rgb / d_raw_live, raw_live or d_raw_live
 *   off 16 bytes. */
int nerf_amd_volume_render_masked_mse_backward_dist(const float* raw_live, const float* rays, const float* u, const float* tbins,
                                                    uint32_t flags, uint64_t seed, int64_t ray_id0, const uint64_t* mask,
                                                    const int64_t* offsets, const float* gt, const float* bg, int64_t bg_stride,
                                                    float std, uint32_t noise_flags, uint64_t noise_seed, const uint64_t* seed_mem,
                                                    float t_far, float coef, float* rgb, float* loss_ray, float* d_raw_live,
                                                    int64_t capacity, int64_t B, int N, void* stream);

/* nerf_amd_volume_render_masked_mse_backward_pdf_bg: the COARSE head of the masked pair with the background and the noise,
 *   ONE launch under the capacity clamp: nerf_amd_volume_render_masked_mse_backward_pdf with the term block (bg, bg_stride,
 *   std, noise_flags, noise_seed, seed_mem) of the head above behind gt.  By definition, bit for bit
 *   (tests/test_gpu_pair_controls.py), rgb and d_raw_live are the head above with coef = 0 at N = Nc, and ts_out[B,Nc+Nf] is
 *   nerf_amd_sample_pdf (u_f, the jitter's flags, seed, ray_id0) on the w of that chain's masked compositor under mask_C:
 *   the weights of the NOISY compositor, exactly 0 at a dead or over-capacity sample whatever std is; a ray with nothing kept
 *   gets rgb = bg and the sampler's uniform placement.  The distortion term is not offered (it belongs on the final weights).
 *   bg == NULL and std == 0: it IS nerf_amd_volume_render_masked_mse_backward_pdf (the same launch).
 *   Rules in order: as nerf_amd_volume_render_masked_mse_backward_pdf up to the jitter arguments; the noise arguments as in
 *   nerf_amd_sigma_noise; bg_stride; then that entry point's again: NERF_AMD_EUNSUP for the sampler's sizes (or B > 2^32);
 *   NERF_AMD_EINVAL for missing rays, capacity > B Nc (so B == 0), a missing or misaligned mask / offsets, a missing raw_live /
 *   gt / rgb / d_raw_live / ts_out, raw_live or d_raw_live off 16 bytes. */
int nerf_amd_volume_render_masked_mse_backward_pdf_bg(const float* raw_live, const float* rays, const float* u, const float* tbins,
                                                      uint32_t flags, uint64_t seed, int64_t ray_id0, const uint64_t* mask,
                                                      const int64_t* offsets, const float* gt, const float* bg, int64_t bg_stride,
                                                      float std, uint32_t noise_flags, uint64_t noise_seed,
                                                      const uint64_t* seed_mem, const float* u_f, float* rgb, float* d_raw_live,
                                                      float* ts_out, int64_t capacity, int64_t B, int Nc, int Nf, void* stream);

/* ---- scene box: a ray's samples placed inside an axis-aligned box (csrc/ray_box.hip, csrc/ray_box_device.h) ---------------
 * Not in the reference, whose samples lie in linspace(tn, tf, N + 1) bins whatever the ray (utils/rendering.py:24-30): this
 * generalises that line to a per-ray interval.  tests/box_model.py restates it op for op; DESIGN.md section 33.
 *
 * nerf_amd_box_positions: ts[B,N], the positions of N samples per ray inside the box [h_lo, h_hi] (HOST float[3] each, finite,
 * lo < hi on every axis).  Per ray (o, d), d un-normalised as render_nerf uses it; fp32, every operation rounded on its own
 * (no fma contraction); min / max are comparisons that let a NaN through:
 *   1. slabs, per axis a: d_a != 0 -- ta = (lo_a - o_a) / d_a, tb = (hi_a - o_a) / d_a, near_a = min(ta, tb), far_a = max(ta, tb);
 *      d_a == 0 (either sign) with lo_a <= o_a <= hi_a -- the axis constrains nothing; d_a == 0 otherwise -- the ray misses.
 *   2. interval: t0 = max(tn, near_x, near_y, near_z), t1 = min(tf, far_x, far_y, far_z), folded in that order;
 *      hit = (t0 < t1), false for a NaN: a ray with a NaN component is a miss.
 *   3. a miss keeps the whole interval, t0 = tn, t1 = tf: it renders as it does without a box (and is dead as a whole behind a
 *      grid whose outside is empty).  No special values, no NaN.
 *   4. unit positions c[N]: bit for bit the ts nerf_amd_query_points forms for this ray's (u, flags, seed, ray_id0) on
 *      tbins01 = linspace(0, 1, N + 1) -- every jitter mode of that rule: u, NERF_AMD_DEVICE_RNG, with NERF_AMD_SEED_IN_MEMORY
 *      (then `u` is the address of the offset), and NERF_AMD_TS_GIVEN, where u[B,N] holds unit positions of the caller's own
 *      and tbins01 is not looked at.
 *   5. ts_i = min(t0 + (t1 - t0) c_i, t1): ascending whenever c is; a position may land one rounding outside the box.
 * Outputs: ts[B,N]; span[B,2] = (t0, t1) and hit[B] (int32 0 / 1), each skipped when NULL.  Feed ts to any entry point under
 * NERF_AMD_TS_GIVEN.  One wavefront per ray, every element written by exactly one lane, no atomics: two runs write the same
 * bytes.  Nothing here carries a gradient: the positions are constants of the render, as the fine sampler's are.
 * Rules in order -- NERF_AMD_EINVAL: h_lo / h_hi NULL, not finite or lo_a >= hi_a; tn or tf not finite or !(tn < tf);
 * B < 0 or N <= 0; unknown flags, NERF_AMD_TS_GIVEN without u, no u without the counter RNG, a seed address missing or off
 * 8 bytes, tbins01 NULL unless NERF_AMD_TS_GIVEN.  NERF_AMD_EUNSUP: N > 768 or B > 2^32 (the masked entry points that read ts).
 * NERF_AMD_EINVAL: rays NULL with B > 0, ts NULL with B > 0, a buffer off 4 bytes.  B == 0: nothing is launched or written. */
int nerf_amd_box_positions(const float* rays, const float* u, const float* tbins01, uint32_t flags, uint64_t seed,
                           int64_t ray_id0, const float* h_lo, const float* h_hi, float tn, float tf, float* ts, float* span,
                           int32_t* hit, int64_t B, int N, void* stream);

/* ---- grid span: a ray's samples placed between its first and its last live cell (csrc/grid_span.hip, grid_span_device.h) ---
 * The scene box's successor and not in the reference either: the interval is cut PER RAY from an occupancy grid's bits (layout
 * above, "occupancy grid"), read in place, so nerf_amd_occupancy_from_density between two launches simply takes effect.
 * tests/grid_span_model.py restates it op for op; DESIGN.md section 39.
 *
 * nerf_amd_span_positions: ts[B,N] for the grid of (nx, ny, nz) grid points, C_a = n_a - 1 cells per axis, bounds [h_lo, h_hi]
 * and h_inv_step = 1 / cell size (HOST float[3] each), K = probes segments.  Per ray (o, d), d un-normalised; fp32, every
 * operation rounded on its own (fl), no fma contraction:
 *   1. clip to the grid: [a, b] and hit are the scene box's steps 1-3 with the box [h_lo, h_hi].  A slab miss -- which covers any
 *      NaN component -- reads nothing: hit = 0 and the interval is [tn, tf].
 *   2. K segments: edges e_0 = a, e_K = b exactly and e_j = fl(a + fl(fl(b - a) * fl(j / K))) between; segment j is
 *      [e_j, e_j+1].  The point of an edge is p = fl(o + fl(e * d)) per axis, its cell index floor(fl(fl(p - lo) * inv_step))
 *      CLAMPED into [0, C - 1] by comparisons that send a NaN to 0, before any address is formed: no input reads outside `bits`.
 *      Segment j is live iff any of the 8 cells (c0|c1)_x x (c0|c1)_y x (c0|c1)_z of its two edges' indices has its bit set.
 *   3. the interval: with j0 / j1 the first / last live segment, t0 = e_j0, t1 = e_(j1+1), hit = 1; with no live segment hit = 0
 *      and [t0, t1] = [tn, tf]: the ray renders as it did, and behind a grid whose outside is empty it is dead as a whole.
 *   4. ts_i = min(t0 + (t1 - t0) c_i, t1) on the unit positions c of the scene box's step 4: every jitter mode of that rule.
 * The host rule probes >= 2 max(C_a) makes a segment at most half a cell long per axis, so every cell it crosses is among the
 * 8: the span is CONSERVATIVE -- no point of the ray in [tn, tf] that lies in a live cell lies outside [t0, t1], up to fp32
 * rounding at a cell face.  a <= t0 <= t1 <= b, and t0 < t1 unless [a, b] is only a few roundings long.  With every cell live
 * the result is nerf_amd_box_positions' for the box [h_lo, h_hi], bit for bit.  There is no outside policy: the span speaks for
 * the grid's cells only.
 * Outputs and determinism as nerf_amd_box_positions: ts[B,N]; span[B,2] and hit[B] (int32 0 / 1), each skipped when NULL; one
 * wavefront per ray (64 segments per ballot; the chunks between the first and the last live one are not looked at), every
 * element written by exactly one lane, no atomics.  Nothing here carries a gradient.
 * Rules in order -- NERF_AMD_EINVAL: bits NULL; h_lo / h_hi / h_inv_step NULL or not finite, or lo_a >= hi_a; a grid extent
 * below 2 (or beyond the grid entry points' limits); probes below 64, not a multiple of 64 or below 2 max(C_a); tn / tf, B / N
 * and the jitter rules as nerf_amd_box_positions.  NERF_AMD_EUNSUP: probes > 1024, N > 768 or B > 2^32.  NERF_AMD_EINVAL: rays
 * NULL with B > 0, ts NULL with B > 0, a buffer (bits included) off 4 bytes.  B == 0: nothing is launched or written. */
int nerf_amd_span_positions(const float* rays, const float* u, const float* tbins01, uint32_t flags, uint64_t seed,
                            int64_t ray_id0, const uint32_t* bits, int64_t nx, int64_t ny, int64_t nz, const float* h_lo,
                            const float* h_hi, const float* h_inv_step, int probes, float tn, float tf, float* ts, float* span,
                            int32_t* hit, int64_t B, int N, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERF_AMD_H */
