// api.hip -- the C ABI of libnerf_amd.so (include/nerf_amd.h): argument
// checking, host-side introspection and the composition of the render path
// out of the kernels in this directory.  No allocation, no host sync.
#include "api_checks.h"
#include "launchers.h"
#include <math.h>

using namespace nerf_layout;

namespace {
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline bool bad_precision(int p) { return p != NERF_AMD_F32 && p != NERF_AMD_BF16 && p != NERF_AMD_FP16; }
inline bool bad_image(int p) { return bad_precision(p) && p != NERF_AMD_BF16_BWD; }
// the fused render kernels (sampling + MLP + compositing in one launch) serve rays of up to
// FUSED_RENDER_MAX_N samples, in every precision
inline bool fused_render(int precision, int N) { return !bad_precision(precision) && N <= FUSED_RENDER_MAX_N; }
int launch_mlp(const MlpArgs& a, int rays_mode, int precision, hipStream_t s) {
    if (precision == NERF_AMD_F32) return nerf_amd_launch_mlp_f32(&a, rays_mode, s);
    if (precision == NERF_AMD_FP16) return nerf_amd_launch_mlp_f16_16(&a, rays_mode, s);
    return nerf_amd_launch_mlp_bf16_16(&a, rays_mode, s);
}
// a density / marching-cubes grid: every extent in [2, 2^24], at most 2^40 points
constexpr int64_t GRID_MAX_EXTENT = 1ll << 24, GRID_MAX_POINTS = 1ll << 40;
inline bool bad_grid(int64_t nx, int64_t ny, int64_t nz) {
    for (int64_t r : {nx, ny, nz})
        if (r < 2 || r > GRID_MAX_EXTENT) return true;
    return nx * ny > GRID_MAX_POINTS / nz;
}
inline DensityArgs grid_args(const float* h_lo, const float* h_step, int64_t nx, int64_t ny, int64_t nz) {
    DensityArgs a{};
    a.P = nx * ny * nz; a.ny = ny; a.nz = nz;
    for (int i = 0; i < 3; ++i) { a.lo[i] = h_lo[i]; a.step[i] = h_step[i]; }
    return a;
}
int launch_density(const DensityArgs& a, int precision, hipStream_t s) {
    return precision == NERF_AMD_FP16 ? nerf_amd_launch_density_f16(&a, s) : nerf_amd_launch_density_bf16(&a, s);
}
// the masked render's stages (the mark / emit / composite kernels form the sample positions themselves)
int occ_rays(const float* rays, const float* u, const float* tbins, uint32_t flags, int64_t B, int N) {
    return masked_rays_check(rays, u, tbins, flags, B, N, N > MASKED_MAX_N);
}

// ---- workspace layouts: the *_workspace_bytes function and the entry point that carves the buffer read the same struct ----
struct RenderWs {                      // the two-launch render: raw[B,N,4] at 0, ts[B,N]; nothing on the fused path
    int64_t off_ts, bytes;
};
RenderWs render_ws(int precision, int64_t B, int N) {
    if (fused_render(precision, N)) return {0, 0};
    const int64_t raw = align256(B * N * 16);
    return {raw, raw + align256(B * N * 4)};
}
struct ImageWs {                       // rays[n,6] at 0, then the render's own workspace
    int64_t off_render, bytes;
};
ImageWs image_ws(int precision, int64_t n_rays, int N) {
    const int64_t rays = align256(n_rays * 24);
    return {rays, rays + render_ws(precision, n_rays, N).bytes};
}
struct HierWs {                        // rays[n,6] at 0, ts_c[n,Nc], w_c[n,Nc], ts_f[n,Nc+Nf]
    int64_t off_ts_c, off_w_c, off_ts_f, bytes;
};
HierWs hier_ws(int64_t n_rays, int Nc, int Nf) {
    HierWs w;
    w.off_ts_c = align256(n_rays * 24);
    w.off_w_c = w.off_ts_c + align256(n_rays * Nc * 4);
    w.off_ts_f = w.off_w_c + align256(n_rays * Nc * 4);
    w.bytes = w.off_ts_f + align256(n_rays * (int64_t)(Nc + Nf) * 4);
    return w;
}

// ---- the render of a batch of rays: every render entry point ends here --------------------------------------------------
struct RenderOut {                     // rgb / disp / acc (alpha and w on request), or pixels
    float *rgb, *disp, *alpha, *acc, *w, *pixels;
};
// `a`: rays_args + packed.  One fused launch (sampling + MLP + compositing) up to FUSED_RENDER_MAX_N samples; beyond, the
// MLP leaves raw / ts in the workspace (render_ws) and the compositor reads them.
int render_rays(MlpArgs a, const RenderOut& out, int precision, void* workspace, hipStream_t s) {
    const bool fused = fused_render(precision, a.N);
    if (!fused && !workspace) return NERF_AMD_EINVAL;
    if (!a.rays || !a.packed) return NERF_AMD_EINVAL;
    if (bad_jitter(a.flags, a.u, a.tbins)) return NERF_AMD_EINVAL;
    if (fused) {
        a.rgb = out.rgb; a.disp = out.disp; a.alpha = out.alpha; a.acc = out.acc; a.w = out.w; a.pixels = out.pixels;
        return launch_mlp(a, 1, precision, s);
    }
    const int64_t B = a.P / a.N;
    a.raw = reinterpret_cast<float*>(workspace);
    a.ts_out = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + render_ws(precision, B, a.N).off_ts);
    const int rc = launch_mlp(a, 1, precision, s);
    if (rc) return rc;
    // dirs = rays[:,3:] normalised inside the kernel (utils/rendering.py:37,43)
    return nerf_amd_launch_composite(a.raw, a.ts_out, a.rays + 3, 6, out.rgb, out.disp, out.alpha, out.acc, out.w, B, a.N, 1,
                                     out.pixels, s);
}
}  // namespace

extern "C" {

int nerf_amd_abi_version(void) { return NERF_AMD_ABI_VERSION; }
int64_t nerf_amd_param_count(void) { return PARAM_COUNT; }

int64_t nerf_amd_packed_bytes(int precision) {
    if (bad_image(precision)) return NERF_AMD_EINVAL;
    if (precision == NERF_AMD_BF16_BWD) return BWD_IMAGE_BYTES;
    return precision == NERF_AMD_F32 ? F32_PACKED_BYTES : B16_IMAGE_BYTES;
}

int64_t nerf_amd_packed_status_offset(int precision) {
    if (bad_image(precision)) return NERF_AMD_EINVAL;
    return (precision == NERF_AMD_BF16 || precision == NERF_AMD_FP16) ? B16_STATUS_OFF : -1;
}

int nerf_amd_grad_bucket_range(int bucket, int64_t* first, int64_t* count) {
    if (!first || !count || bucket < 0 || bucket > 2) return NERF_AMD_EINVAL;
    *first = bucket == 1 ? GRAD_BUCKET_SPLIT : 0;
    *count = bucket == 0 ? PARAM_COUNT : bucket == 1 ? PARAM_COUNT - GRAD_BUCKET_SPLIT : GRAD_BUCKET_SPLIT;
    return 0;
}

int64_t nerf_amd_render_image_workspace_bytes(int precision, int64_t n_rays, int N) {
    if (n_rays < 0 || N <= 0 || bad_precision(precision)) return NERF_AMD_EINVAL;
    return image_ws(precision, n_rays, N).bytes;
}

int64_t nerf_amd_render_workspace_bytes(int precision, int64_t B, int N) {
    if (B < 0 || N <= 0 || bad_precision(precision)) return NERF_AMD_EINVAL;
    return render_ws(precision, B, N).bytes;
}

int nerf_amd_layout_src_col(int precision, int layer, int kstep, int half, int elem) {
    if (layer < 0 || layer >= NUM_LAYERS) return -2;
    if (precision == NERF_AMD_BF16 || precision == NERF_AMD_FP16) {
        if (kstep < 0 || kstep >= b16_ks(layer) || half < 0 || half > 3 || elem < 0 || elem > 7) return -2;
        return src_col_b16(layer, kstep, half, elem);
    }
    if (precision == NERF_AMD_F32) {
        if (kstep < 0 || kstep >= f32_ks(layer) || half < 0 || half > 3) return -2;
        return src_col_f32(layer, kstep, half);
    }
    return -2;
}

// Every source column of every layer must be hit exactly once by the packed
// k positions (the permutations are bijections onto the true K, padding aside).
int nerf_amd_layout_selfcheck(void) {
    static_assert(F32_NUM_CHUNKS == 154, "f32 chunk count");
    static_assert(B16_WEIGHT_KIB == 1172 && B16_BIAS_FLOATS == F32_BIAS_FLOATS, "16-row 16-bit image");
    for (int L = 0; L < NUM_LAYERS; ++L) {
        const LayerDesc d = layer_desc(L);
        for (int prec = 0; prec < 2; ++prec) {          // 0: f32 k order, 1: 16-bit k order
            int seen[320] = {0}, pads = 0;
            if (prec == 1) {
                for (int s = 0; s < b16_ks(L); ++s)
                    for (int g = 0; g < 4; ++g)
                        for (int j = 0; j < 8; ++j) {
                            const int c = src_col_b16(L, s, g, j);
                            if (c < 0) { ++pads; continue; }
                            if (c >= d.ld) return 100 + L;
                            ++seen[c];
                        }
            } else {
                for (int s = 0; s < f32_ks(L); ++s)
                    for (int g = 0; g < 4; ++g) {
                        const int c = src_col_f32(L, s, g);
                        if (c < 0) { ++pads; continue; }
                        if (c >= d.ld) return 200 + L;
                        ++seen[c];
                    }
            }
            for (int i = 0; i < d.ld; ++i)
                if (seen[i] != 1) return 300 + 20 * prec + L;
            if (pads != layer_k(L) - d.ld) return 400 + 20 * prec + L;
        }
    }
    return 0;
}

int nerf_amd_pack_weights(const float* params, void* packed, int precision, void* stream) {
    if (!params || !packed || bad_image(precision)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_pack(params, packed, precision, S(stream));
}

int nerf_amd_pack_weights_train(const float* params, void* packed_bf16, void* packed_bwd, void* stream) {
    if (!params || !packed_bf16 || !packed_bwd) return NERF_AMD_EINVAL;
    return nerf_amd_launch_pack_train(params, packed_bf16, packed_bwd, S(stream));
}

int nerf_amd_gamma(const float* x, int64_t x_stride, float* out, int64_t n, int L, void* stream) {
    if (n < 0 || L < 0 || x_stride < 0) return NERF_AMD_EINVAL;
    if (n == 0 || L == 0) return 0;
    if (!x || !out) return NERF_AMD_EINVAL;
    return nerf_amd_launch_gamma(x, x_stride, out, n, L, S(stream));
}

int nerf_amd_positional_encoder(const float* vec, float* posx, float* posd, int64_t P, int Lp, int Ld,
                                void* stream) {
    if (P < 0 || Lp < 0 || Ld < 0) return NERF_AMD_EINVAL;
    if (P == 0) return 0;
    if (!vec || !posx || !posd) return NERF_AMD_EINVAL;
    return nerf_amd_launch_posenc(vec, posx, posd, P, Lp, Ld, S(stream));
}

int nerf_amd_gamma_backward(const float* x, int64_t x_stride, const float* d_out, float* d_x, int64_t n, int L, void* stream) {
    if (n < 0 || L < 0 || x_stride < 0) return NERF_AMD_EINVAL;
    if (n == 0) return 0;
    if (!x || !d_out || !d_x) return NERF_AMD_EINVAL;
    return nerf_amd_launch_gamma_backward(x, x_stride, d_out, d_x, n, L, S(stream));
}

int nerf_amd_positional_encoder_backward(const float* vec, const float* d_posx, const float* d_posd, float* d_vec,
                                         int64_t P, int Lp, int Ld, void* stream) {
    if (P < 0 || Lp < 0 || Ld < 0) return NERF_AMD_EINVAL;
    if (P == 0) return 0;
    if (!vec || !d_posx || !d_posd || !d_vec) return NERF_AMD_EINVAL;
    return nerf_amd_launch_posenc_backward(vec, d_posx, d_posd, d_vec, P, Lp, Ld, S(stream));
}

int nerf_amd_query_points_backward(const float* rays, const float* ts, const float* d_q, float* d_rays, int64_t B, int N,
                                   void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!rays || !ts || !d_q || !d_rays) return NERF_AMD_EINVAL;
    return nerf_amd_launch_query_points_backward(rays, ts, d_q, d_rays, B, N, S(stream));
}

int nerf_amd_input_gradients(const void* dys, const float* params, const float* pts, const float* rays, const float* ts,
                             float* dv, float* d_rays, int64_t P, int N, void* stream) {
    if (P < 0) return NERF_AMD_EINVAL;
    const bool rays_mode = pts == nullptr;
    if (rays_mode && (N <= 0 || P % N != 0)) return NERF_AMD_EINVAL;
    if (P == 0) return 0;
    if (!dys || !params || !dv) return NERF_AMD_EINVAL;
    if (rays_mode ? (!rays || !ts || !d_rays) : (rays || ts || d_rays)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_input_gradients(dys, params, pts, rays, ts, dv, d_rays, P, rays_mode ? N : 1, S(stream));
}

int nerf_amd_query_points(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed,
                          int64_t ray_id0, float* query_pts, float* ts, int64_t B, int N, void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!rays || !query_pts) return NERF_AMD_EINVAL;
    if (bad_jitter(flags, u, tbins)) return NERF_AMD_EINVAL;
    MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    a.ts_out = ts;
    return nerf_amd_launch_query_points(&a, query_pts, S(stream));
}

int nerf_amd_range_check(const float* rays, const float* pts, const float* u, const float* tbins, uint32_t flags, uint64_t seed,
                         int64_t ray_id0, uint32_t* word, int64_t B, int N, void* stream) {
    if (B < 0 || !word || (rays && pts)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    MlpArgs a{};
    if (pts) {
        a.pts = pts; a.P = B;          // B floats
    } else {
        if (!rays || N <= 0) return NERF_AMD_EINVAL;
        if (bad_jitter(flags, u, tbins)) return NERF_AMD_EINVAL;
        a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    }
    return nerf_amd_launch_range_check(&a, B, word, S(stream));
}

int nerf_amd_mlp_forward(const float* pts, void* packed, float* out, int64_t P, int precision,
                         void* stream) {
    if (P < 0 || bad_precision(precision)) return NERF_AMD_EINVAL;
    if (P == 0) return 0;
    if (!pts || !packed || !out) return NERF_AMD_EINVAL;
    MlpArgs a{};
    a.pts = pts; a.packed = packed; a.raw = out; a.P = P; a.N = 1;
    return launch_mlp(a, 0, precision, S(stream));
}

int nerf_amd_volume_render(const float* raw, const float* ts, const float* dirs, int64_t dirs_stride,
                           float* rgb, float* disp, float* alpha, float* acc, float* w, int64_t B, int N,
                           void* stream) {
    if (B < 0 || N <= 0 || dirs_stride < 3) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!raw || !ts || !dirs || !rgb || !disp || !acc) return NERF_AMD_EINVAL;
    return nerf_amd_launch_composite(raw, ts, dirs, dirs_stride, rgb, disp, alpha, acc, w, B, N, 0, nullptr, S(stream));
}

int nerf_amd_volume_render_pixels(const float* raw, const float* ts, const float* rays, float* pixels,
                                  int64_t B, int N, void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!raw || !ts || !rays || !pixels) return NERF_AMD_EINVAL;
    return nerf_amd_launch_composite(raw, ts, rays + 3, 6, nullptr, nullptr, nullptr, nullptr, nullptr, B, N, 1,
                                     pixels, S(stream));
}

int nerf_amd_volume_render_rays(const float* raw, const float* ts, const float* rays, float* rgb, float* disp,
                                float* alpha, float* acc, float* w, int64_t B, int N, void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!raw || !ts || !rays || !rgb || !disp || !acc) return NERF_AMD_EINVAL;
    return nerf_amd_launch_composite(raw, ts, rays + 3, 6, rgb, disp, alpha, acc, w, B, N, 1, nullptr, S(stream));
}

int nerf_amd_volume_render_rays_backward(const float* raw, const float* ts, const float* rays, const float* g_rgb,
                                         const float* g_disp, const float* g_alpha, const float* g_acc,
                                         const float* g_w, float* d_raw, int64_t B, int N, void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (N > COMPOSITE_BWD_MAX_N) return NERF_AMD_EUNSUP;
    if (!raw || !ts || !rays || !d_raw) return NERF_AMD_EINVAL;
    return nerf_amd_launch_composite_backward(raw, ts, rays + 3, 6, g_rgb, g_disp, g_alpha, g_acc, g_w, d_raw, B, N, 1,
                                              S(stream));
}

int nerf_amd_volume_render_mse_backward(const float* raw, const float* ts, const float* rays, const float* target,
                                       float* rgb, float* d_raw, int64_t B, int N, void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (N > COMPOSITE_BWD_MAX_N) return NERF_AMD_EUNSUP;
    if (!raw || !ts || !rays || !target || !d_raw) return NERF_AMD_EINVAL;
    return nerf_amd_launch_composite_mse_backward(raw, ts, rays, target, rgb, d_raw, B, N, S(stream));
}

int nerf_amd_volume_render_mse_backward_pdf(const float* raw, const float* ts, const float* rays, const float* target,
                                            const float* u, uint32_t flags, uint64_t seed, int64_t ray_id0,
                                            float* rgb, float* d_raw, float* ts_out, int64_t B, int Nc, int Nf,
                                            void* stream) {
    if (B < 0 || Nc <= 0 || Nf < 0) return NERF_AMD_EINVAL;
    if (bad_pdf_jitter(flags, u, Nf)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (nerf_pdf::unsupported_sizes(Nc, Nf)) return NERF_AMD_EUNSUP;
    if (!raw || !ts || !rays || !target || !d_raw || !ts_out) return NERF_AMD_EINVAL;
    return nerf_amd_launch_composite_mse_backward_pdf(raw, ts, rays, target, rgb, d_raw, u, ts_out, B, Nc, Nf, seed, ray_id0,
                                                      (flags & NERF_AMD_DEVICE_RNG) ? 1 : 0,
                                                      (flags & NERF_AMD_SEED_IN_MEMORY) ? 1 : 0, S(stream));
}

// Order of the rules of the four entry points below: sizes; the noise arguments (api_checks.h bad_sigma_noise); the background's
// stride; the empty problem; the size limit (NERF_AMD_EUNSUP); the pointers.
int nerf_amd_sigma_noise(const float* raw, float* out, float std, uint32_t flags, uint64_t seed, const uint64_t* seed_mem,
                         int64_t ray_id0, int64_t B, int N, void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (bad_sigma_noise(std, flags, seed_mem)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!raw || !out) return NERF_AMD_EINVAL;
    return nerf_amd_launch_sigma_noise(raw, out, std, seed, noise_seed_mem(flags, seed_mem), ray_id0, B, N, S(stream));
}

int nerf_amd_background_blend(const float* rgb, const float* acc, const float* disp, const float* bg, int64_t bg_stride,
                              float* rgb_out, float* pixels, int64_t B, void* stream) {
    if (B < 0) return NERF_AMD_EINVAL;
    if (bad_bg_stride(bg_stride)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!rgb || !acc || !bg || (!rgb_out && !pixels) || (pixels && !disp)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_background_blend(rgb, acc, disp, bg, bg_stride, rgb_out, pixels, B, S(stream));
}

int nerf_amd_background_blend_backward(const float* g_rgb_bg, const float* bg, int64_t bg_stride, float* g_acc, int64_t B,
                                       void* stream) {
    if (B < 0) return NERF_AMD_EINVAL;
    if (bad_bg_stride(bg_stride)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!g_rgb_bg || !bg || !g_acc) return NERF_AMD_EINVAL;
    return nerf_amd_launch_background_blend_backward(g_rgb_bg, bg, bg_stride, g_acc, B, S(stream));
}

int nerf_amd_volume_render_mse_backward_bg(const float* raw, const float* ts, const float* rays, const float* target,
                                           const float* bg, int64_t bg_stride, float std, uint32_t flags, uint64_t seed,
                                           const uint64_t* seed_mem, int64_t ray_id0, float* rgb, float* d_raw, int64_t B, int N,
                                           void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (bad_sigma_noise(std, flags, seed_mem)) return NERF_AMD_EINVAL;
    if (bad_bg_stride(bg_stride)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (N > COMPOSITE_BWD_MAX_N) return NERF_AMD_EUNSUP;
    if (!raw || !ts || !rays || !target || !d_raw) return NERF_AMD_EINVAL;
    const DenseHeadArgs a{.raw = raw, .ts = ts, .rays = rays, .target = target, .rgb = rgb, .d_raw = d_raw, .B = B, .N = N,
                          .bg = bg, .bg_stride = bg_stride, .std = std, .seed = seed,
                          .seed_mem = noise_seed_mem(flags, seed_mem), .ray_id0 = ray_id0};
    return nerf_amd_launch_dense_head(&a, S(stream));          // bg == NULL and std == 0: the plain head's launch
}

// The coarse head of the pair behind a background and / or with noise on sigma (composite_head.hip).  Order of the rules: the
// plain coarse head's (sizes; the sampler's jitter arguments), then the noise arguments and the background's stride, then the
// plain head's again (the empty problem; the size limit, NERF_AMD_EUNSUP; the pointers).
int nerf_amd_volume_render_mse_backward_pdf_bg(const float* raw, const float* ts, const float* rays, const float* target,
                                               const float* bg, int64_t bg_stride, float std, uint32_t noise_flags,
                                               uint64_t noise_seed, const uint64_t* seed_mem, const float* u, uint32_t flags,
                                               uint64_t seed, int64_t ray_id0, float* rgb, float* d_raw, float* ts_out, int64_t B,
                                               int Nc, int Nf, void* stream) {
    if (B < 0 || Nc <= 0 || Nf < 0) return NERF_AMD_EINVAL;
    if (bad_pdf_jitter(flags, u, Nf)) return NERF_AMD_EINVAL;
    if (bad_sigma_noise(std, noise_flags, seed_mem)) return NERF_AMD_EINVAL;
    if (bad_bg_stride(bg_stride)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (nerf_pdf::unsupported_sizes(Nc, Nf)) return NERF_AMD_EUNSUP;
    if (!raw || !ts || !rays || !target || !d_raw || !ts_out) return NERF_AMD_EINVAL;
    const DenseHeadArgs a{.raw = raw, .ts = ts, .rays = rays, .target = target, .rgb = rgb, .d_raw = d_raw, .B = B, .N = Nc,
                          .bg = bg, .bg_stride = bg_stride, .std = std, .seed = noise_seed,
                          .seed_mem = noise_seed_mem(noise_flags, seed_mem), .ray_id0 = ray_id0};
    const DensePdfArgs p{u, ts_out, Nf, (flags & NERF_AMD_DEVICE_RNG) ? 1 : 0, (flags & NERF_AMD_SEED_IN_MEMORY) ? 1 : 0, seed};
    return nerf_amd_launch_dense_head_pdf(&a, &p, S(stream));  // bg == NULL and std == 0: the plain coarse head's launch
}

// The distortion term (composite_dist.hip).  Order of the rules: sizes; [the noise arguments; the background's stride;] the
// term's scalars (api_checks.h bad_distortion); the empty problem; the size limit (NERF_AMD_EUNSUP); the pointers.
int nerf_amd_distortion_loss(const float* ts, const float* w, float t_far, float coef, float* loss_ray, float* g_w, int64_t B,
                             int N, void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (bad_distortion(t_far, coef)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (N > COMPOSITE_BWD_MAX_N || B > MASKED_MAX_RAYS) return NERF_AMD_EUNSUP;
    if (!ts || !w || (!loss_ray && !g_w)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_distortion_loss(ts, w, t_far, coef, loss_ray, g_w, B, N, S(stream));
}

int nerf_amd_sum_f32(const float* x, float* out, int64_t n, void* stream) {
    if (n <= 0 || !x || !out) return NERF_AMD_EINVAL;
    return nerf_amd_launch_sum_f32(x, out, n, S(stream));
}

int nerf_amd_volume_render_mse_backward_dist(const float* raw, const float* ts, const float* rays, const float* target,
                                             const float* bg, int64_t bg_stride, float std, uint32_t flags, uint64_t seed,
                                             const uint64_t* seed_mem, int64_t ray_id0, float t_far, float coef, float* rgb,
                                             float* loss_ray, float* d_raw, int64_t B, int N, void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (bad_sigma_noise(std, flags, seed_mem)) return NERF_AMD_EINVAL;
    if (bad_bg_stride(bg_stride)) return NERF_AMD_EINVAL;
    if (bad_distortion(t_far, coef)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (N > COMPOSITE_BWD_MAX_N) return NERF_AMD_EUNSUP;
    if (!raw || !ts || !rays || !target || !d_raw) return NERF_AMD_EINVAL;
    const DenseHeadArgs a{.raw = raw, .ts = ts, .rays = rays, .target = target, .rgb = rgb, .d_raw = d_raw, .B = B, .N = N,
                          .bg = bg, .bg_stride = bg_stride, .std = std, .seed = seed,
                          .seed_mem = noise_seed_mem(flags, seed_mem), .ray_id0 = ray_id0, .dist = true, .t_far = t_far,
                          .coef = coef, .loss_ray = loss_ray};
    return nerf_amd_launch_dense_head(&a, S(stream));
}

int nerf_amd_mse_loss(const float* pred, const float* target, float* loss, float* g_pred, int64_t n, void* stream) {
    if (n <= 0 || !pred || !target || !loss) return NERF_AMD_EINVAL;
    return nerf_amd_launch_mse_loss(pred, target, loss, g_pred, n, S(stream));
}

int nerf_amd_volume_render_backward(const float* raw, const float* ts, const float* dirs, int64_t dirs_stride,
                                    const float* g_rgb, const float* g_disp, const float* g_alpha,
                                    const float* g_acc, const float* g_w, float* d_raw, int64_t B, int N,
                                    void* stream) {
    if (B < 0 || N <= 0 || dirs_stride < 3) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (N > COMPOSITE_BWD_MAX_N) return NERF_AMD_EUNSUP;
    if (!raw || !ts || !dirs || !d_raw) return NERF_AMD_EINVAL;
    return nerf_amd_launch_composite_backward(raw, ts, dirs, dirs_stride, g_rgb, g_disp, g_alpha, g_acc, g_w,
                                              d_raw, B, N, 0, S(stream));
}

int nerf_amd_sample_encode(const float* rays, const float* u, const float* tbins, uint32_t flags,
                           uint64_t seed, int64_t ray_id0, float* posx, float* posd, float* ts, int64_t B,
                           int N, void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!rays || !posx || !posd) return NERF_AMD_EINVAL;
    if (bad_jitter(flags, u, tbins)) return NERF_AMD_EINVAL;
    MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    a.ts_out = ts;
    return nerf_amd_launch_sample_encode(&a, posx, posd, S(stream));
}

int nerf_amd_mlp_forward_rays(const float* rays, const float* u, const float* tbins, void* packed,
                              int precision, uint32_t flags, uint64_t seed, int64_t ray_id0, float* raw,
                              float* ts, int64_t B, int N, void* stream) {
    if (B < 0 || N <= 0 || bad_precision(precision)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!rays || !packed || !raw) return NERF_AMD_EINVAL;
    if (bad_jitter(flags, u, tbins)) return NERF_AMD_EINVAL;
    MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    a.packed = packed; a.raw = raw; a.ts_out = ts;
    return launch_mlp(a, 1, precision, S(stream));
}

int nerf_amd_render_forward(const float* rays, const float* u, const float* tbins, void* packed,
                            int precision, uint32_t flags, uint64_t seed, int64_t ray_id0, float* rgb,
                            float* disp, float* alpha, float* acc, float* w, void* workspace, int64_t B,
                            int N, void* stream) {
    if (B < 0 || N <= 0 || bad_precision(precision)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!rgb || !disp || !acc) return NERF_AMD_EINVAL;
    MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    a.packed = packed;
    return render_rays(a, RenderOut{rgb, disp, alpha, acc, w, nullptr}, precision, workspace, S(stream));
}

int nerf_amd_render_pixels_forward(const float* rays, const float* u, const float* tbins, void* packed,
                                   int precision, uint32_t flags, uint64_t seed, int64_t ray_id0, float* pixels,
                                   void* workspace, int64_t B, int N, void* stream) {
    if (B < 0 || N <= 0 || bad_precision(precision)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!pixels) return NERF_AMD_EINVAL;
    MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    a.packed = packed;
    return render_rays(a, RenderOut{nullptr, nullptr, nullptr, nullptr, nullptr, pixels}, precision, workspace, S(stream));
}

int nerf_amd_generate_rays(const float* h_pose, int H, int W, float f, int64_t ray0, int64_t n_rays,
                           float* rays, void* stream) {
    if (!h_pose || H <= 0 || W <= 0 || !(f > 0.f) || ray0 < 0 || n_rays < 0 ||
        ray0 + n_rays > (int64_t)H * W) return NERF_AMD_EINVAL;
    if (n_rays == 0) return 0;
    if (!rays) return NERF_AMD_EINVAL;
    return nerf_amd_launch_generate_rays(h_pose, H, W, f, ray0, n_rays, rays, S(stream));
}

int nerf_amd_render_image_forward(const float* h_pose, int H, int W, float f, int64_t ray0, int64_t n_rays,
                                  const float* u, const float* tbins, void* packed, int precision,
                                  uint32_t flags, uint64_t seed, float* pixels, void* workspace, int N,
                                  void* stream) {
    if (n_rays < 0 || N <= 0 || bad_precision(precision)) return NERF_AMD_EINVAL;
    if (n_rays == 0) return 0;
    if (!workspace || !pixels || !packed) return NERF_AMD_EINVAL;
    if (bad_jitter(flags, u, tbins)) return NERF_AMD_EINVAL;      // before the rays are generated: nothing is launched
    char* ws = reinterpret_cast<char*>(workspace);
    float* rays = reinterpret_cast<float*>(ws);
    const int rc = nerf_amd_generate_rays(h_pose, H, W, f, ray0, n_rays, rays, stream);
    if (rc) return rc;
    // jitter is keyed by the GLOBAL pixel id, so the image does not depend on how it is sharded
    return nerf_amd_render_pixels_forward(rays, u, tbins, packed, precision, flags, seed, ray0, pixels,
                                          ws + image_ws(precision, n_rays, N).off_render, n_rays, N, stream);
}

int nerf_amd_sample_pdf(const float* ts, const float* w, const float* u, uint32_t flags, uint64_t seed,
                        int64_t ray_id0, float* ts_out, int64_t B, int Nc, int Nf, void* stream) {
    if (B < 0 || Nc <= 0 || Nf < 0) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (nerf_pdf::unsupported_sizes(Nc, Nf)) return NERF_AMD_EUNSUP;
    if (!ts || !w || !ts_out) return NERF_AMD_EINVAL;
    if (flags & ~NERF_AMD_DEVICE_RNG) return NERF_AMD_EINVAL;
    if (!(flags & NERF_AMD_DEVICE_RNG) && !u && Nf > 0) return NERF_AMD_EINVAL;
    return nerf_amd_launch_sample_pdf(ts, w, u, ts_out, B, Nc, Nf, seed, ray_id0,
                                      (flags & NERF_AMD_DEVICE_RNG) ? 1 : 0, S(stream));
}

int64_t nerf_amd_render_hierarchical_workspace_bytes(int64_t n_rays, int Nc, int Nf) {
    if (n_rays < 0 || Nc <= 0 || Nf < 0) return NERF_AMD_EINVAL;
    return hier_ws(n_rays, Nc, Nf).bytes;
}

int nerf_amd_render_hierarchical_forward(const float* h_pose, int H, int W, float f, int64_t ray0, int64_t n_rays,
                                         const float* u_c, const float* u_f, const float* tbins_c,
                                         void* packed_c, void* packed_f, int precision, uint32_t flags,
                                         uint64_t seed, float* pixels, void* workspace, int Nc, int Nf, void* stream) {
    if (n_rays < 0 || Nc <= 0 || Nf < 0 || bad_precision(precision)) return NERF_AMD_EINVAL;
    if (n_rays == 0) return 0;
    if (nerf_pdf::unsupported_sizes(Nc, Nf) || !fused_render(precision, Nc + Nf)) return NERF_AMD_EUNSUP;
    if (!workspace || !pixels || !packed_c || !packed_f || !tbins_c) return NERF_AMD_EINVAL;
    // explicit jitter for both passes, or the counter RNG with its seed in the argument: the seed-in-memory form would
    // need u_c to be that address, which this entry point does not offer (the coarse kernel would dereference it)
    if (flags & ~NERF_AMD_DEVICE_RNG) return NERF_AMD_EINVAL;
    if (!(flags & NERF_AMD_DEVICE_RNG) && (!u_c || (!u_f && Nf > 0))) return NERF_AMD_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    const HierWs l = hier_ws(n_rays, Nc, Nf);
    float* rays = reinterpret_cast<float*>(ws);
    float* ts_c = reinterpret_cast<float*>(ws + l.off_ts_c);
    float* w_c = reinterpret_cast<float*>(ws + l.off_w_c);
    float* ts_f = reinterpret_cast<float*>(ws + l.off_ts_f);
    int rc = nerf_amd_generate_rays(h_pose, H, W, f, ray0, n_rays, rays, stream);
    if (rc) return rc;
    // coarse pass: one fused launch that leaves only what the sampler needs (positions and weights)
    MlpArgs a = rays_args(rays, u_c, tbins_c, flags, seed, ray0, n_rays, Nc);
    a.packed = packed_c; a.ts_out = ts_c; a.w = w_c;
    rc = launch_mlp(a, 1, precision, S(stream));
    if (rc) return rc;
    rc = nerf_amd_launch_sample_pdf(ts_c, w_c, u_f, ts_f, n_rays, Nc, Nf, seed, ray0,
                                    (flags & NERF_AMD_DEVICE_RNG) ? 1 : 0, S(stream));
    if (rc) return rc;
    // fine pass on the merged, sorted positions -> clipped pixels
    return nerf_amd_render_pixels_forward(rays, ts_f, nullptr, packed_f, precision, NERF_AMD_TS_GIVEN, seed, ray0, pixels,
                                          nullptr, n_rays, Nc + Nf, stream);
}

int64_t nerf_amd_train_activation_bytes(int64_t P) {
    return P < 0 ? (int64_t)NERF_AMD_EINVAL : (int64_t)acts_total_bytes(P);
}

int nerf_amd_mlp_forward_train(const float* rays, const float* u, const float* tbins, void* packed,
                               uint32_t flags, uint64_t seed, int64_t ray_id0, float* raw, float* ts,
                               void* acts, int64_t B, int N, void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!rays || !packed || !raw || !acts) return NERF_AMD_EINVAL;
    if (bad_jitter(flags & ~NERF_AMD_STORE_E4M3, u, tbins)) return NERF_AMD_EINVAL;
    static_assert(NERF_AMD_STORE_E4M3 == NERF_FLAG_STORE_E4M3, "the flag travels to the kernel as it is");
    MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    a.packed = packed; a.raw = raw; a.ts_out = ts; a.acts = acts;
    return nerf_amd_launch_mlp_bf16_16(&a, 1, S(stream));
}

int nerf_amd_mlp_forward_train_points(const float* pts, void* packed, float* out, void* acts, int64_t P,
                                      void* stream) {
    if (P < 0) return NERF_AMD_EINVAL;
    if (P == 0) return 0;
    if (!pts || !packed || !out || !acts) return NERF_AMD_EINVAL;
    MlpArgs a{};
    a.pts = pts; a.packed = packed; a.raw = out; a.acts = acts; a.P = P; a.N = 1;
    return nerf_amd_launch_mlp_bf16_16(&a, 1, S(stream));
}

int nerf_amd_encode_points_bf16(const float* pts, void* posx64, void* posd32, int64_t P, void* stream) {
    if (P < 0) return NERF_AMD_EINVAL;
    if (P == 0) return 0;
    if (!pts || !posx64 || !posd32) return NERF_AMD_EINVAL;
    MlpArgs a{};
    a.pts = pts; a.P = P; a.N = 1;
    return nerf_amd_launch_sample_encode_bf16(&a, posx64, posd32, S(stream));
}

int nerf_amd_mlp_backward(const float* d_raw, const void* bwd_image, const void* acts, void* dys, int64_t P,
                          void* stream) {
    if (P < 0) return NERF_AMD_EINVAL;
    if (P == 0) return 0;
    if (!d_raw || !bwd_image || !acts || !dys) return NERF_AMD_EINVAL;
    return nerf_amd_launch_mlp_backward(d_raw, bwd_image, acts, dys, P, 0, S(stream));
}

int64_t nerf_amd_train_activation_bytes_e4m3(int64_t P) {
    return P < 0 ? (int64_t)NERF_AMD_EINVAL : (int64_t)f8_acts_total_bytes(P);
}
int64_t nerf_amd_train_gradient_bytes_e4m3(int64_t P) {
    return P < 0 ? (int64_t)NERF_AMD_EINVAL : (int64_t)f8_data_bytes(P);
}
int64_t nerf_amd_param_gradients_scratch_e4m3_bytes(int64_t P) {
    return P < 0 ? (int64_t)NERF_AMD_EINVAL : (int64_t)nerf_amd_f8_scratch_bytes(P);
}
int nerf_amd_mlp_backward_e4m3(const float* d_raw, const void* bwd_image, const void* acts, void* dys, int64_t P,
                               void* stream) {
    if (P < 0) return NERF_AMD_EINVAL;
    if (P == 0) return 0;
    if (!d_raw || !bwd_image || !acts || !dys) return NERF_AMD_EINVAL;
    return nerf_amd_launch_mlp_backward(d_raw, bwd_image, acts, dys, P, 1, S(stream));
}
int nerf_amd_param_gradients_convert_e4m3(const void* posx64, const void* posd32, const void* scratch, void* scratch_e4m3,
                                          int64_t P, int which, void* stream) {
    if (P < 0 || which < 1 || which > 3) return NERF_AMD_EINVAL;
    if (P == 0) return 0;
    if (!scratch_e4m3 || ((which & 1) && (!posx64 || !posd32)) || ((which & 2) && !scratch)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_param_gradients_convert_e4m3(posx64, posd32, scratch, scratch_e4m3, P, which, S(stream));
}
int nerf_amd_param_gradients_finish_e4m3(const void* acts, const void* dys, const void* scratch_e4m3, float* grads, int64_t P,
                                         int bucket, void* stream) {
    if (P < 0 || !grads || bucket < 0 || bucket > 2) return NERF_AMD_EINVAL;
    if (P > 0 && (!acts || !dys || !scratch_e4m3)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_param_gradients_finish_e4m3(acts, dys, scratch_e4m3, grads, P, bucket, S(stream));
}

int nerf_amd_sample_encode_bf16(const float* rays, const float* u, const float* tbins, uint32_t flags,
                                uint64_t seed, int64_t ray_id0, void* posx64, void* posd32, float* ts, int64_t B,
                                int N, void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!rays || !posx64 || !posd32) return NERF_AMD_EINVAL;
    if (bad_jitter(flags, u, tbins)) return NERF_AMD_EINVAL;
    MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    a.ts_out = ts;
    return nerf_amd_launch_sample_encode_bf16(&a, posx64, posd32, S(stream));
}

int64_t nerf_amd_param_gradients_scratch_bytes(int64_t P) { return P < 0 ? (int64_t)NERF_AMD_EINVAL : P * 64; }

int nerf_amd_param_gradients(const float* d_raw, const void* acts, const void* dys, const void* posx64,
                             const void* posd32, void* scratch, float* grads, int64_t P, void* stream) {
    if (P < 0 || !grads) return NERF_AMD_EINVAL;
    if (P > 0 && (!d_raw || !acts || !dys || !posx64 || !posd32 || !scratch)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_param_gradients(d_raw, acts, dys, posx64, posd32, scratch, grads, P, S(stream));
}

int nerf_amd_param_gradients_begin(const float* d_raw, void* scratch, float* grads, int64_t P, void* stream) {
    if (P < 0 || !grads) return NERF_AMD_EINVAL;
    if (P > 0 && (!d_raw || !scratch)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_param_gradients_begin(d_raw, scratch, grads, P, S(stream));
}

int nerf_amd_param_gradients_finish(const void* acts, const void* dys, const void* posx64, const void* posd32,
                                    const void* scratch, float* grads, int64_t P, void* stream) {
    return nerf_amd_param_gradients_finish_bucket(acts, dys, posx64, posd32, scratch, grads, P, 0, stream);
}

int nerf_amd_param_gradients_finish_bucket(const void* acts, const void* dys, const void* posx64, const void* posd32,
                                           const void* scratch, float* grads, int64_t P, int bucket, void* stream) {
    if (P < 0 || !grads || bucket < 0 || bucket > 2) return NERF_AMD_EINVAL;
    if (P > 0 && (!acts || !dys || !posx64 || !posd32 || !scratch)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_param_gradients_finish(acts, dys, posx64, posd32, scratch, grads, P, bucket, S(stream));
}

int nerf_amd_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                       float lr, float beta1, float beta2, float eps, int64_t step, void* stream) {
    if (n < 0 || step < 1) return NERF_AMD_EINVAL;
    if (n == 0) return 0;
    if (!params || !grads || !exp_avg || !exp_avg_sq) return NERF_AMD_EINVAL;
    // bias corrections in double on the host, as torch does for a python-number step
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    return nerf_amd_launch_adam(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, (float)bc1,
                                (float)sqrt(bc2), S(stream));
}

int nerf_amd_mt19937_uniform(const uint32_t* state624, int next, float* out, int64_t n, uint32_t* state_out624,
                             void* stream) {
    if (n < 0 || next < 0 || next > 624) return NERF_AMD_EINVAL;
    if (!state624 || !state_out624 || (n > 0 && !out)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_mt19937_uniform(state624, next, out, n, state_out624, S(stream));
}

int64_t nerf_amd_mt19937_segments(int next, int64_t n, int64_t seg_words) {
    if (n < 0 || next < 0 || next > 624 || seg_words <= 0 || seg_words % 624) return NERF_AMD_EINVAL;
    const int64_t avail = 624 - next;
    return n > avail + seg_words ? 1 + (n - avail - seg_words + seg_words - 1) / seg_words : 1;
}

int nerf_amd_mt19937_uniform_par(const uint32_t* state624, int next, float* out, int64_t n, uint32_t* state_out624,
                                 const uint32_t* polys, int levels, int64_t seg_words, uint32_t* seg_states,
                                 void* stream) {
    if (n < 0 || next < 0 || next > 624 || levels < -4096 || levels > 30) return NERF_AMD_EINVAL;
    if (seg_words <= 0 || seg_words % 624) return NERF_AMD_EINVAL;
    if (!state624 || !state_out624 || (n > 0 && !out)) return NERF_AMD_EINVAL;
    const int64_t nseg = nerf_amd_mt19937_segments(next, n, seg_words);
    if (nseg > 1 && (!polys || !seg_states)) return NERF_AMD_EINVAL;
    if (levels >= 0 ? nseg > ((int64_t)1 << levels) : nseg > 1 - (int64_t)levels) return NERF_AMD_EUNSUP;
    return nerf_amd_launch_mt19937_uniform_par(state624, next, out, n, state_out624, polys, levels, seg_words, seg_states,
                                               S(stream));
}

int nerf_amd_mt19937_raw(const uint32_t* state624, int next, uint32_t* out, int64_t n, uint32_t* state_out624, void* stream) {
    if (n < 0 || next < 0 || next > 624) return NERF_AMD_EINVAL;
    if (!state624 || (n > 0 && !out)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_mt19937_raw(state624, next, out, n, state_out624, S(stream));
}

int nerf_amd_mt19937_jump_poly(int64_t blocks, const uint32_t* h_phi624, uint32_t* h_poly624) {
    if (blocks < 0 || blocks > ((int64_t)1 << 52) || !h_phi624 || !h_poly624) return NERF_AMD_EINVAL;
    return nerf_amd_host_mt19937_jump_poly(blocks, h_phi624, h_poly624) == 0 ? 0 : NERF_AMD_EINVAL;
}

int nerf_amd_mt19937_advance(const uint32_t* state624, const uint32_t* poly624, uint32_t* state_out624, void* stream) {
    if (!state624 || !poly624 || !state_out624 || state624 == state_out624) return NERF_AMD_EINVAL;
    return nerf_amd_launch_mt19937_advance(state624, poly624, state_out624, S(stream));
}

int nerf_amd_mt19937_uniform_after(const uint32_t* state624, const uint32_t* polys, int segments, int next_after, float* out,
                                   int64_t n, uint32_t* state_out624, int64_t seg_words, uint32_t* seg_states, void* stream) {
    if (n <= 0 || segments < 1 || segments > 4096 || next_after < 0 || next_after > 624) return NERF_AMD_EINVAL;
    if (seg_words <= 0 || seg_words % 624) return NERF_AMD_EINVAL;
    if (!state624 || !polys || !out || !state_out624 || !seg_states) return NERF_AMD_EINVAL;
    if (nerf_amd_mt19937_segments(next_after, n, seg_words) != segments) return NERF_AMD_EINVAL;
    return nerf_amd_launch_mt19937_uniform_after(state624, polys, segments, next_after, out, n, state_out624, seg_words, seg_states,
                                                 S(stream));
}

int64_t nerf_amd_select_workspace_bytes(int64_t B) { return B < 0 ? NERF_AMD_EINVAL : align256(B * 12 + 16); }

int nerf_amd_select_rays(const uint32_t* draws, uint64_t seed, const uint64_t* seed_mem, int64_t n, int64_t B,
                         const float* table, const float* colours, float* rays_out, float* gt_out, int64_t* ids_out,
                         void* workspace, void* stream) {
    if (n < 0 || B < 0 || B > n) return NERF_AMD_EINVAL;
    if (n >= (int64_t)(0xffffffffu / 20u)) return NERF_AMD_EUNSUP;      // torch.randperm switches algorithm there
    if (B == 0) return 0;
    if (!workspace || (rays_out && !table) || (gt_out && !colours)) return NERF_AMD_EINVAL;
    if (misaligned(table, 8) || misaligned(rays_out, 8) || misaligned(seed_mem, 8) || misaligned(workspace, 16)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_select_rays(draws, seed, reinterpret_cast<const unsigned long long*>(seed_mem), n, B, table, colours,
                                       rays_out, gt_out, reinterpret_cast<long long*>(ids_out), workspace, S(stream));
}

int nerf_amd_linear_f32(const float* A, int64_t sa_i, int64_t sa_k, const float* A_mask, const float* B, int64_t sb_k,
                        int64_t sb_j, const float* bias, float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, uint32_t flags,
                        void* stream) {
    if (M < 0 || N < 0 || K < 0 || (flags & ~3u)) return NERF_AMD_EINVAL;
    if (M == 0 || N == 0) return 0;
    if (!C || ldc < N || (K > 0 && (!A || !B))) return NERF_AMD_EINVAL;
    return nerf_amd_launch_linear_f32(A, sa_i, sa_k, A_mask, B, sb_k, sb_j, bias, C, ldc, M, N, K, (int)flags, S(stream));
}

int64_t nerf_amd_pinned_device_address(const void* host) {
    if (!host) return NERF_AMD_EINVAL;
    (void)hipGetLastError();
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<void*>(host), 0) != hipSuccess || !d) {
        (void)hipGetLastError();
        return NERF_AMD_EINVAL;                    // not pinned (or not mapped into the device's address space)
    }
    return (int64_t)reinterpret_cast<uintptr_t>(d);
}

int nerf_amd_hyper_fetch(const float* ring_dev, int slots, float* hyper, uint32_t* counter, void* stream) {
    if (!ring_dev || !hyper || !counter || slots <= 0) return NERF_AMD_EINVAL;
    return nerf_amd_launch_hyper_fetch(ring_dev, slots, hyper, counter, S(stream));
}

int nerf_amd_adam_step_hyper(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                             const float* hyper, void* stream) {
    if (n < 0) return NERF_AMD_EINVAL;
    if (n == 0) return 0;
    if (!params || !grads || !exp_avg || !exp_avg_sq || !hyper) return NERF_AMD_EINVAL;
    return nerf_amd_launch_adam_hyper(params, grads, exp_avg, exp_avg_sq, n, hyper, S(stream));
}

int64_t nerf_amd_grad_guard_workspace_bytes(int64_t n) { return n < 0 ? NERF_AMD_EINVAL : grad_guard_ws_bytes(); }

int nerf_amd_grad_guard(const float* grads, int64_t n, void* workspace, void* guard, void* stream) {
    if (n < 0) return NERF_AMD_EINVAL;
    if (bad_guard_record(guard) || !workspace || misaligned(workspace, 8)) return NERF_AMD_EINVAL;
    if (n > 0 && (!grads || misaligned(grads, 4))) return NERF_AMD_EINVAL;
    return nerf_amd_launch_grad_guard(grads, n, reinterpret_cast<double*>(workspace), reinterpret_cast<unsigned*>(guard), S(stream));
}

int nerf_amd_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                               const float* hyper, const void* guard, void* stream) {
    if (n < 0) return NERF_AMD_EINVAL;
    if (bad_guard_record(guard)) return NERF_AMD_EINVAL;          // looked at before the empty problem: a record is always needed
    if (n == 0) return 0;
    if (!params || !grads || !exp_avg || !exp_avg_sq || !hyper) return NERF_AMD_EINVAL;
    return nerf_amd_launch_adam_guarded(params, grads, exp_avg, exp_avg_sq, n, hyper, reinterpret_cast<const unsigned*>(guard),
                                        S(stream));
}

// ---- camera optimiser: rays from (stored pose, correction, pixel), their backward, the corrected poses ------------------
int nerf_amd_camera_rays(const float* poses, const float* xi, const int64_t* ids, int64_t* ids_copy, int H, int W, float f,
                         float* rays, int64_t B, int64_t M, void* stream) {
    if (bad_camera_sizes(B, M, H, W, f)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (unsupported_camera_sizes(B, M, H, W)) return NERF_AMD_EUNSUP;
    if (!ids || !rays || (M > 0 && !poses)) return NERF_AMD_EINVAL;
    if (misaligned(poses, 4) || misaligned(xi, 4) || misaligned(ids, 8) || misaligned(ids_copy, 8) || misaligned(rays, 8))
        return NERF_AMD_EINVAL;
    return nerf_amd_launch_camera_rays(poses, xi, reinterpret_cast<const long long*>(ids), reinterpret_cast<long long*>(ids_copy),
                                       H, W, f, rays, B, M, S(stream));
}

int64_t nerf_amd_camera_workspace_bytes(int64_t B, int64_t M) { return B < 0 || M < 0 ? NERF_AMD_EINVAL : 0; }

int nerf_amd_camera_rays_backward(const float* poses, const float* xi, const int64_t* ids, const float* d_rays, int H, int W,
                                  float f, float* g_xi, void* workspace, int64_t B, int64_t M, void* stream) {
    if (bad_camera_sizes(B, M, H, W, f)) return NERF_AMD_EINVAL;
    if (M == 0) return 0;                                    // no image: nothing to write (B == 0 still writes M zero rows)
    if (unsupported_camera_sizes(B, M, H, W)) return NERF_AMD_EUNSUP;
    if (!poses || !g_xi || (B > 0 && (!ids || !d_rays))) return NERF_AMD_EINVAL;
    if (misaligned(poses, 4) || misaligned(xi, 4) || misaligned(ids, 8) || misaligned(d_rays, 8) || misaligned(g_xi, 8))
        return NERF_AMD_EINVAL;
    (void)workspace;                                         // nerf_amd_camera_workspace_bytes is 0: not looked at
    return nerf_amd_launch_camera_rays_backward(poses, xi, reinterpret_cast<const long long*>(ids), d_rays, H, W, f, g_xi, B, M,
                                                S(stream));
}

int nerf_amd_camera_poses(const float* poses, const float* xi, float* out, int64_t M, void* stream) {
    if (M < 0) return NERF_AMD_EINVAL;
    if (M == 0) return 0;
    if (M > CAMERA_MAX) return NERF_AMD_EUNSUP;
    if (!poses || !out) return NERF_AMD_EINVAL;
    if (misaligned(poses, 4) || misaligned(xi, 4) || misaligned(out, 16)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_camera_poses(poses, xi, out, M, S(stream));
}

// ---- per-image colour correction (csrc/appearance.hip).  Order of the rules: sizes and the stride; the empty problem (B == 0:
// nothing is launched or looked at); the limits (NERF_AMD_EUNSUP); the pointers; their alignment (rows of six floats: 8 bytes).
int nerf_amd_appearance_gather(const float* theta, const int64_t* ids, int64_t* ids_copy, int64_t HW, float* theta_ray, int64_t B,
                               int64_t M, void* stream) {
    if (bad_appearance_sizes(B, M, HW)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (unsupported_appearance_sizes(B, M, HW)) return NERF_AMD_EUNSUP;
    if (!theta || !ids || !theta_ray) return NERF_AMD_EINVAL;
    if (misaligned(theta, 8) || misaligned(ids, 8) || misaligned(ids_copy, 8) || misaligned(theta_ray, 8)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_appearance_gather(theta, reinterpret_cast<const long long*>(ids), reinterpret_cast<long long*>(ids_copy),
                                             HW, theta_ray, B, M, S(stream));
}

int nerf_amd_appearance_apply(const float* rgb, const float* theta_ray, int64_t theta_stride, float* out, int64_t B, void* stream) {
    if (B < 0 || bad_theta_stride(theta_stride)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (B > CAMERA_MAX) return NERF_AMD_EUNSUP;
    if (!rgb || !theta_ray || !out) return NERF_AMD_EINVAL;
    if (misaligned(rgb, 4) || misaligned(theta_ray, 8) || misaligned(out, 4)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_appearance_apply(rgb, theta_ray, theta_stride, out, B, S(stream));
}

int nerf_amd_appearance_apply_backward(const float* g_out, const float* rgb, const float* theta_ray, int64_t theta_stride,
                                       float* g_rgb, float* g_theta_ray, int64_t B, void* stream) {
    if (B < 0 || bad_theta_stride(theta_stride)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (B > CAMERA_MAX) return NERF_AMD_EUNSUP;
    if (!g_out || !rgb || !theta_ray || !g_rgb || !g_theta_ray) return NERF_AMD_EINVAL;
    if (misaligned(g_out, 4) || misaligned(rgb, 4) || misaligned(theta_ray, 8) || misaligned(g_rgb, 4) || misaligned(g_theta_ray, 8))
        return NERF_AMD_EINVAL;
    return nerf_amd_launch_appearance_apply_backward(g_out, rgb, theta_ray, theta_stride, g_rgb, g_theta_ray, B, S(stream));
}

int nerf_amd_appearance_reduce(const float* g_theta_ray, const int64_t* ids, int64_t HW, const float* theta, float reg,
                               const int32_t* frozen, float* g_theta, int64_t B, int64_t M, void* stream) {
    if (bad_appearance_sizes(B, M, HW)) return NERF_AMD_EINVAL;
    if (!(reg >= 0.f) || reg > 3.402823466e38f) return NERF_AMD_EINVAL;        // negative, NaN, inf
    if (B == 0) return 0;
    if (unsupported_appearance_sizes(B, M, HW)) return NERF_AMD_EUNSUP;
    if (!g_theta_ray || !ids || !theta || !g_theta) return NERF_AMD_EINVAL;
    if (misaligned(g_theta_ray, 8) || misaligned(ids, 8) || misaligned(theta, 8) || misaligned(frozen, 4) || misaligned(g_theta, 8))
        return NERF_AMD_EINVAL;
    return nerf_amd_launch_appearance_reduce(g_theta_ray, reinterpret_cast<const long long*>(ids), HW, theta, reg, frozen, g_theta,
                                             B, M, S(stream));
}

int nerf_amd_volume_render_mse_backward_affine(const float* raw, const float* ts, const float* rays, const float* target,
                                               const float* theta_ray, int64_t theta_stride, float* rgb, float* g_theta_ray,
                                               float* d_raw, int64_t B, int N, void* stream) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (bad_theta_stride(theta_stride)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (N > COMPOSITE_BWD_MAX_N) return NERF_AMD_EUNSUP;
    if (!raw || !ts || !rays || !target || !theta_ray || !g_theta_ray || !d_raw) return NERF_AMD_EINVAL;
    if (misaligned(raw, 16) || misaligned(d_raw, 16) || misaligned(theta_ray, 8) || misaligned(g_theta_ray, 8)) return NERF_AMD_EINVAL;
    const DenseHeadArgs a{.raw = raw, .ts = ts, .rays = rays, .target = target, .rgb = rgb, .d_raw = d_raw, .B = B, .N = N,
                          .theta = theta_ray, .theta_stride = theta_stride, .g_theta = g_theta_ray};
    return nerf_amd_launch_dense_head(&a, S(stream));
}

// ---- image metrics: squared error, max(gt) and SSIM of M image pairs (csrc/image_metrics.hip) ---------------------------
int64_t nerf_amd_image_metrics_workspace_bytes(int64_t M, int H, int W) {
    if (bad_metrics_sizes(M, H, W, 3, 3)) return NERF_AMD_EINVAL;
    if (M == 0) return 0;
    if (unsupported_metrics_sizes(H, W)) return NERF_AMD_EUNSUP;
    return nerf_amd_image_metrics_ws_bytes(M, H, W);              // NERF_AMD_EUNSUP where the size leaves an int64
}

int nerf_amd_image_metrics(const float* pred, int64_t pred_stride, const float* gt, int64_t gt_stride, double* sums, double* ssim,
                           float* ssim_map, void* workspace, int64_t M, int H, int W, void* stream) {
    if (bad_metrics_sizes(M, H, W, pred_stride, gt_stride)) return NERF_AMD_EINVAL;
    if (M == 0) return 0;
    if (unsupported_metrics_sizes(H, W) || nerf_amd_image_metrics_ws_bytes(M, H, W) < 0) return NERF_AMD_EUNSUP;
    if ((ssim || ssim_map) && unsupported_ssim_sizes(H, W)) return NERF_AMD_EUNSUP;
    if (!pred || !gt || !sums || !workspace) return NERF_AMD_EINVAL;
    if (misaligned(pred, 4) || misaligned(gt, 4) || misaligned(ssim_map, 4) || misaligned(sums, 8) || misaligned(ssim, 8) ||
        misaligned(workspace, 8))
        return NERF_AMD_EINVAL;
    return nerf_amd_launch_image_metrics(pred, pred_stride, gt, gt_stride, sums, ssim, ssim_map, workspace, M, H, W, S(stream));
}

// ---- density grid and marching cubes (not in the reference) ----------------------------------------------------------
int nerf_amd_density_forward(const float* pts, int64_t stride, void* packed, int precision, float* sigma, int64_t P,
                             void* stream) {
    if (P < 0 || stride < 3 || bad_precision(precision)) return NERF_AMD_EINVAL;
    if (precision == NERF_AMD_F32) return NERF_AMD_EUNSUP;
    if (P == 0) return 0;
    if (!pts || !packed || !sigma) return NERF_AMD_EINVAL;
    DensityArgs a{};
    a.pts = pts; a.stride = stride; a.packed = packed; a.sigma = sigma; a.P = P;
    return launch_density(a, precision, S(stream));
}

int nerf_amd_density_grid(const float* h_lo, const float* h_step, int64_t nx, int64_t ny, int64_t nz, void* packed, int precision,
                          float* sigma, void* stream) {
    if (bad_grid(nx, ny, nz) || bad_precision(precision) || !h_lo || !h_step) return NERF_AMD_EINVAL;
    if (precision == NERF_AMD_F32) return NERF_AMD_EUNSUP;
    if (!packed || !sigma) return NERF_AMD_EINVAL;
    DensityArgs a = grid_args(h_lo, h_step, nx, ny, nz);
    a.packed = packed; a.sigma = sigma;
    return launch_density(a, precision, S(stream));
}

int nerf_amd_grid_points(const float* h_lo, const float* h_step, int64_t nx, int64_t ny, int64_t nz, int64_t first, int64_t count,
                         float* pts6, void* stream) {
    if (bad_grid(nx, ny, nz) || !h_lo || !h_step || first < 0 || count < 0 || first > nx * ny * nz - count) return NERF_AMD_EINVAL;
    if (count == 0) return 0;
    if (!pts6) return NERF_AMD_EINVAL;
    const DensityArgs a = grid_args(h_lo, h_step, nx, ny, nz);
    return nerf_amd_launch_grid_points(&a, first, count, pts6, S(stream));
}

int64_t nerf_amd_marching_cubes_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) {
    if (bad_grid(nx, ny, nz)) return NERF_AMD_EINVAL;
    return nerf_amd_mc_workspace_bytes(nx * ny * nz);
}

int nerf_amd_marching_cubes_count(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float level, void* workspace,
                                  int64_t* counts, void* stream) {
    if (bad_grid(nx, ny, nz) || !sigma || !workspace || !counts) return NERF_AMD_EINVAL;
    if (misaligned(workspace, 16) || misaligned(counts, 8)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_mc_count(sigma, nx, ny, nz, level, workspace, reinterpret_cast<long long*>(counts), S(stream));
}

int nerf_amd_marching_cubes_emit(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float level, const float* h_lo,
                                 const float* h_step, void* workspace, float* verts, float* normals, int32_t* faces,
                                 int64_t max_verts, int64_t max_faces, void* stream) {
    if (bad_grid(nx, ny, nz) || !sigma || !workspace || !h_lo || !h_step) return NERF_AMD_EINVAL;
    if (max_verts < 0 || max_faces < 0 || max_verts > INT32_MAX) return NERF_AMD_EINVAL;      // vertex numbers are int32
    if ((max_verts > 0 && !verts) || (max_faces > 0 && !faces) || misaligned(workspace, 16)) return NERF_AMD_EINVAL;
    return nerf_amd_launch_mc_emit(sigma, nx, ny, nz, level, h_lo, h_step, workspace, verts, normals, faces, max_verts, max_faces,
                                   S(stream));
}

// ---- occupancy grid and the masked render (not in the reference) -------------------------------------------------------
int64_t nerf_amd_occupancy_grid_words(int64_t nx, int64_t ny, int64_t nz) {
    if (bad_grid(nx, ny, nz)) return NERF_AMD_EINVAL;
    return (nx - 1) * (ny - 1) * ((nz - 1 + 31) / 32);
}

int nerf_amd_occupancy_from_density(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float level, int dilate,
                                    uint32_t* bits, void* stream) {
    if (bad_grid(nx, ny, nz) || dilate < 0 || !sigma || !bits) return NERF_AMD_EINVAL;
    if (dilate > nerf_amd_occ_max_dilate()) return NERF_AMD_EUNSUP;
    return nerf_amd_launch_occ_bits(sigma, nx, ny, nz, level, dilate, bits, S(stream));
}

int nerf_amd_occupancy_from_mask(const uint8_t* cells, int64_t nx, int64_t ny, int64_t nz, uint32_t* bits, void* stream) {
    if (bad_grid(nx, ny, nz) || !cells || !bits) return NERF_AMD_EINVAL;
    return nerf_amd_launch_occ_pack(cells, nx - 1, ny - 1, nz - 1, bits, S(stream));
}

int64_t nerf_amd_occupancy_mask_words(int64_t B, int N) {
    if (B < 0 || N <= 0) return NERF_AMD_EINVAL;
    if (N > MASKED_MAX_N || B > MASKED_MAX_RAYS) return NERF_AMD_EUNSUP;
    return B * (((int64_t)N + 63) / 64);
}

int64_t nerf_amd_occupancy_workspace_bytes(int64_t B) {
    if (B < 0) return NERF_AMD_EINVAL;
    if (B > MASKED_MAX_RAYS) return NERF_AMD_EUNSUP;
    return nerf_amd_occ_workspace_bytes(B);
}

int nerf_amd_occupancy_mark(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed, int64_t ray_id0,
                            const uint32_t* bits, int64_t nx, int64_t ny, int64_t nz, const float* h_lo, const float* h_inv_step,
                            uint64_t* mask, int64_t* offsets, int64_t* live, void* workspace, int64_t B, int N, void* stream) {
    const int rc = occ_rays(rays, u, tbins, flags & ~NERF_AMD_OUTSIDE_EMPTY, B, N);
    if (rc) return rc;
    if (bad_grid(nx, ny, nz) || !bits || !h_lo || !h_inv_step || !offsets || !workspace) return NERF_AMD_EINVAL;
    if (B > 0 && !mask) return NERF_AMD_EINVAL;
    if (misaligned(mask, 8) || misaligned(offsets, 8) || misaligned(live, 8) || misaligned(workspace, 16)) return NERF_AMD_EINVAL;
    const MlpArgs a = rays_args(rays, u, tbins, flags & ~NERF_AMD_OUTSIDE_EMPTY, seed, ray_id0, B, N);
    return nerf_amd_launch_occ_mark(&a, bits, nx, ny, nz, h_lo, h_inv_step, (flags & NERF_AMD_OUTSIDE_EMPTY) ? 0 : 1,
                                    reinterpret_cast<unsigned long long*>(mask), reinterpret_cast<long long*>(offsets),
                                    reinterpret_cast<long long*>(live), workspace, B, S(stream));
}

int nerf_amd_occupancy_points(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed, int64_t ray_id0,
                              const uint64_t* mask, const int64_t* offsets, float* pts, int64_t max_points, int64_t B, int N,
                              void* stream) {
    const int rc = occ_rays(rays, u, tbins, flags, B, N);
    if (rc) return rc;
    if (max_points < 0) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    if (!mask || !offsets || (max_points > 0 && !pts) || misaligned(mask, 8) || misaligned(offsets, 8)) return NERF_AMD_EINVAL;
    const MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    return nerf_amd_launch_occ_emit(&a, reinterpret_cast<const unsigned long long*>(mask), reinterpret_cast<const long long*>(offsets),
                                    pts, max_points, B, S(stream));
}

int nerf_amd_volume_render_masked(const float* raw_live, const float* rays, const float* u, const float* tbins, uint32_t flags,
                                  uint64_t seed, int64_t ray_id0, const uint64_t* mask, const int64_t* offsets, float* rgb,
                                  float* disp, float* alpha, float* acc, float* w, int64_t B, int N, void* stream) {
    const int rc = occ_rays(rays, u, tbins, flags, B, N);
    if (rc) return rc;
    if (B == 0) return 0;
    if (!mask || !offsets || !rgb || !disp || !acc || misaligned(mask, 8) || misaligned(offsets, 8) || misaligned(raw_live, 16))
        return NERF_AMD_EINVAL;
    MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    a.rgb = rgb; a.disp = disp; a.alpha = alpha; a.acc = acc; a.w = w;
    return nerf_amd_launch_occ_composite(&a, reinterpret_cast<const unsigned long long*>(mask),
                                         reinterpret_cast<const long long*>(offsets), raw_live, B, S(stream));
}

int nerf_amd_volume_render_masked_pixels(const float* raw_live, const float* rays, const float* u, const float* tbins, uint32_t flags,
                                         uint64_t seed, int64_t ray_id0, const uint64_t* mask, const int64_t* offsets, float* pixels,
                                         int64_t B, int N, void* stream) {
    const int rc = occ_rays(rays, u, tbins, flags, B, N);
    if (rc) return rc;
    if (B == 0) return 0;
    if (!mask || !offsets || !pixels || misaligned(mask, 8) || misaligned(offsets, 8) || misaligned(raw_live, 16) ||
        misaligned(pixels, 16))
        return NERF_AMD_EINVAL;
    MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    a.pixels = pixels;
    return nerf_amd_launch_occ_composite(&a, reinterpret_cast<const unsigned long long*>(mask),
                                         reinterpret_cast<const long long*>(offsets), raw_live, B, S(stream));
}

// ---- training with the occupancy grid (csrc/occupancy_train.hip; not in the reference) ---------------------------------
int nerf_amd_volume_render_masked_backward(const float* raw_live, const float* rays, const float* u, const float* tbins,
                                           uint32_t flags, uint64_t seed, int64_t ray_id0, const uint64_t* mask,
                                           const int64_t* offsets, const float* g_rgb, const float* g_disp, const float* g_alpha,
                                           const float* g_acc, const float* g_w, float* d_raw_live, int64_t B, int N, void* stream) {
    const int rc = occ_rays(rays, u, tbins, flags, B, N);
    if (rc) return rc;
    if (N > COMPOSITE_BWD_MAX_N) return NERF_AMD_EUNSUP;
    if (B == 0) return 0;
    if (!mask || !offsets || misaligned(mask, 8) || misaligned(offsets, 8) || misaligned(raw_live, 16) ||
        misaligned(d_raw_live, 16) || (!raw_live != !d_raw_live))
        return NERF_AMD_EINVAL;
    const MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    MaskedBackwardArgs b{};                    // the five gradients, no MSE head, no sampler, no capacity clamp
    b.mask = reinterpret_cast<const unsigned long long*>(mask);
    b.offsets = reinterpret_cast<const long long*>(offsets);
    b.raw_live = raw_live; b.d_raw_live = d_raw_live;
    b.B = B; b.capacity = MASKED_NO_CLAMP;
    b.g_rgb = g_rgb; b.g_disp = g_disp; b.g_alpha = g_alpha; b.g_acc = g_acc; b.g_w = g_w;
    return nerf_amd_launch_masked_backward(&a, &b, S(stream));
}

int nerf_amd_occupancy_decay_max(float* state, const float* sigma_now, float decay, int64_t n, void* stream) {
    if (n < 0 || !(decay >= 0.f && decay <= 1.f)) return NERF_AMD_EINVAL;
    if (n == 0) return 0;
    if (!state || !sigma_now) return NERF_AMD_EINVAL;
    return nerf_amd_launch_occ_decay_max(state, sigma_now, decay, n, S(stream));
}

// the scene box: the box and the global interval first (host scalars, as the terminated render's eps and slab), then the
// rays / jitter / size rules of the masked stages -- the entry points that read ts[B,N] -- then the outputs
int nerf_amd_box_positions(const float* rays, const float* u, const float* tbins01, uint32_t flags, uint64_t seed,
                           int64_t ray_id0, const float* h_lo, const float* h_hi, float tn, float tf, float* ts, float* span,
                           int32_t* hit, int64_t B, int N, void* stream) {
    if (bad_box(h_lo, h_hi)) return NERF_AMD_EINVAL;
    if (!(tn < tf) || !(tn >= -3.402823466e38f) || !(tf <= 3.402823466e38f)) return NERF_AMD_EINVAL;       // also NaN
    const int rc = masked_rays_check(rays, u, tbins01, flags, B, N, N > MASKED_MAX_N);
    if (rc) return rc;
    if (misaligned(rays, 4) || misaligned(u, 4) || misaligned(tbins01, 4)) return NERF_AMD_EINVAL;
    if ((B > 0 && !ts) || misaligned(ts, 4) || misaligned(span, 4) || misaligned(hit, 4)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    const MlpArgs a = rays_args(rays, u, tbins01, flags, seed, ray_id0, B, N);
    return nerf_amd_launch_box_positions(&a, h_lo, h_hi, tn, tf, ts, span, hit, B, S(stream));
}

// the grid span: the grid (its bounds are the box the ray is clipped to) and the segment count first, then the box's rules in
// the box's order; probes > SPAN_MAX_PROBES is a size the kernel does not serve, beside N and B
int nerf_amd_span_positions(const float* rays, const float* u, const float* tbins01, uint32_t flags, uint64_t seed,
                            int64_t ray_id0, const uint32_t* bits, int64_t nx, int64_t ny, int64_t nz, const float* h_lo,
                            const float* h_hi, const float* h_inv_step, int probes, float tn, float tf, float* ts, float* span,
                            int32_t* hit, int64_t B, int N, void* stream) {
    if (!bits || bad_box(h_lo, h_hi) || bad_f32x3(h_inv_step)) return NERF_AMD_EINVAL;
    if (bad_grid(nx, ny, nz) || bad_span_probes(probes, nx, ny, nz)) return NERF_AMD_EINVAL;
    if (!(tn < tf) || !(tn >= -3.402823466e38f) || !(tf <= 3.402823466e38f)) return NERF_AMD_EINVAL;       // also NaN
    const int rc = masked_rays_check(rays, u, tbins01, flags, B, N, N > MASKED_MAX_N || probes > SPAN_MAX_PROBES);
    if (rc) return rc;
    if (misaligned(rays, 4) || misaligned(u, 4) || misaligned(tbins01, 4) || misaligned(bits, 4)) return NERF_AMD_EINVAL;
    if ((B > 0 && !ts) || misaligned(ts, 4) || misaligned(span, 4) || misaligned(hit, 4)) return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    const MlpArgs a = rays_args(rays, u, tbins01, flags, seed, ray_id0, B, N);
    return nerf_amd_launch_span_positions(&a, bits, nx, ny, nz, h_lo, h_hi, h_inv_step, probes, tn, tf, ts, span, hit, B, S(stream));
}

}  // extern "C"
