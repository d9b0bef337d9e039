// composite_backward_device.h -- the per-ray backward walk of the compositor, shared by its kernels:
// composite_backward_kernel<E> (composite.hip, dense raw[B, N, 4]), dense_head_kernel<.., E> (composite_head.hip, the dense
// head with its optional terms) and masked_backward_kernel<Up, NOISE, E> (occupancy_train.hip, the masked samples: the five
// gradients, or the MSE head under the capacity clamp, with the dense head's terms).  Behind each of the three the fine
// pass's sampler may run in the same wave (E > 0: the coarse head of a pair).
//
// d loss / d raw given the upstream gradients of the five outputs.  With G_i = dL/dw_i gathered from every consumer of w,
//   dL/dc_i     = w_i * g_rgb
//   dL/dalpha_i = G_i T_i - (1/f_i) * sum_{k>i} G_k w_k + g_alpha_i       (f = 1 - alpha + 1e-10)
//   dL/dsigma_i = dL/dalpha_i * e_i * delta_i * softplus'(sigma_i)        (e = exp(-softplus(sigma) delta) = 1 - alpha)
// ONE wavefront per ray, one sample per lane; chunks of 64 samples are walked forward once (recomputing alpha, T, w with the
// forward compositor's ops, composite_device.h) and backward once, the suffix sum over k > i a wave-level reverse scan.
//
// Every floating-point operation is one explicitly rounded op (mul_rn / add_rn / sub_rn / __fmaf_rn / a division), as in
// composite_device.h: the compiler has no contraction left to choose, so every caller writes the same bits from the same
// samples.  The one fused pair is G T - suffix / f; everything else rounds separately.
//
// The three axes on which the callers differ are compile-time choices; a term a caller does not have is not computed.
//   Src  -- the ray's samples, asked chunk by chunk in ascending order (DenseSamples below; MaskedSamplesBwd; either in
//           nerf_noise::Noisy<>, sigma_noise_device.h)
//   Up   -- the upstream gradients (FiveGrads: five pointers, each may be NULL; LossHead<BG, DIST, AFFINE>: the MSE loss
//           gradient formed here -- BG: behind a background colour, whose gradient to acc reaches every w_i; DIST: with the
//           distortion loss of the ray's weights beside the MSE, whose gradient joins G_i where FiveGrads adds g_w; AFFINE:
//           behind a per-image colour map of rgb, whose backward scales the gradient to rgb.  MseHead is the plain one)
//   Sink -- where the forward sweep's weights go (NoSink; PdfSink: the sampler's LDS slice, sample_pdf_device.h)
#pragma once
#include "appearance_device.h"          // LossHead<.., AFFINE>: the per-image colour map and its backward
#include "composite_device.h"
#include "composite_dist_device.h"      // LossHead<.., DIST, ..>: the distortion loss of a ray's weights

namespace nerf_composite {

// ---- sample sources --------------------------------------------------------------------------------------------------------
struct BwdSample {
    float t, t_next;                   // t(i), t(i + 1) (0 at the last sample, whose delta is 1e10)
    f32x4 c;                           // the network's output
    int row;                           // the row of d_raw this sample writes, -1 = none
};

struct DenseSamples {                  // ts / raw in HBM, row = i
    const float* ts;
    const f32x4* raw;
    __device__ __forceinline__ BwdSample chunk(int, int i, int, bool valid, int N) {
        BwdSample s{0.f, 0.f, f32x4{0.f, 0.f, 0.f, 0.f}, -1};
        if (valid) {
            s.t = ts[i];
            if (i + 1 < N) s.t_next = ts[i + 1];
            s.c = raw[i];
            s.row = i;
        }
        return s;
    }
};

// positions in the wave's LDS slice, the network's output at rank = set mask bits of the ray below i.  A sample whose bit
// is clear, or whose rank is not below n_kept, is (0, 0, 0, -inf): softplus' = 0, alpha = 0, w = 0, it receives nothing and
// adds exact zeros to the suffix sums.  A capacity clamp lives in how the caller forms `raw` and `n_kept`.
struct MaskedSamplesBwd {
    const float* ts;                   // the ray's N positions (LDS)
    const unsigned long long* m;       // the ray's mask words
    const f32x4* raw;                  // the row of the ray's first kept sample
    long long n_kept;
    long long before = 0;              // set mask bits of this ray in earlier chunks
    __device__ __forceinline__ BwdSample chunk(int ch, int i, int lane, bool valid, int N) {
        const unsigned long long mw = m[ch];
        BwdSample s{0.f, 0.f, f32x4{0.f, 0.f, 0.f, -__builtin_inff()}, -1};
        if (valid) {
            const long long rank = before + __popcll(mw & ((1ull << lane) - 1ull));
            s.t = ts[i];
            if (i + 1 < N) s.t_next = ts[i + 1];
            if (((mw >> lane) & 1ull) && rank < n_kept) {
                s.c = raw[rank];
                s.row = (int)rank;
            }
        }
        before += __popcll(mw);
        return s;
    }
};

// ---- upstream gradients ----------------------------------------------------------------------------------------------------
struct FiveGrads {                     // of rgb[B,3], disp[B], alpha[B,N], acc[B], w[B,N]; NULL = zero
    static constexpr bool MSE = false, BG = false, DIST = false, AFFINE = false;
    const float *g_rgb, *g_disp, *g_alpha, *g_acc, *g_w;
};

// loss = MSELoss(rgb, target) (train.py:52): d loss / d rgb = 2 (rgb - target) scale, formed from the forward sweep's rgb.
// Three optional terms, each BY DEFINITION -- and bit for bit -- a chain of the stages around the compositor:
//   BG      the MSE behind a background colour: rgb_bg = rgb + (1 - acc) bg (two rounded ops per channel, no fma).  The chain
//           compositor (rgb, acc) -> blend -> 2 (rgb_bg - target) scale -> the blend's backward (g_rgb passes through, g_acc =
//           -((g0 bg0 + g1 bg1) + g2 bg2)) -> compositor backward (g_rgb, g_acc): acc is summed with the forward compositor's
//           ops, g_acc joins G_i where FiveGrads adds gac.
//   DIST    loss = MSE + sum_rays coef D(w, t) (composite_dist_device.h).  The chain  compositor (rgb, acc, w) ->
//           nerf_amd_distortion_loss on that w (loss_ray, g_w) -> [blend] -> the MSE gradient -> [the blend's backward] ->
//           compositor backward (g_rgb, g_acc, g_w): G_i = (rgb terms + g_acc) + g_w_i.
//   AFFINE  the MSE behind a per-image colour correction (appearance_device.h): c' = (1 + a) rgb + b with the ray's row of
//           theta = (a, b).  The chain  compositor (rgb) -> nerf_amd_appearance_apply -> 2 (c' - target) scale ->
//           nerf_amd_appearance_apply_backward (g_rgb = g fl(1 + a); the ray's row of d loss / d theta = (g rgb, g)) ->
//           compositor backward (g_rgb).
// A term's fields are looked at only where the term is on; MseHead{target, rgb_out, scale} leaves them zero.
template <bool BG_, bool DIST_, bool AFFINE_>
struct LossHead {
    static_assert(!(BG_ && AFFINE_), "the order of the blend and the colour map in one chain is not defined");
    static constexpr bool MSE = true, BG = BG_, DIST = DIST_, AFFINE = AFFINE_;
    const float* target;               // [B,3]
    float* rgb_out;                    // [B,3]: the loss's prediction (rgb, rgb_bg or c'), or NULL
    float scale;                       // 1 / (3 B)
    const float* bg;                   // BG: one colour [3] (bg_stride 0) or one per ray [B,3] (bg_stride 3); no gradient
    long long bg_stride;
    float t_far, coef;                 // DIST: the last sample's interval ends at t_far; coef = lambda / (B (tf - tn))
    float* loss_ray;                   // DIST: [B]: coef D of each ray, or NULL
    const float* theta;                // AFFINE: one row per ray [B,6] (theta_stride 6) or one for all rays (theta_stride 0)
    long long theta_stride;
    float* g_theta;                    // AFFINE: [B,6]: every ray's own row of d loss / d theta (its image sums them)
};
using MseHead = LossHead<false, false, false>;

// The reference composites an EMPTY sample axis at N == 1 (composite_device.h): rgb = acc = 0 and no sample receives anything.
// So d_raw's one row is 0, the ray has no weight (D = 0), rgb_bg = bg exactly (through the blend's own three rounded ops),
// and c' = fl(fl(1 + a) 0) + b with the ray's row of g_theta = (g 0, g).  rout: the ray's row of d_raw.
template <class Up>
__device__ __forceinline__ void loss_head_empty_ray(const Up& up, int lane, long long ray, f32x4* rout) {
    if (lane != 0) return;
    rout[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (Up::DIST) {
        if (up.loss_ray) up.loss_ray[ray] = 0.f;
    }
    float c[3] = {0.f, 0.f, 0.f};
    if constexpr (Up::BG) {
        for (int k = 0; k < 3; ++k) c[k] = add_rn(0.f, mul_rn(sub_rn(1.0f, 0.f), up.bg[ray * up.bg_stride + k]));
    }
    if constexpr (Up::AFFINE) {
        const nerf_appearance::Row row = nerf_appearance::load_row(up.theta + ray * up.theta_stride);
        float gain[3], g[3], g_c[3], g_a[3];
        const float zero[3] = {0.f, 0.f, 0.f};
        nerf_appearance::gains(row, gain);
        for (int k = 0; k < 3; ++k) {
            c[k] = nerf_appearance::apply(gain[k], 0.f, row.b[k]);
            g[k] = mul_rn(mul_rn(2.0f, sub_rn(c[k], up.target[ray * 3 + k])), up.scale);
        }
        nerf_appearance::apply_backward(g, zero, gain, g_c, g_a);
        nerf_appearance::store_row(up.g_theta + ray * 6, g_a, g);
    }
    if (up.rgb_out) {
        for (int k = 0; k < 3; ++k) up.rgb_out[ray * 3 + k] = c[k];
    }
}

// ---- weight sinks ----------------------------------------------------------------------------------------------------------
struct NoSink {
    __device__ __forceinline__ void put(int, float, float) const {}
};
struct PdfSink {                       // the sampler's inputs: the positions and the forward compositor's weights
    float* ts;                         // NULL: the source's positions already are the sampler's
    float* w;
    __device__ __forceinline__ void put(int i, float t, float wt) const {
        if (ts) ts[i] = t;
        w[i] = wt;
    }
};

// rout: row 0 of this ray in d_raw.  N >= 2 (the callers handle the reference's empty sample axis at N == 1), N <= 64 CHUNKS.
template <int CHUNKS, class Src, class Up, class Sink>
__device__ __forceinline__ void composite_backward_ray(Src src, const Up& up, const Sink& sink, int N, int lane, float dnorm,
                                                       long long ray, f32x4* rout) {
    // forward sweep: per chunk keep alpha, T, fac, d alpha / d sigma, the colour and the row
    float al[CHUNKS], Tt[CHUNKS], fc[CHUNKS], ds[CHUNKS], tt[CHUNKS];
    f32x4 cc[CHUNKS];
    int rk[CHUNKS];
    float carry = 1.0f, depth = 0.f, accw = 0.f;
    float sr = 0.f, sg = 0.f, sb = 0.f;            // MSE head: the forward's rgb, for the loss gradient
    float sa = 0.f;                                // ... behind a background: the forward's acc
#pragma unroll
    for (int ch = 0; ch < CHUNKS; ++ch) {
        const int base = ch * 64;
        al[ch] = 0.f; Tt[ch] = 0.f; fc[ch] = 1.f; ds[ch] = 0.f; tt[ch] = 0.f;
        cc[ch] = f32x4{0.f, 0.f, 0.f, 0.f};
        rk[ch] = -1;
        if (base < N) {
            const int i = base + lane;
            const bool valid = i < N;
            const BwdSample s = src.chunk(ch, i, lane, valid, N);
            float a = 0.f, fac = 1.0f;
            if (valid) {
                const float sigma = s.c[3];
                const AlphaFactor f = alpha_factor((i == N - 1) ? 1e10f : sub_rn(s.t_next, s.t), dnorm, sigma);
                a = f.alpha; fac = f.fac;
                // softplus' as torch's backward forms it: z / (z + 1) keeps exp(sigma) down to the subnormals, where
                // 1 / (1 + exp(-sigma)) is 0 from sigma = -88.7 on (a last sample's delta = 1e10 brings that back up)
                const float spd = sigma > 20.f ? 1.0f : __fdiv_rn(f.z, add_rn(f.z, 1.0f));
                // e itself, not 1 - alpha: that recovers e to an absolute 2^-24, a relative 2^-24 / e on a nearly opaque sample
                ds[ch] = mul_rn(mul_rn(f.e, f.delta), spd);
                tt[ch] = s.t; cc[ch] = s.c; rk[ch] = s.row;
            }
            // the forward compositor's scan (composite_device.h): same tree, same rounded products
            const float incl = wave_scan_mul(fac);
            const float excl = dpp_move<0x138, 0xf>(1.0f, incl);          // wave_shr:1
            al[ch] = a; fc[ch] = fac; Tt[ch] = mul_rn(carry, excl);
            carry = mul_rn(carry, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(incl), 63)));
            if (valid) {
                const float wt = mul_rn(a, Tt[ch]);
                if constexpr (Up::MSE) {
                    // the same ops as the forward compositor (composite_device.h), so rgb_out equals its rgb
                    sr = __fmaf_rn(wt, cc[ch][0], sr); sg = __fmaf_rn(wt, cc[ch][1], sg); sb = __fmaf_rn(wt, cc[ch][2], sb);
                    if constexpr (Up::BG) sa = add_rn(sa, wt);
                } else {
                    depth = add_rn(depth, mul_rn(wt, tt[ch])); accw = add_rn(accw, wt);
                }
                sink.put(i, tt[ch], rk[ch] >= 0 ? wt : 0.f);       // exactly 0 at a dead or over-capacity sample
            }
        }
    }

    // upstream gradients that reach every w_i of the ray
    float gr, gg, gb, gdep = 0.f, gac = 0.f;
    if constexpr (Up::MSE) {
        sr = wave_total(sr); sg = wave_total(sg); sb = wave_total(sb);
        float b0 = 0.f, b1 = 0.f, b2 = 0.f;
        if constexpr (Up::BG) {     // sr, sg, sb become rgb_bg: the loss's prediction and the rgb output
            const float* bg = up.bg + ray * up.bg_stride;
            b0 = bg[0]; b1 = bg[1]; b2 = bg[2];
            const float through = sub_rn(1.0f, wave_total(sa));
            sr = add_rn(sr, mul_rn(through, b0)); sg = add_rn(sg, mul_rn(through, b1)); sb = add_rn(sb, mul_rn(through, b2));
        }
        [[maybe_unused]] float plain[3], gain[3];
        if constexpr (Up::AFFINE) {         // sr, sg, sb become c': the loss's prediction and the rgb output
            const nerf_appearance::Row row = nerf_appearance::load_row(up.theta + ray * up.theta_stride);
            nerf_appearance::gains(row, gain);
            plain[0] = sr; plain[1] = sg; plain[2] = sb;
            sr = nerf_appearance::apply(gain[0], sr, row.b[0]); sg = nerf_appearance::apply(gain[1], sg, row.b[1]);
            sb = nerf_appearance::apply(gain[2], sb, row.b[2]);
        }
        gr = mul_rn(mul_rn(2.0f, sub_rn(sr, up.target[ray * 3 + 0])), up.scale);
        gg = mul_rn(mul_rn(2.0f, sub_rn(sg, up.target[ray * 3 + 1])), up.scale);
        gb = mul_rn(mul_rn(2.0f, sub_rn(sb, up.target[ray * 3 + 2])), up.scale);
        if constexpr (Up::AFFINE) {         // the map's backward: the ray's row of g_theta, then g_rgb = g fl(1 + a)
            const float g[3] = {gr, gg, gb};
            float g_c[3], g_a[3];
            nerf_appearance::apply_backward(g, plain, gain, g_c, g_a);
            if (lane == 0) nerf_appearance::store_row(up.g_theta + ray * 6, g_a, g);
            gr = g_c[0]; gg = g_c[1]; gb = g_c[2];
        }
        if constexpr (Up::BG) gac = -add_rn(add_rn(mul_rn(gr, b0), mul_rn(gg, b1)), mul_rn(gb, b2));
        if (up.rgb_out && lane == 0) { up.rgb_out[ray * 3 + 0] = sr; up.rgb_out[ray * 3 + 1] = sg; up.rgb_out[ray * 3 + 2] = sb; }
    } else {
        depth = wave_sum(depth); accw = wave_sum(accw);
        gr = up.g_rgb ? up.g_rgb[ray * 3 + 0] : 0.f; gg = up.g_rgb ? up.g_rgb[ray * 3 + 1] : 0.f;
        gb = up.g_rgb ? up.g_rgb[ray * 3 + 2] : 0.f;
        gac = up.g_acc ? up.g_acc[ray] : 0.f;
        if (up.g_disp) {
            const float q = __fdiv_rn(depth, accw);
            if (q > 1e-10f) {                        // disp = 1/q there; the clamp branch has zero slope
                const float dq = __fdiv_rn(-up.g_disp[ray], mul_rn(q, q));
                gdep = __fdiv_rn(dq, accw);
                gac = add_rn(gac, __fdiv_rn(mul_rn(-dq, depth), mul_rn(accw, accw)));
            }
        }
    }
    // the distortion term on the forward sweep's weights: its gradient to every w_i, and the ray's loss value
    [[maybe_unused]] float gw[Up::DIST ? CHUNKS : 1];
    if constexpr (Up::DIST) {
        float wv[CHUNKS];
#pragma unroll
        for (int ch = 0; ch < CHUNKS; ++ch) wv[ch] = (ch * 64 + lane < N) ? mul_rn(al[ch], Tt[ch]) : 0.f;
        const float dist = distortion_ray<CHUNKS>(tt, wv, N, lane, up.t_far, up.coef, gw);
        if (up.loss_ray && lane == 0) up.loss_ray[ray] = dist;
    }
    // backward sweep over chunks, carrying sum_{k in later chunks} G_k w_k
    float later = 0.f;
#pragma unroll
    for (int ch = CHUNKS - 1; ch >= 0; --ch) {
        const int base = ch * 64;
        if (base < N) {
            const int i = base + lane;
            const bool valid = i < N;
            const float w = mul_rn(al[ch], Tt[ch]);
            float G = 0.f;
            if (valid) {
                G = add_rn(add_rn(mul_rn(gr, cc[ch][0]), mul_rn(gg, cc[ch][1])), mul_rn(gb, cc[ch][2]));
                if constexpr (Up::BG) G = add_rn(G, gac);
                if constexpr (Up::DIST) G = add_rn(G, gw[ch]);
                if constexpr (!Up::MSE) {
                    G = add_rn(add_rn(G, mul_rn(gdep, tt[ch])), gac);
                    if (up.g_w) G = add_rn(G, up.g_w[ray * N + i]);
                }
            }
            float tot;
            const float suffix = add_rn(wave_suffix_excl(valid ? mul_rn(G, w) : 0.f, lane, tot), later);
            later = add_rn(later, tot);
            if (valid && rk[ch] >= 0) {
                float dalpha = __fmaf_rn(G, Tt[ch], -__fdiv_rn(suffix, fc[ch]));
                if constexpr (!Up::MSE) {
                    if (up.g_alpha) dalpha = add_rn(dalpha, up.g_alpha[ray * N + i]);
                }
                const f32x4 o = {mul_rn(w, gr), mul_rn(w, gg), mul_rn(w, gb), mul_rn(dalpha, ds[ch])};
                rout[rk[ch]] = o;
            }
        }
    }
}

}  // namespace nerf_composite
