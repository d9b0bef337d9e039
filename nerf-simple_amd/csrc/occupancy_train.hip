// occupancy_train.hip -- training with empty-space skipping: the backward of the masked compositor, under every head that
// runs it, and the running density volume a training occupancy grid is refreshed from.  Not in the reference.
//
//   masked_backward_kernel<Up, NOISE, E> -- d loss / d raw_live of nerf_amd_volume_render_masked, the one walk of every masked
//       backward and head.  One wavefront per ray, lane = ORIGINAL sample index, N walked in chunks of 64 by
//       composite_backward_ray (composite_backward_device.h), the walk of the dense raw[B, N, 4]: positions recomputed
//       (fetch_point_rays) into the wave's LDS slice, the network's output read at the ray's first row + rank for a kept
//       sample -- rank from popcounts of the mask words -- and (0, 0, 0, -inf) for a dead one.  A dead sample has
//       softplus' = 0, alpha = 0 and w = 0 there: it receives nothing and adds exact zeros to the suffix sums.  The result is
//       the rows at the kept samples of the dense backward on the overwritten raw, bit for bit.  No atomics: a row is written
//       by exactly one lane, and two runs write the same bytes.  Twenty-five instantiations, the combinations the one launcher
//       below reaches, on four axes:
//         Up        FiveGrads: the five upstream gradients are given (nerf_amd_volume_render_masked_backward);
//                   MseHead: g_rgb = 2 (rgb - gt) / (3 B) is formed from the sweep's own forward, and rgb is written
//                   (the graphed steps' heads, occupancy_graph.hip; DESIGN.md sections 14, 15);
//                   LossHead<BG, DIST, false>: that head behind a background colour, with the distortion loss beside the
//                   MSE, or both (the training controls, masked_controls.hip).  A head's empty ray is
//                   the dense head's (loss_head_empty_ray), its row a register where the ray owns none;
//         NOISE     Noisy<> around the source (sigma_noise_device.h): noise on the raw density of the kept samples;
//         E         0: no sampler.  1, 2, 4, 8, behind the MseHead -- plain, or behind a background and / or with noise (the
//                   coarse head of the masked pair with its controls, DESIGN.md section 35: the sampler sees the weights of
//                   the NOISY masked compositor, the background never touches them) -- : the fine pass's sample placement
//                   (sample_pdf_device.h, E keys per lane) runs in the same wave from the weights of the forward sweep, as
//                   composite.hip's dense coarse head does it: wt = mul_rn(alpha, T) goes from registers to the wave's LDS
//                   slice beside the positions (a dead or over-capacity sample carries exactly 0), and the sampler reads
//                   both there.  w never reaches HBM.  Nc <= 256: four chunks; LDS per block 4 * (6 KB + 256 E B), the
//                   dense head's figures;
//         capacity  a clamp C of every row index (wave-uniform): sample i of ray b is KEPT iff its mask bit is set and
//                   offsets[b] + (set bits of the ray below i) < C, and the rows [min(P', C), C) are zero-filled, so every
//                   row of d_raw_live[C, 4] is written by exactly one lane on every launch.  MASKED_NO_CLAMP: the kept rows
//                   are the live ones, nothing else is written and offsets[B] is not read.
//   occ_decay_max_kernel -- state = max(fl(state decay), softplus(sigma_now)), softplus as the compositor's.
#include "composite_backward_device.h"
#include "sample_pdf_device.h"
#include "sigma_noise_device.h"
#include "occ_scan_device.h"
#include "launchers.h"

namespace {

using nerf_composite::FiveGrads;
using nerf_composite::MseHead;
constexpr int OCCT_MAX_N = nerf_layout::COMPOSITE_BWD_MAX_N;               // N <= 512, the dense backward's limit

// the wave's LDS slice: the ray's positions, and with a sampler its workspace (whose ts[] the positions then are) and weights
template <int E>
struct MaskedLds {
    nerf_pdf::WaveLds<E> pdf;
    float w[nerf_pdf::MAXC];
    __device__ float* ts() { return pdf.ts; }
};
template <>
struct MaskedLds<0> {
    float t[OCCT_MAX_N];
    __device__ float* ts() { return t; }
};

template <class Up, bool NOISE, int E>
__global__ __launch_bounds__(MASKED_THREADS) void masked_backward_kernel(MlpArgs a, MaskedBackwardArgs b) {
    static_assert(E == 0 || (Up::MSE && !Up::DIST && !Up::AFFINE), "the sampler runs behind the MSE head, plain or with background / noise");
    static_assert(Up::MSE || !NOISE, "the terms belong to the loss head");
    constexpr int CHUNKS = E ? nerf_pdf::MAXC / 64 : nerf_layout::COMPOSITE_BWD_MAX_CHUNKS;
    __shared__ MaskedLds<E> lds[MASKED_RAYS_PER_BLOCK];
    const int wv = threadIdx.x >> 6;
    const long long ray = (long long)blockIdx.x * MASKED_RAYS_PER_BLOCK + wv;
    const int lane = threadIdx.x & 63;
    const int N = a.N;                         // with a sampler: 3 <= N <= 256
    if (b.capacity != MASKED_NO_CLAMP) {
        // the surplus rows [min(P', C), C) of d_raw_live: exact zeros, grid-stride (no wave depends on another's rows)
        const long long kept = min_ll(b.offsets[b.B], b.capacity);
        f32x4* pad = reinterpret_cast<f32x4*>(b.d_raw_live) + kept;
        for (long long r = (long long)blockIdx.x * MASKED_THREADS + threadIdx.x; r < b.capacity - kept;
             r += (long long)gridDim.x * MASKED_THREADS)
            pad[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (ray >= b.B) return;                    // whole wave leaves together; no workgroup barrier below
    const long long first = min_ll(b.offsets[ray], b.capacity);
    const long long n_kept = min_ll(b.offsets[ray + 1], b.capacity) - first;
    if constexpr (!Up::MSE) {
        if (!b.raw_live) return;               // NULL buffers: P' = 0 only
    }
    const unsigned long long* m = b.mask + ray * ((N + 63) >> 6);
    f32x4* rout = reinterpret_cast<f32x4*>(b.d_raw_live) + first;
    float* rts = lds[wv].ts();
    const auto up = [&] {
        // loss = MSELoss(rgb, gt) (train.py:52), with the head's terms: only rgb (and, behind a background, acc) feeds it
        if constexpr (Up::MSE)
            return Up{b.target, b.rgb, b.scale, b.bg, b.bg_stride, b.t_far, b.coef, b.loss_ray, nullptr, 0, nullptr};
        else return FiveGrads{b.g_rgb, b.g_disp, b.g_alpha, b.g_acc, b.g_w};
    }();
    const bool empty = N == 1 || n_kept <= 0;
    if (empty) {
        // N == 1: the reference composites an EMPTY sample axis (composite_device.h), no output depends on raw.  Nothing
        // kept: every sample is (0, 0, 0, -inf), w = 0 throughout.  Either way the ray has no weight and a kept row (N == 1)
        // gets zeros: the dense head's empty ray (rgb = bg through the blend's own ops, 0 without one; D = 0), whose one row
        // may not exist here.
        const bool owns_row = n_kept > 0 && (m[0] & 1ull);
        if constexpr (!Up::MSE) {
            if (lane == 0 && owns_row) rout[0] = f32x4{0.f, 0.f, 0.f, 0.f};
        } else if (owns_row) {
            nerf_composite::loss_head_empty_ray(up, lane, ray, rout);
        } else {
            f32x4 none;                        // a register: the routine's store of the row goes nowhere
            nerf_composite::loss_head_empty_ray(up, lane, ray, &none);
        }
        if constexpr (E == 0) return;
    }
    fill_ray_positions(a, ray, lane, rts);
    const auto src = [&] {
        using nerf_composite::MaskedSamplesBwd;
        const auto masked = MaskedSamplesBwd{rts, m, reinterpret_cast<const f32x4*>(b.raw_live) + first, n_kept};
        if constexpr (NOISE)
            return nerf_noise::Noisy<MaskedSamplesBwd>{masked, b.std, nerf_noise::noise_key(b.noise_seed, b.seed_mem),
                                                       (unsigned long long)((a.ray_id0 + ray) * N)};
        else return masked;
    }();
    if constexpr (E == 0) {
        nerf_composite::composite_backward_ray<CHUNKS>(src, up, nerf_composite::NoSink{}, N, lane, ray_dnorm(a, ray), ray, rout);
    } else {
        float* rw = lds[wv].w;
        // nothing kept: the sampler's 1e-5 floor spreads the new samples uniformly.  Otherwise the sweep's weights, exactly 0
        // at a dead sample
        if (empty) {
            for (int i = lane; i < N; i += 64) rw[i] = 0.f;
        } else {
            nerf_composite::composite_backward_ray<CHUNKS>(src, up, nerf_composite::PdfSink{nullptr, rw}, N, lane,
                                                           ray_dnorm(a, ray), ray, rout);
        }
        // the fine pass's positions from this ray's weights (nerf_amd_sample_pdf's body, same draws)
        wave_lds_fence();
        nerf_pdf::sample_ray<E>(lds[wv].pdf, rw, N, b.Nf, lane, b.u_f, (a.flags & NERF_FLAG_DEVICE_RNG) != 0, effective_seed(a),
                                a.ray_id0, ray, b.ts_out + ray * (long long)(N + b.Nf));
    }
}

__global__ __launch_bounds__(256) void occ_decay_max_kernel(float* __restrict__ state, const float* __restrict__ sigma_now,
                                                            float decay, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float s = sigma_now[i];
        const float sp = nerf_composite::softplus(s, expf(s));
        const float dcy = mul_rn(state[i], decay);
        // the maximum that keeps a NaN of either side (a NaN state is live in nerf_amd_occupancy_from_density)
        state[i] = (dcy != dcy) ? dcy : (sp != sp) ? sp : (dcy > sp ? dcy : sp);
    }
}

}  // namespace

extern "C" int nerf_amd_occ_train_max_n(void) { return OCCT_MAX_N; }

// The head's terms are on where std != 0 (noise), bg != NULL, coef != 0 (distortion); loss_ray without the distortion term
// gets its zeros here, so no kernel carries code for a term it does not have.
extern "C" int nerf_amd_launch_masked_backward(const MlpArgs* args, const MaskedBackwardArgs* head, hipStream_t stream) {
    (void)hipGetLastError();
    MaskedBackwardArgs b = *head;
    if (b.B == 0) return 0;
    const bool noise = b.std != 0.f, bg = b.bg != nullptr, dist = b.coef != 0.f, term = noise || bg || dist;
    // the sampler and the terms run behind the MSE head only; the sampler with the background and the noise, not with the
    // distortion term
    if (((b.ts_out || term) && !b.target) || (b.ts_out && dist)) return -2;
    if (b.ts_out ? nerf_pdf::unsupported_sizes(args->N, b.Nf) : args->N > OCCT_MAX_N) return -2;
    if (b.loss_ray && !dist) {
        const hipError_t e = hipMemsetAsync(b.loss_ray, 0, (size_t)b.B * sizeof(float), stream);
        if (e != hipSuccess) return (int)e;
    }
    b.scale = 1.0f / (3.0f * (float)b.B);
    const dim3 grid((unsigned)((b.B + MASKED_RAYS_PER_BLOCK - 1) / MASKED_RAYS_PER_BLOCK)), block(MASKED_THREADS);
#define MASKED_BACKWARD(...) hipLaunchKernelGGL((masked_backward_kernel<__VA_ARGS__>), grid, block, 0, stream, *args, b)
#define MASKED_HEAD(NOISE_, BG_, DIST_, E_) MASKED_BACKWARD(nerf_composite::LossHead<BG_, DIST_, false>, NOISE_, E_)
    if (!b.target) MASKED_BACKWARD(FiveGrads, false, 0);
    else if (b.ts_out) nerf_pdf::with_keys_per_lane(b.Nf, [&](auto e) {        // the coarse head of a pair: term = noise || bg
        if (!term) MASKED_BACKWARD(MseHead, false, e());
        else with_noise_bg(noise, bg, [&](auto n, auto g) { MASKED_HEAD(n(), g(), false, e()); });
    });
    else if (!term) MASKED_BACKWARD(MseHead, false, 0);
    else if (dist && !noise && !bg) MASKED_HEAD(false, false, true, 0);
    else if (dist) with_noise_bg(noise, bg, [&](auto n, auto g) { MASKED_HEAD(n(), g(), true, 0); });
    else with_noise_bg(noise, bg, [&](auto n, auto g) { MASKED_HEAD(n(), g(), false, 0); });
#undef MASKED_HEAD
#undef MASKED_BACKWARD
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_occ_decay_max(float* state, const float* sigma_now, float decay, long long n, hipStream_t stream) {
    (void)hipGetLastError();
    if (n == 0) return 0;
    long long blocks = (n + 255) / 256;
    if (blocks > 65536 * 16) blocks = 65536 * 16;
    hipLaunchKernelGGL(occ_decay_max_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, state, sigma_now, decay, n);
    return (int)hipGetLastError();
}

