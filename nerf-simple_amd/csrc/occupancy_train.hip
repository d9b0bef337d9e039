// occupancy_train.hip -- training with empty-space skipping: the backward of the masked compositor, under every head that
// runs it, and the running density volume a training occupancy grid is refreshed from.  Not in the reference.
//
//   masked_backward_kernel<Up, E> -- d loss / d raw_live of nerf_amd_volume_render_masked.  One wavefront per ray, lane =
//       ORIGINAL sample index, N walked in chunks of 64 by composite_backward_ray (composite_backward_device.h), the walk of
//       the dense raw[B, N, 4]: positions recomputed (fetch_point_rays) into the wave's LDS slice, the network's output read
//       at the ray's first row + rank for a kept sample -- rank from popcounts of the mask words -- and (0, 0, 0, -inf) for
//       a dead one.  A dead sample has softplus' = 0, alpha = 0 and w = 0 there: it receives nothing and adds exact zeros to
//       the suffix sums.  The result is the rows at the kept samples of the dense backward on the overwritten raw, bit for
//       bit.  No atomics: a row is written by exactly one lane, and two runs write the same bytes.  Three axes:
//         Up        FiveGrads: the five upstream gradients are given (nerf_amd_volume_render_masked_backward);
//                   MseHead: g_rgb = 2 (rgb - gt) / (3 B) is formed from the sweep's own forward, and rgb is written
//                   (the graphed steps' heads, occupancy_graph.hip; DESIGN.md sections 14, 15);
//         E         0: no sampler.  1, 2, 4, 8: the fine pass's sample placement (sample_pdf_device.h, E keys per lane) runs
//                   in the same wave from the weights of the forward sweep, as composite.hip's dense coarse head does it:
//                   wt = mul_rn(alpha, T) goes from registers to the wave's LDS slice beside the positions (a dead or
//                   over-capacity sample carries exactly 0), and the sampler reads both there.  w never reaches HBM.
//                   Nc <= 256: four chunks; LDS per block 4 * (6 KB + 256 E B), the dense head's figures;
//         capacity  a clamp C of every row index (wave-uniform): sample i of ray b is KEPT iff its mask bit is set and
//                   offsets[b] + (set bits of the ray below i) < C, and the rows [min(P', C), C) are zero-filled, so every
//                   row of d_raw_live[C, 4] is written by exactly one lane on every launch.  MASKED_NO_CLAMP: the kept rows
//                   are the live ones, nothing else is written and offsets[B] is not read.
//   occ_decay_max_kernel -- state = max(fl(state decay), softplus(sigma_now)), softplus as the compositor's.
#include "composite_backward_device.h"
#include "sample_pdf_device.h"
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

template <class Up, int E>
__global__ __launch_bounds__(MASKED_THREADS) void masked_backward_kernel(MlpArgs a, MaskedBackwardArgs b) {
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
    const bool empty = N == 1 || n_kept <= 0;
    if (empty) {
        // N == 1: the reference composites an EMPTY sample axis (composite_device.h), no output depends on raw.  Nothing
        // kept: every sample is (0, 0, 0, -inf), w = 0 throughout.  Either way rgb = 0 and a kept row (N == 1) gets zeros.
        if (lane == 0) {
            if constexpr (Up::MSE) { b.rgb[ray * 3 + 0] = 0.f; b.rgb[ray * 3 + 1] = 0.f; b.rgb[ray * 3 + 2] = 0.f; }
            if (n_kept > 0 && (m[0] & 1ull)) rout[0] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if constexpr (E == 0) return;
    }
    fill_ray_positions(a, ray, lane, rts);
    const auto up = [&] {
        // loss = MSELoss(rgb, gt) (train.py:52): only rgb feeds it
        if constexpr (Up::MSE) return MseHead{b.target, b.rgb, b.scale};
        else return FiveGrads{b.g_rgb, b.g_disp, b.g_alpha, b.g_acc, b.g_w};
    }();
    const nerf_composite::MaskedSamplesBwd src{rts, m, reinterpret_cast<const f32x4*>(b.raw_live) + first, n_kept};
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

extern "C" int nerf_amd_launch_masked_backward(const MlpArgs* args, const MaskedBackwardArgs* head, hipStream_t stream) {
    (void)hipGetLastError();
    MaskedBackwardArgs b = *head;
    if (b.B == 0) return 0;
    if (b.ts_out && !b.target) return -2;      // the sampler runs behind the MSE head only
    if (b.ts_out ? nerf_pdf::unsupported_sizes(args->N, b.Nf) : args->N > OCCT_MAX_N) return -2;
    b.scale = 1.0f / (3.0f * (float)b.B);
    const dim3 grid((unsigned)((b.B + MASKED_RAYS_PER_BLOCK - 1) / MASKED_RAYS_PER_BLOCK)), block(MASKED_THREADS);
#define MASKED_BACKWARD(UP_, E_) hipLaunchKernelGGL((masked_backward_kernel<UP_, E_>), grid, block, 0, stream, *args, b)
    if (!b.target) MASKED_BACKWARD(FiveGrads, 0);
    else if (!b.ts_out) MASKED_BACKWARD(MseHead, 0);
    else switch (nerf_pdf::keys_per_lane(b.Nf)) {
        case 1: MASKED_BACKWARD(MseHead, 1); break;
        case 2: MASKED_BACKWARD(MseHead, 2); break;
        case 4: MASKED_BACKWARD(MseHead, 4); break;
        default: MASKED_BACKWARD(MseHead, 8); break;
    }
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
