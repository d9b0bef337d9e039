// image_metrics.hip -- image quality on the device: per-channel squared error, max(gt) and SSIM of M image pairs, read in
// place with the caller's row strides (render_view's [H W, 4] pixels against the [H W, 3] colour table).  The contract is
// include/nerf_amd.h; the float64 definition is restated by tests/ssim_model.py; DESIGN.md section 27.
//
//   window   g_k = exp(-(k-5)^2 / 4.5) / sum, k = 0..10: normalised in double, rounded ONCE to fp32 (WINDOW below);
//            G_ij = g_i g_j
//   per position (y, x) in [0, H-10) x [0, W-10) and channel, sums over the 11 x 11 window, sum G x evaluated row by row as
//   sum_i g_i (sum_j g_j x_ij), taps in ascending order:
//     pass 1:  mu_a = sum G a,  mu_b = sum G b
//     pass 2:  s_aa = sum G (a - mu_a)^2,  s_ab = sum G (a - mu_a)(b - mu_b),  s_bb = sum G (b - mu_b)^2  (all 121 taps)
//     ssim = (2 mu_a mu_b + C1)(2 s_ab + C2) / ((mu_a^2 + mu_b^2 + C1)(s_aa + s_bb + C2))
//   The CENTRED second moments are the point: E[a^2] - mu^2 in fp32 cancels to 5e-4 on a white background, the centred
//   form stays within 17 units of 2^-24.  Every operation is rounded on its own (mul_rn / add_rn / sub_rn / __fdiv_rn:
//   hipcc would contract a*b+c), which also makes a == b give num == den bit for bit: the quotient is exactly 1.
//
// A workgroup of 256 threads owns the T x T pixels of its tile -- every pixel of the image lies in exactly one tile, so the
// squared error needs no halo rule -- and the output positions among them.  It stages the (T+10)^2 pixels behind the tile
// of both images, channel-planar, in LDS (44,352 B); a thread then owns 4 neighbouring positions of one row and reads 14
// values per window row for them.  Per-tile partial sums (double) go to the workspace; a second launch, one block per
// image, adds them in a fixed order.  No atomics, no counter: two runs write the same bytes.
#include "nerf_device.h"
#include "launchers.h"

namespace {

constexpr int T = 32;                     // tile edge (tests/test_gpu_metrics.py states it too)
constexpr int WIN = 11, HALO = WIN - 1;
constexpr int R = T + HALO;               // staged rows / columns
constexpr int LW = 44;                    // LDS row pitch (floats)
constexpr int THREADS = 256;
constexpr int PX = 4;                     // positions per thread: T * T / PX = THREADS
constexpr int NPART = 7;                  // per tile: sse r g b, max_gt, ssim sums r g b
static_assert(T * T == THREADS * PX && T % PX == 0 && (T - PX) + (PX - 1) + HALO < LW, "tile shape");

// g_k = exp(-(k-5)^2 / 4.5), normalised to sum 1 in double and rounded once to fp32 (tests/test_metrics_cpu.py reads this row)
__constant__ float WINDOW[WIN] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f,
                                  0x1.b43c4p-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};

__device__ __forceinline__ double max_nan(double a, double b) {          // torch.max: a NaN wins
    return a != a ? a : (b != b ? b : (b > a ? b : a));
}

// sum (or max_nan) of v over the block, in a fixed order; valid in thread 0
template <bool MAX>
__device__ __forceinline__ double block_fold(double v, double* part) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_down(v, d, 64);
        v = MAX ? max_nan(v, o) : v + o;
    }
    __syncthreads();                                                    // `part` may still be read from the fold before
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = part[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) t = MAX ? max_nan(t, part[w]) : t + part[w];
    return t;
}

template <bool SSIM>
__global__ __launch_bounds__(THREADS) void image_metrics_tile_kernel(const float* __restrict__ pred, long long pred_stride,
                                                                     const float* __restrict__ gt, long long gt_stride,
                                                                     float* __restrict__ ssim_map, double* __restrict__ ws,
                                                                     long long M, int H, int W, int tiles_x) {
    __shared__ float s[2][3][R * LW];
    __shared__ double part[THREADS / 64];
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * T, x0 = tx * T;
    const int OH = H - HALO, OW = W - HALO;                              // output positions (SSIM: both >= 1)
    const int row = threadIdx.x >> 3, x4 = (threadIdx.x & 7) * PX;
    const int rows = SSIM ? R : T;                                       // staged extent
    const long long tiles = (long long)gridDim.x;

    for (long long m = blockIdx.y; m < M; m += gridDim.y) {
        __syncthreads();                                                 // the previous image's reads are done
        for (int idx = threadIdx.x; idx < rows * rows; idx += THREADS) {
            const int r = idx / rows, c = idx - r * rows;
            const long long gy = (long long)y0 + r, gx = (long long)x0 + c;      // x0 + c may leave an int at W near 2^31
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f;
            if (gy < H && gx < W) {
                const long long pix = (m * H + gy) * (long long)W + gx;
                const float* pa = pred + pix * pred_stride;
                const float* pb = gt + pix * gt_stride;
                a0 = pa[0]; a1 = pa[1]; a2 = pa[2];
                b0 = pb[0]; b1 = pb[1]; b2 = pb[2];
            }
            const int o = r * LW + c;
            s[0][0][o] = a0; s[0][1][o] = a1; s[0][2][o] = a2;
            s[1][0][o] = b0; s[1][1][o] = b1; s[1][2][o] = b2;
        }
        __syncthreads();

        double acc[NPART];
#pragma unroll
        for (int k = 0; k < NPART; ++k) acc[k] = 0.0;
        acc[3] = -__builtin_inf();

        // squared error and max(gt) of the pixels this tile owns
        if (y0 + row < H) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int p = 0; p < PX; ++p) {
                    if (x0 + x4 + p < W) {
                        const float a = s[0][c][row * LW + x4 + p], b = s[1][c][row * LW + x4 + p];
                        const float d = sub_rn(a, b);
                        acc[c] += (double)mul_rn(d, d);
                        acc[3] = max_nan(acc[3], (double)b);
                    }
                }
            }
        }

        if constexpr (SSIM) {
            if (y0 < OH && x0 < OW) {                                    // block-uniform: the tile has output positions
                const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);       // the double products, rounded once
                const int oy = y0 + row;
#pragma unroll 1
                for (int c = 0; c < 3; ++c) {
                    const float* A = &s[0][c][row * LW + x4];
                    const float* B = &s[1][c][row * LW + x4];
                    float ma[PX], mb[PX];
                    double sc = 0.0;
#pragma unroll
                    for (int p = 0; p < PX; ++p) ma[p] = mb[p] = 0.f;
#pragma unroll 1
                    for (int i = 0; i < WIN; ++i) {
                        float ra[PX + HALO], rb[PX + HALO];
#pragma unroll
                        for (int k = 0; k < PX + HALO; ++k) { ra[k] = A[i * LW + k]; rb[k] = B[i * LW + k]; }
                        const float gi = WINDOW[i];
#pragma unroll
                        for (int p = 0; p < PX; ++p) {
                            float ha = 0.f, hb = 0.f;                   // the window row, then its weight
#pragma unroll
                            for (int j = 0; j < WIN; ++j) {
                                ha = add_rn(ha, mul_rn(WINDOW[j], ra[p + j]));
                                hb = add_rn(hb, mul_rn(WINDOW[j], rb[p + j]));
                            }
                            ma[p] = add_rn(ma[p], mul_rn(gi, ha));
                            mb[p] = add_rn(mb[p], mul_rn(gi, hb));
                        }
                    }
                    float saa[PX], sab[PX], sbb[PX];
#pragma unroll
                    for (int p = 0; p < PX; ++p) saa[p] = sab[p] = sbb[p] = 0.f;
#pragma unroll 1
                    for (int i = 0; i < WIN; ++i) {
                        float ra[PX + HALO], rb[PX + HALO];
#pragma unroll
                        for (int k = 0; k < PX + HALO; ++k) { ra[k] = A[i * LW + k]; rb[k] = B[i * LW + k]; }
                        const float gi = WINDOW[i];
#pragma unroll
                        for (int p = 0; p < PX; ++p) {
                            float haa = 0.f, hab = 0.f, hbb = 0.f;
#pragma unroll
                            for (int j = 0; j < WIN; ++j) {
                                const float da = sub_rn(ra[p + j], ma[p]), db = sub_rn(rb[p + j], mb[p]);
                                haa = add_rn(haa, mul_rn(WINDOW[j], mul_rn(da, da)));
                                hab = add_rn(hab, mul_rn(WINDOW[j], mul_rn(da, db)));
                                hbb = add_rn(hbb, mul_rn(WINDOW[j], mul_rn(db, db)));
                            }
                            saa[p] = add_rn(saa[p], mul_rn(gi, haa));
                            sab[p] = add_rn(sab[p], mul_rn(gi, hab));
                            sbb[p] = add_rn(sbb[p], mul_rn(gi, hbb));
                        }
                    }
#pragma unroll
                    for (int p = 0; p < PX; ++p) {
                        const float n1 = add_rn(mul_rn(2.f, mul_rn(ma[p], mb[p])), C1);
                        const float n2 = add_rn(mul_rn(2.f, sab[p]), C2);
                        const float d1 = add_rn(add_rn(mul_rn(ma[p], ma[p]), mul_rn(mb[p], mb[p])), C1);
                        const float d2 = add_rn(add_rn(saa[p], sbb[p]), C2);
                        const float v = __fdiv_rn(mul_rn(n1, n2), mul_rn(d1, d2));
                        const int ox = x0 + x4 + p;
                        if (oy < OH && ox < OW) {
                            sc += (double)v;
                            if (ssim_map) ssim_map[((m * OH + oy) * (long long)OW + ox) * 3 + c] = v;
                        }
                    }
                    acc[4] = c == 0 ? sc : acc[4];
                    acc[5] = c == 1 ? sc : acc[5];
                    acc[6] = c == 2 ? sc : acc[6];
                }
            }
        }

        double* out = ws + (m * tiles + tile) * NPART;
#pragma unroll
        for (int k = 0; k < NPART; ++k) {
            if (!SSIM && k > 3) break;
            const double t = (k == 3) ? block_fold<true>(acc[k], part) : block_fold<false>(acc[k], part);
            if (threadIdx.x == 0) out[k] = t;
        }
    }
}

// one block per image: the tiles' partials in a fixed order
__global__ __launch_bounds__(THREADS) void image_metrics_reduce_kernel(const double* __restrict__ ws, double* __restrict__ sums,
                                                                       double* __restrict__ ssim, long long M, long long tiles,
                                                                       double positions) {
    __shared__ double part[THREADS / 64];
    for (long long m = blockIdx.x; m < M; m += gridDim.x) {
        double acc[NPART];
#pragma unroll
        for (int k = 0; k < NPART; ++k) acc[k] = 0.0;
        acc[3] = -__builtin_inf();
        for (long long t = threadIdx.x; t < tiles; t += THREADS) {
            const double* p = ws + (m * tiles + t) * NPART;
#pragma unroll
            for (int k = 0; k < NPART; ++k) {
                if (k > 3 && !ssim) break;
                acc[k] = (k == 3) ? max_nan(acc[k], p[k]) : acc[k] + p[k];
            }
        }
#pragma unroll
        for (int k = 0; k < NPART; ++k) {
            if (k > 3 && !ssim) break;
            const double t = (k == 3) ? block_fold<true>(acc[k], part) : block_fold<false>(acc[k], part);
            if (threadIdx.x == 0) {
                if (k <= 3) sums[m * 4 + k] = t;
                else ssim[m * 3 + (k - 4)] = t / positions;
            }
        }
    }
}

// in 64 bits: W + T - 1 leaves an int at W = 2^31 - 1
inline long long tiles_across(int n) { return ((long long)n + T - 1) / T; }
inline long long tiles_of(int H, int W) { return tiles_across(H) * tiles_across(W); }

}  // namespace

// H W < 2^31 (api.hip), so the tile count fits an int; a negative result is "too large for an int64"
extern "C" long long nerf_amd_image_metrics_ws_bytes(long long M, int H, int W) {
    const long long per_image = tiles_of(H, W) * NPART * (long long)sizeof(double);
    if (M > 0x7fffffffffffffffll / per_image) return -2;
    return M * per_image;
}

extern "C" int nerf_amd_launch_image_metrics(const float* pred, long long pred_stride, const float* gt, long long gt_stride,
                                             double* sums, double* ssim, float* ssim_map, void* workspace, long long M, int H, int W,
                                             hipStream_t stream) {
    const int tiles_x = (int)tiles_across(W);
    const long long tiles = tiles_of(H, W);
    const bool want_ssim = ssim || ssim_map;
    double* ws = static_cast<double*>(workspace);
    // the per-image result rows are only written by the second launch when `ssim` is given; a map alone still needs pass 1
    const dim3 grid((unsigned)tiles, (unsigned)(M < 65535 ? M : 65535));
    (void)hipGetLastError();
    if (want_ssim)
        hipLaunchKernelGGL(image_metrics_tile_kernel<true>, grid, dim3(THREADS), 0, stream, pred, pred_stride, gt, gt_stride, ssim_map,
                           ws, M, H, W, tiles_x);
    else
        hipLaunchKernelGGL(image_metrics_tile_kernel<false>, grid, dim3(THREADS), 0, stream, pred, pred_stride, gt, gt_stride,
                           static_cast<float*>(nullptr), ws, M, H, W, tiles_x);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    const double positions = want_ssim ? (double)(H - HALO) * (double)(W - HALO) : 1.0;
    hipLaunchKernelGGL(image_metrics_reduce_kernel, dim3((unsigned)(M < 0x7fffffffll ? M : 0x7fffffffll)), dim3(THREADS), 0, stream,
                       ws, sums, ssim, M, tiles, positions);
    return (int)hipGetLastError();
}
