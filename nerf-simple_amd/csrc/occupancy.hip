// occupancy.hip -- empty-space skipping for the inference render: an occupancy grid and the masked render path around
// the existing points-mode forward.  Not in the reference.
//
// Grid: R = (nx, ny, nz) grid points per axis (the axes of a density grid, density.hip) make C = R - 1 cells per axis; cell
// (i, j, k) spans points i .. i + 1 etc.  One bit per cell, packed z fastest: word (i Cy + j) Wz + (k >> 5), bit k & 31,
// Wz = ceil(Cz / 32); the padding bits of a row's last word are zero (include/nerf_amd.h).
//   bits:   occ_bits_kernel   -- sigma volume -> bits.  A cell is dead iff every corner of every cell within `dilate` cells
//                                of it (Chebyshev, clipped at the grid's edge) has sigma <= level, i.e. it is live iff a
//                                grid point in [i - d, i + d + 1] x [j - d, j + d + 1] x [k - d, k + d + 1] (clipped) is hot,
//                                hot = !(sigma <= level) (NaN is hot).  One wavefront per output word.
//           occ_pack_kernel   -- a caller's byte-per-cell mask -> bits.
//   mark:   occ_mark_kernel   -- one wavefront per ray: the N sample points as every render forms them (fetch_point_rays),
//                                the cell of each (fp32, separately rounded: floor(fl(fl(x - lo) inv_step))), its bit, one
//                                ballot per 64 samples -> mask[B, ceil(N / 64)] and the ray's live count.
//   scan:   occ_block_sum_kernel / occ_scan_blocks_kernel / occ_offsets_kernel -- exclusive scan of the counts into
//                                offsets[B + 1] (int64); offsets[B] = the live count P'.
//   emit:   occ_emit_kernel   -- the query points of the live samples, compacted ray-major (rows of nerf_amd_query_points).
//   render: occ_composite_kernel -- composite_ray (composite_device.h, unchanged) over ALL N samples of a ray: positions
//                                recomputed into the wave's LDS slice, the network's output read at offsets[ray] + rank
//                                for a live sample and (0, 0, 0, -inf) for a dead one, which contributes exactly nothing.
// Fixed partitions and hand-written scans, no atomics: every run writes the same bytes.
#include "composite_device.h"
#include "launchers.h"
#include "occ_grid_device.h"
#include "occ_scan_device.h"

namespace {

constexpr int OCC_MAX_N = nerf_layout::MASKED_MAX_N;      // samples per ray (the fused render's own limit, nerf_layout.h)
constexpr int OCC_MAX_DILATE = 15;             // 33 + 2 d grid points along z feed one word: one per lane
constexpr int OCC_SCAN_THREADS = 256;
constexpr int OCC_SCAN_PER_THREAD = 8;
constexpr long long OCC_SCAN_ITEMS = (long long)OCC_SCAN_THREADS * OCC_SCAN_PER_THREAD;      // rays per scan block
constexpr int OCC_TOP_THREADS = 1024;

// ---- bits from sigma ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void occ_bits_kernel(const float* __restrict__ sigma, long long nx, long long ny, long long nz,
                                                       float level, int d, unsigned* __restrict__ bits, long long n_words) {
    const int lane = threadIdx.x & 63;
    const long long cy = ny - 1, cz = nz - 1, wz = (cz + 31) >> 5;
    for (long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); wid < n_words; wid += (long long)gridDim.x * 4) {
        const long long w = wid % wz, r = wid / wz, j = r % cy, i = r / cy;
        // lane l looks at the column of grid points z = 32 w - d + l: hot iff any point of the (p, q) window is
        const long long z = w * 32 - d + lane;
        bool hot = false;
        if (lane < 33 + 2 * d && z >= 0 && z < nz) {
            const long long p0 = i - d > 0 ? i - d : 0, p1 = i + d + 1 < nx - 1 ? i + d + 1 : nx - 1;
            const long long q0 = j - d > 0 ? j - d : 0, q1 = j + d + 1 < ny - 1 ? j + d + 1 : ny - 1;
            for (long long p = p0; p <= p1; ++p)
                for (long long q = q0; q <= q1; ++q) hot |= !(sigma[(p * ny + q) * nz + z] <= level);
        }
        const unsigned long long H = __ballot(hot);
        // cell k = 32 w + c reads points k - d .. k + d + 1 = lanes c .. c + 2 d + 1
        unsigned word = 0;
        for (int s = 0; s <= 2 * d + 1; ++s) word |= (unsigned)(H >> s);
        const long long rem = cz - w * 32;
        if (rem < 32) word &= (1u << rem) - 1u;
        if (lane == 0) bits[wid] = word;
    }
}

__global__ __launch_bounds__(256) void occ_pack_kernel(const unsigned char* __restrict__ cells, long long cz, long long wz,
                                                       unsigned* __restrict__ bits, long long n_words) {
    for (long long wid = (long long)blockIdx.x * 256 + threadIdx.x; wid < n_words; wid += (long long)gridDim.x * 256) {
        const long long w = wid % wz, row = wid / wz;
        const unsigned char* c = cells + row * cz + w * 32;
        const int n = cz - w * 32 < 32 ? (int)(cz - w * 32) : 32;
        unsigned word = 0;
        for (int b = 0; b < n; ++b) word |= (c[b] ? 1u : 0u) << b;
        bits[wid] = word;
    }
}

// ---- mark ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MASKED_THREADS) void occ_mark_kernel(MlpArgs a, OccGrid g, unsigned long long* __restrict__ mask,
                                                                  int* __restrict__ counts, long long B) {
    const long long ray = (long long)blockIdx.x * MASKED_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= B) return;                      // whole wave leaves together
    mark_ray(g, a.N, threadIdx.x & 63, [&](int i) { return fetch_point_rays<false>(a, ray * a.N + i, RaySample{ray, i}); },
             mask + ray * ((a.N + 63) >> 6), counts + ray);
}

// ---- scan ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OCC_SCAN_THREADS) void occ_block_sum_kernel(const int* __restrict__ counts, long long B,
                                                                         long long* __restrict__ blk) {
    __shared__ long long lds_waves[OCC_SCAN_THREADS / 64];
    const long long base = (long long)blockIdx.x * OCC_SCAN_ITEMS + (long long)threadIdx.x * OCC_SCAN_PER_THREAD;
    long long s = 0;
    for (int r = 0; r < OCC_SCAN_PER_THREAD; ++r)
        if (base + r < B) s += counts[base + r];
    long long total;
    (void)block_exclusive_scan<OCC_SCAN_THREADS>(s, total, lds_waves);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the block sums; the total goes to offsets[B] and to *live
__global__ __launch_bounds__(OCC_TOP_THREADS) void occ_scan_blocks_kernel(const long long* __restrict__ blk, long long nblk,
                                                                          long long* __restrict__ blkoff,
                                                                          long long* __restrict__ offsets_end,
                                                                          long long* __restrict__ live) {
    __shared__ long long lds[OCC_TOP_THREADS];
    const long long per = (nblk + OCC_TOP_THREADS - 1) / OCC_TOP_THREADS;
    const long long b0 = (long long)threadIdx.x * per;
    const long long b1 = b0 + per < nblk ? b0 + per : nblk;
    long long s = 0;
    for (long long b = b0; b < b1; ++b) s += blk[b];
    lds[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < OCC_TOP_THREADS; d <<= 1) {          // Hillis-Steele inclusive scan over the run sums
        const long long add = threadIdx.x >= (unsigned)d ? lds[threadIdx.x - d] : 0;
        __syncthreads();
        lds[threadIdx.x] += add;
        __syncthreads();
    }
    long long p = lds[threadIdx.x] - s;
    for (long long b = b0; b < b1; ++b) {
        blkoff[b] = p;
        p += blk[b];
    }
    if (threadIdx.x == OCC_TOP_THREADS - 1) {
        *offsets_end = lds[threadIdx.x];
        if (live) *live = lds[threadIdx.x];
    }
}

__global__ __launch_bounds__(OCC_SCAN_THREADS) void occ_offsets_kernel(const int* __restrict__ counts, long long B,
                                                                       const long long* __restrict__ blkoff,
                                                                       long long* __restrict__ offsets) {
    __shared__ long long lds_waves[OCC_SCAN_THREADS / 64];
    const long long base = (long long)blockIdx.x * OCC_SCAN_ITEMS + (long long)threadIdx.x * OCC_SCAN_PER_THREAD;
    int c[OCC_SCAN_PER_THREAD];
    long long s = 0;
    for (int r = 0; r < OCC_SCAN_PER_THREAD; ++r) {
        c[r] = base + r < B ? counts[base + r] : 0;
        s += c[r];
    }
    long long total;
    long long p = blkoff[blockIdx.x] + block_exclusive_scan<OCC_SCAN_THREADS>(s, total, lds_waves);
    for (int r = 0; r < OCC_SCAN_PER_THREAD; ++r) {
        if (base + r < B) offsets[base + r] = p;
        p += c[r];
    }
}

// ---- emit ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MASKED_THREADS) void occ_emit_kernel(MlpArgs a, const unsigned long long* __restrict__ mask,
                                                                           const long long* __restrict__ offsets,
                                                                           float* __restrict__ pts, long long max_points,
                                                                           long long B) {
    const long long ray = (long long)blockIdx.x * MASKED_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= B) return;
    const int lane = threadIdx.x & 63;
    const long long first = offsets[ray];
    if (offsets[ray + 1] == first) return;     // nothing live on this ray
    // never past the capacity the caller states
    emit_ray_rows(a, mask + ray * ((a.N + 63) >> 6), pts, first, max_points, ray, lane);
}

// ---- masked composite ----------------------------------------------------------------------------------------------------
struct MaskedSamples {
    const float* ts;                           // the ray's N positions (LDS)
    const unsigned long long* m;               // the ray's mask words
    const f32x4* raw;                          // the network's output for the ray's first live sample
    long long n_live;                          // live samples of this ray
    __device__ __forceinline__ float t(int i) const { return ts[i]; }
    __device__ __forceinline__ f32x4 c(int i) const {
        const int w = i >> 6, b = i & 63;
        long long rank = 0;
        for (int q = 0; q < w; ++q) rank += __popcll(m[q]);
        const unsigned long long mw = m[w];
        rank += __popcll(mw & ((1ull << b) - 1ull));
        if (((mw >> b) & 1ull) && rank < n_live) return raw[rank];
        return f32x4{0.f, 0.f, 0.f, -__builtin_inff()};     // softplus(-inf) = 0: alpha = 0, transmittance factor 1, w = 0
    }
};

__global__ __launch_bounds__(MASKED_THREADS) void occ_composite_kernel(MlpArgs a, const unsigned long long* __restrict__ mask,
                                                                                const long long* __restrict__ offsets,
                                                                                const float* __restrict__ raw,
                                                                                nerf_composite::RayOut o, long long B) {
    __shared__ float s_t[MASKED_RAYS_PER_BLOCK][OCC_MAX_N];
    const int wv = threadIdx.x >> 6;
    const long long ray = (long long)blockIdx.x * MASKED_RAYS_PER_BLOCK + wv;
    if (ray >= B) return;                      // whole wave leaves together; no workgroup barrier below
    const int lane = threadIdx.x & 63;
    const int N = a.N;
    fill_ray_positions(a, ray, lane, s_t[wv]);
    const float dnorm = ray_dnorm(a, ray);
    const long long first = offsets[ray];
    const MaskedSamples src{s_t[wv], mask + ray * ((N + 63) >> 6), reinterpret_cast<const f32x4*>(raw) + first,
                            offsets[ray + 1] - first};
    nerf_composite::composite_ray(src, N, lane, dnorm, ray, o);
}

inline unsigned capped_blocks(long long blocks) { return (unsigned)(blocks < 65536 * 16 ? (blocks > 0 ? blocks : 1) : 65536 * 16); }

struct OccWs {
    long long nblk, off_counts, off_blk, off_blkoff, bytes;
};
OccWs occ_ws(long long B) {
    constexpr auto up = nerf_layout::align256;
    OccWs w;
    w.nblk = (B + OCC_SCAN_ITEMS - 1) / OCC_SCAN_ITEMS;
    w.off_counts = 0;                          // occ_ws_counts (occ_grid_device.h)
    w.off_blk = up(B * 4);
    w.off_blkoff = w.off_blk + up(w.nblk * 8);
    w.bytes = w.off_blkoff + up(w.nblk * 8);
    return w;
}

}  // namespace

extern "C" int nerf_amd_occ_max_n(void) { return OCC_MAX_N; }
extern "C" int nerf_amd_occ_max_dilate(void) { return OCC_MAX_DILATE; }
extern "C" long long nerf_amd_occ_workspace_bytes(long long B) { return occ_ws(B).bytes; }

extern "C" int nerf_amd_launch_occ_bits(const float* sigma, long long nx, long long ny, long long nz, float level, int dilate,
                                        unsigned* bits, hipStream_t stream) {
    (void)hipGetLastError();
    const long long n_words = (nx - 1) * (ny - 1) * ((nz - 1 + 31) >> 5);
    hipLaunchKernelGGL(occ_bits_kernel, dim3(capped_blocks((n_words + 3) / 4)), dim3(256), 0, stream, sigma, nx, ny, nz, level,
                       dilate, bits, n_words);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_occ_pack(const unsigned char* cells, long long cx, long long cy, long long cz, unsigned* bits,
                                        hipStream_t stream) {
    (void)hipGetLastError();
    const long long wz = (cz + 31) >> 5, n_words = cx * cy * wz;
    hipLaunchKernelGGL(occ_pack_kernel, dim3(capped_blocks((n_words + 255) / 256)), dim3(256), 0, stream, cells, cz, wz, bits,
                       n_words);
    return (int)hipGetLastError();
}

// the exclusive scan of the rays' live counts (int[B] at the head of `ws`, occ_ws_counts) into offsets[B + 1]; the total goes
// to offsets[B] and, when given, to *live.  Enqueued behind the kernel that wrote the counts: the mark below, or the masked
// guided sampler (guided_masked.hip).
extern "C" int nerf_amd_launch_occ_scan(void* ws, long long* offsets, long long* live, long long B, hipStream_t stream) {
    const OccWs w = occ_ws(B);
    char* b = reinterpret_cast<char*>(ws);
    int* counts = reinterpret_cast<int*>(b + w.off_counts);
    long long* blk = reinterpret_cast<long long*>(b + w.off_blk);
    long long* blkoff = reinterpret_cast<long long*>(b + w.off_blkoff);
    if (B > 0)
        hipLaunchKernelGGL(occ_block_sum_kernel, dim3((unsigned)w.nblk), dim3(OCC_SCAN_THREADS), 0, stream, (const int*)counts, B,
                           blk);
    hipLaunchKernelGGL(occ_scan_blocks_kernel, dim3(1), dim3(OCC_TOP_THREADS), 0, stream, (const long long*)blk, w.nblk, blkoff,
                       offsets + B, live);
    if (B > 0)
        hipLaunchKernelGGL(occ_offsets_kernel, dim3((unsigned)w.nblk), dim3(OCC_SCAN_THREADS), 0, stream, (const int*)counts, B,
                           (const long long*)blkoff, offsets);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_occ_mark(const MlpArgs* args, const unsigned* bits, long long nx, long long ny, long long nz,
                                        const float* h_lo, const float* h_inv_step, int outside_live, unsigned long long* mask,
                                        long long* offsets, long long* live, void* ws, long long B, hipStream_t stream) {
    (void)hipGetLastError();
    const OccGrid g = occ_grid_args(bits, nx, ny, nz, h_lo, h_inv_step, outside_live);
    if (B > 0) {
        const long long blocks = (B + MASKED_RAYS_PER_BLOCK - 1) / MASKED_RAYS_PER_BLOCK;
        hipLaunchKernelGGL(occ_mark_kernel, dim3((unsigned)blocks), dim3(MASKED_THREADS), 0, stream, *args, g, mask,
                           occ_ws_counts(ws), B);
    }
    return nerf_amd_launch_occ_scan(ws, offsets, live, B, stream);
}

extern "C" int nerf_amd_launch_occ_emit(const MlpArgs* args, const unsigned long long* mask, const long long* offsets, float* pts,
                                        long long max_points, long long B, hipStream_t stream) {
    (void)hipGetLastError();
    if (B == 0) return 0;
    const long long blocks = (B + MASKED_RAYS_PER_BLOCK - 1) / MASKED_RAYS_PER_BLOCK;
    hipLaunchKernelGGL(occ_emit_kernel, dim3((unsigned)blocks), dim3(MASKED_THREADS), 0, stream, *args, mask, offsets, pts,
                       max_points, B);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_occ_composite(const MlpArgs* args, const unsigned long long* mask, const long long* offsets,
                                             const float* raw, long long B, hipStream_t stream) {
    (void)hipGetLastError();
    if (B == 0) return 0;
    const long long blocks = (B + MASKED_RAYS_PER_BLOCK - 1) / MASKED_RAYS_PER_BLOCK;
    const nerf_composite::RayOut o{args->rgb, args->disp, args->alpha, args->acc, args->w, args->pixels};
    hipLaunchKernelGGL(occ_composite_kernel, dim3((unsigned)blocks), dim3(MASKED_THREADS), 0, stream, *args, mask, offsets,
                       raw, o, B);
    return (int)hipGetLastError();
}
