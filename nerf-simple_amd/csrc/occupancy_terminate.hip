// occupancy_terminate.hip -- early ray termination for the masked render (include/nerf_amd.h, "terminated render";
// DESIGN.md section 16).  Not in the reference.
//
// A ray's N samples are walked in slabs of S in {16, 32, 64} sample indices; between two slabs this source decides, from the
// transmittance over the rows evaluated so far, whether the next slab of the ray is evaluated at all.  One call of
// nerf_amd_termination_advance, for the slab [s0, s1) just evaluated and the next slab [s1, s2):
//   term_advance_kernel -- one wavefront per ray, four rays per block (occ_composite_kernel's shape), one sample of the
//       64-chunk of sample s1 - 1 per lane:
//         retire:  the slab's rows of the network's output go to their places in raw0, the M0 layout the masked compositor
//                  reads (a row never written stays the caller's (0, 0, 0, -inf): a dead sample);
//         T:       the transmittance entering sample s1 = carry of the earlier chunks x the compositor's own product scan
//                  (composite_device.h: wave_scan_mul) over the chunk's factors below s1.  Lane l of the inclusive scan
//                  depends on lanes <= l only, so lane s1 - chunk - 1 holds, bit for bit, what composite_ray will form
//                  as the exclusive product of lane s1 - chunk when it composites raw0; the carry of a completed chunk is
//                  the compositor's carry.  A retired row is taken from raw_slab itself, so no lane reads what another
//                  lane of this launch wrote;
//         select:  alive = !(T < eps) (a NaN T is alive), mask_next = M0 & [s1, s2) & alive, the ray's count and what it
//                  still has beyond s1.
//   term_block_sum_kernel / term_offsets_kernel -- exclusive scan of the counts into offsets_next[B + 1] and the two totals.
// Fixed partitions, hand-written scans, no atomics: two runs write the same bytes.  The host wrapper below is the C ABI
// itself (argument rules: api_checks.h).
#include "composite_device.h"
#include "occ_scan_device.h"
#include "api_checks.h"

namespace {

constexpr int TERM_SCAN_THREADS = 256;
constexpr int TERM_SCAN_PER_THREAD = 8;
constexpr long long TERM_SCAN_ITEMS = (long long)TERM_SCAN_THREADS * TERM_SCAN_PER_THREAD;      // rays per scan block

struct TermArgs {
    const f32x4* raw_slab;                     // [rows_slab]: the network on the slab's compacted points, or NULL
    const unsigned long long* mask_slab;       // [B, W]: the mask that compacted them (an earlier mask_next)
    const long long* offsets_slab;             // [B + 1]
    long long rows_slab;
    const unsigned long long* mask0;           // [B, W]: the occupancy mask M0
    const long long* offsets0;                 // [B + 1]
    f32x4* raw0;                               // [rows0]: M0 layout
    long long rows0;
    float eps;
    int S, s0, s1, s2;
    float* trans;                              // [B, K]
    float* carry;                              // [B]: transmittance entering the 64-chunk under way
    unsigned long long* mask_next;             // [B, W]
    int* cnt;                                  // [B]: set bits of mask_next
    int* rem;                                  // [B]: M0 bits at or beyond s1 of a ray still alive
};

__global__ __launch_bounds__(MASKED_THREADS) void term_advance_kernel(MlpArgs a, TermArgs t, long long B) {
    const long long ray = (long long)blockIdx.x * MASKED_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= B) return;                      // whole wave leaves together; no workgroup barrier below
    const int lane = threadIdx.x & 63;
    const int N = a.N, W = (N + 63) >> 6, K = (N + t.S - 1) / t.S;
    const unsigned long long* m0 = t.mask0 + ray * W;
    float T = 1.0f;
    if (t.s1 == 0) {
        if (lane == 0) t.carry[ray] = 1.0f;
    } else {
        const int q = (t.s1 - 1) >> 6, cb = q << 6;        // the chunk of the last retired sample
        const int i = cb + lane;
        long long before = 0;
        for (int p = 0; p < q; ++p) before += __popcll(m0[p]);
        const unsigned long long mw = m0[q], below = (1ull << lane) - 1ull;
        const long long row0 = t.offsets0[ray] + before + __popcll(mw & below);
        f32x4 c = {0.f, 0.f, 0.f, -__builtin_inff()};
        if (((mw >> lane) & 1ull) && i < t.s1 && row0 >= 0 && row0 < min_ll(t.offsets0[ray + 1], t.rows0)) {
            bool retired = false;
            if (t.raw_slab && i >= t.s0) {
                const unsigned long long ms = t.mask_slab[ray * W + q];
                const long long src = t.offsets_slab[ray] + __popcll(ms & below);
                if (((ms >> lane) & 1ull) && src >= 0 && src < min_ll(t.offsets_slab[ray + 1], t.rows_slab)) {
                    c = t.raw_slab[src];
                    t.raw0[row0] = c;
                    retired = true;
                }
            }
            if (!retired) c = t.raw0[row0];    // an earlier slab's row, or the caller's (0, 0, 0, -inf)
        }
        // positions as the masked compositor recomputes them; lane l needs t(i) and t(i + 1) for i < s1
        float tc = 0.f;
        if (i < N && i <= t.s1) tc = fetch_point_rays<false>(a, ray * N + i, RaySample{ray, i}).t;
        float tn = __shfl_down(tc, 1);
        if (lane == 63 && i + 1 < N && i < t.s1) tn = fetch_point_rays<false>(a, ray * N + i + 1, RaySample{ray, i + 1}).t;
        const float dnorm = ray_dnorm(a, ray);
        float fac = 1.0f;      // composite_ray's factor of sample i: the routine it calls (composite_device.h)
        if (i < t.s1) fac = nerf_composite::alpha_factor((i == N - 1) ? 1e10f : sub_rn(tn, tc), dnorm, c[3]).fac;
        const float incl = nerf_composite::wave_scan_mul(fac);
        const float upto = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(incl), t.s1 - cb - 1));
        T = mul_rn(t.carry[ray], upto);
        if (t.s1 - cb == 64 && lane == 0) t.carry[ray] = T;          // the chunk is complete: the compositor's carry
        // termination is permanent: a terminated ray evaluates nothing more, and its T is frozen rather than re-formed (the
        // scan's product tree is not associative to the last bit, so a re-formed T could differ from T_k in an ulp)
        if (t.s1 < N) {
            const float prev = t.trans[ray * K + t.s1 / t.S - 1];
            if (prev < t.eps) T = prev;
        }
    }
    unsigned long long sel = 0;
    int remaining = 0;
    const int q1 = t.s1 >> 6;
    if (t.s1 < N) {
        const bool alive = !(T < t.eps);       // NaN stays alive: termination never hides a NaN
        if (lane == 0) t.trans[ray * K + t.s1 / t.S] = T;
        if (alive) {
            const int n = t.s2 - t.s1, sh = t.s1 & 63;
            const unsigned long long range = (n >= 64 ? ~0ull : ((1ull << n) - 1ull)) << sh;
            sel = m0[q1] & range;
            remaining = __popcll(m0[q1] & (~0ull << sh));
            for (int p = q1 + 1; p < W; ++p) remaining += __popcll(m0[p]);
        }
    }
    if (lane < W) t.mask_next[ray * W + lane] = lane == q1 ? sel : 0ull;
    if (lane == 0) {
        t.cnt[ray] = __popcll(sel);
        t.rem[ray] = remaining;
    }
}

// ---- scan ----------------------------------------------------------------------------------------------------------------
// blk[2 b], blk[2 b + 1]: the sums of cnt / rem over scan block b
__global__ __launch_bounds__(TERM_SCAN_THREADS) void term_block_sum_kernel(const int* __restrict__ cnt, const int* __restrict__ rem,
                                                                           long long B, long long* __restrict__ blk) {
    __shared__ long long lds_waves[TERM_SCAN_THREADS / 64];
    const long long base = (long long)blockIdx.x * TERM_SCAN_ITEMS + (long long)threadIdx.x * TERM_SCAN_PER_THREAD;
    long long s = 0, r = 0;
    for (int k = 0; k < TERM_SCAN_PER_THREAD; ++k)
        if (base + k < B) { s += cnt[base + k]; r += rem[base + k]; }
    long long ts, tr;
    (void)block_exclusive_scan<TERM_SCAN_THREADS>(s, ts, lds_waves);
    (void)block_exclusive_scan<TERM_SCAN_THREADS>(r, tr, lds_waves);
    if (threadIdx.x == 0) { blk[2 * (long long)blockIdx.x] = ts; blk[2 * (long long)blockIdx.x + 1] = tr; }
}

// offsets[ray] = (sum of the blocks before this one) + (scan inside the block); the last block also writes offsets[B] and
// totals[0] = the next slab's live count, totals[1] = the live samples left beyond s1 on rays still alive
__global__ __launch_bounds__(TERM_SCAN_THREADS) void term_offsets_kernel(const int* __restrict__ cnt, long long B,
                                                                         const long long* __restrict__ blk, long long nblk,
                                                                         long long* __restrict__ offsets,
                                                                         long long* __restrict__ totals) {
    __shared__ long long lds_waves[TERM_SCAN_THREADS / 64];
    const bool last = blockIdx.x == nblk - 1;
    long long p = 0, r = 0;
    for (long long b = threadIdx.x; b < nblk; b += TERM_SCAN_THREADS) {
        if (b < blockIdx.x) p += blk[2 * b];
        if (last) r += blk[2 * b + 1];
    }
    long long prefix, rem_total;
    (void)block_exclusive_scan<TERM_SCAN_THREADS>(p, prefix, lds_waves);
    (void)block_exclusive_scan<TERM_SCAN_THREADS>(r, rem_total, lds_waves);
    const long long base = (long long)blockIdx.x * TERM_SCAN_ITEMS + (long long)threadIdx.x * TERM_SCAN_PER_THREAD;
    int c[TERM_SCAN_PER_THREAD];
    long long s = 0;
    for (int k = 0; k < TERM_SCAN_PER_THREAD; ++k) {
        c[k] = base + k < B ? cnt[base + k] : 0;
        s += c[k];
    }
    long long total;
    long long o = prefix + block_exclusive_scan<TERM_SCAN_THREADS>(s, total, lds_waves);
    for (int k = 0; k < TERM_SCAN_PER_THREAD; ++k) {
        if (base + k < B) offsets[base + k] = o;
        o += c[k];
    }
    if (last && threadIdx.x == 0) {
        offsets[B] = prefix + total;
        totals[0] = prefix + total;
        totals[1] = rem_total;
    }
}

struct TermWs {
    long long nblk, off_cnt, off_rem, off_blk, bytes;      // the carries are the first B floats
};
TermWs term_ws(long long B) {
    constexpr auto up = align256;
    TermWs w;
    w.nblk = (B + TERM_SCAN_ITEMS - 1) / TERM_SCAN_ITEMS;
    w.off_cnt = up(B * 4);
    w.off_rem = w.off_cnt + up(B * 4);
    w.off_blk = w.off_rem + up(B * 4);
    w.bytes = w.off_blk + up(w.nblk * 16);
    return w;
}

}  // namespace

extern "C" int64_t nerf_amd_termination_workspace_bytes(int64_t B) {
    if (B < 0) return NERF_AMD_EINVAL;
    if (B > MASKED_MAX_RAYS) return NERF_AMD_EUNSUP;
    return term_ws(B).bytes;
}

extern "C" int nerf_amd_termination_advance(const float* raw_slab, const uint64_t* mask_slab, const int64_t* offsets_slab,
                                            int64_t rows_slab, const float* rays, const float* u, const float* tbins,
                                            uint32_t flags, uint64_t seed, int64_t ray_id0, const uint64_t* mask0,
                                            const int64_t* offsets0, float* raw0, int64_t rows0, float eps, int slab, int s0,
                                            int s1, int s2, float* trans, uint64_t* mask_next, int64_t* offsets_next,
                                            int64_t* totals, void* workspace, int64_t B, int N, void* stream) {
    if (rows_slab < 0 || rows0 < 0) return NERF_AMD_EINVAL;
    if (!(eps > 0.0f && eps < 1.0f)) return NERF_AMD_EINVAL;                    // also NaN
    if (slab != 16 && slab != 32 && slab != 64) return NERF_AMD_EINVAL;
    // the rays and jitter rules of the other masked stages; N: the mask layout's and the masked compositor's limit
    const int rc = masked_rays_check(rays, u, tbins, flags, B, N, N > MASKED_MAX_N);
    if (rc) return rc;
    // the slabs: (0, 0, min(S, N)) at first, then (k S, min((k + 1) S, N), min((k + 2) S, N))
    auto clip = [N](int64_t x) { return (int)(x < N ? x : N); };
    if (s0 < 0 || s0 > s1 || s1 > s2 || s2 > N || s0 % slab != 0) return NERF_AMD_EINVAL;
    if (s1 != clip((int64_t)s0 + slab) && !(s0 == 0 && s1 == 0)) return NERF_AMD_EINVAL;
    if (s2 != clip((int64_t)s1 + slab)) return NERF_AMD_EINVAL;
    if (raw_slab) {
        if (s0 == s1 || !mask_slab || !offsets_slab || misaligned(raw_slab, 16) || misaligned(mask_slab, 8) ||
            misaligned(offsets_slab, 8))
            return NERF_AMD_EINVAL;
        if (mask_slab == mask_next || offsets_slab == offsets_next) return NERF_AMD_EINVAL;      // the scan is not in place
    } else if (rows_slab != 0) {
        return NERF_AMD_EINVAL;
    }
    if (!mask0 || !offsets0 || !trans || !mask_next || !offsets_next || !totals || !workspace || (rows0 > 0 && !raw0))
        return NERF_AMD_EINVAL;
    if (misaligned(mask0, 8) || misaligned(offsets0, 8) || misaligned(raw0, 16) || misaligned(trans, 4) ||
        misaligned(mask_next, 8) || misaligned(offsets_next, 8) || misaligned(totals, 8) ||
        misaligned(workspace, 16))
        return NERF_AMD_EINVAL;
    if (B == 0) return 0;
    (void)hipGetLastError();
    const MlpArgs a = rays_args(rays, u, tbins, flags, seed, ray_id0, B, N);
    const TermWs w = term_ws(B);
    char* b = reinterpret_cast<char*>(workspace);
    TermArgs t;
    t.raw_slab = reinterpret_cast<const f32x4*>(raw_slab);
    t.mask_slab = reinterpret_cast<const unsigned long long*>(mask_slab);
    t.offsets_slab = reinterpret_cast<const long long*>(offsets_slab);
    t.rows_slab = rows_slab;
    t.mask0 = reinterpret_cast<const unsigned long long*>(mask0);
    t.offsets0 = reinterpret_cast<const long long*>(offsets0);
    t.raw0 = reinterpret_cast<f32x4*>(raw0);
    t.rows0 = rows0;
    t.eps = eps; t.S = slab; t.s0 = s0; t.s1 = s1; t.s2 = s2;
    t.trans = trans;
    t.carry = reinterpret_cast<float*>(b);
    t.mask_next = reinterpret_cast<unsigned long long*>(mask_next);
    t.cnt = reinterpret_cast<int*>(b + w.off_cnt);
    t.rem = reinterpret_cast<int*>(b + w.off_rem);
    long long* blk = reinterpret_cast<long long*>(b + w.off_blk);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long blocks = (B + MASKED_RAYS_PER_BLOCK - 1) / MASKED_RAYS_PER_BLOCK;
    hipLaunchKernelGGL(term_advance_kernel, dim3((unsigned)blocks), dim3(MASKED_THREADS), 0, s, a, t, (long long)B);
    hipLaunchKernelGGL(term_block_sum_kernel, dim3((unsigned)w.nblk), dim3(TERM_SCAN_THREADS), 0, s, (const int*)t.cnt,
                       (const int*)t.rem, (long long)B, blk);
    hipLaunchKernelGGL(term_offsets_kernel, dim3((unsigned)w.nblk), dim3(TERM_SCAN_THREADS), 0, s, (const int*)t.cnt, (long long)B,
                       (const long long*)blk, w.nblk, reinterpret_cast<long long*>(offsets_next),
                       reinterpret_cast<long long*>(totals));
    return (int)hipGetLastError();
}
