// occ_scan_device.h -- the device pieces the occupancy sources share: the workgroup exclusive scan behind every offsets[]
// array (occupancy.hip, occupancy_terminate.hip), the per-ray body of the emit kernels (occupancy.hip, occupancy_graph.hip)
// and the per-ray prologue of the masked kernels (one wavefront per ray, nerf_layout::MASKED_RAYS_PER_BLOCK rays per block):
// the ray's positions into an LDS slice, its dnorm, and the min the clamps are formed with.  Fixed order, no atomics: every
// run writes the same bytes.
#pragma once
#include "composite_device.h"

using nerf_layout::MASKED_RAYS_PER_BLOCK;
constexpr int MASKED_THREADS = 64 * MASKED_RAYS_PER_BLOCK;

__device__ __forceinline__ long long min_ll(long long a, long long b) { return a < b ? a : b; }

// the ray's N positions, as every render forms them, into ts[] (the wave's own LDS slice), fenced for the wave's reads
__device__ __forceinline__ void fill_ray_positions(const MlpArgs& a, long long ray, int lane, float* ts) {
    for (int i = lane; i < a.N; i += 64) ts[i] = fetch_point_rays<false>(a, ray * a.N + i, RaySample{ray, i}).t;
    wave_lds_fence();
}

// the norm of the ray's unit direction, the compositor's scale of every interval
__device__ __forceinline__ float ray_dnorm(const MlpArgs& a, long long ray) {
    const float* d = a.rays + ray * 6 + 3;
    return nerf_composite::unit_dir_norm(d[0], d[1], d[2], true);
}

// exclusive scan of one value per thread over a workgroup of THREADS threads, in thread order, and the block total.  The
// leading barrier makes a second call on the same lds_waves[THREADS / 64] safe: the slots may still be read from the first.
template <int THREADS>
__device__ __forceinline__ long long block_exclusive_scan(long long x, long long& total, long long* lds_waves) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
    }
    __syncthreads();
    if (lane == 63) lds_waves[wave] = incl;
    __syncthreads();
    long long before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
        const long long v = lds_waves[w];
        if (w < wave) before += v;
        total += v;
    }
    return before + incl - x;
}

// One wavefront, one ray: the query points of its set mask bits (rows of nerf_amd_query_points) go to rows first, first + 1,
// ... of pts[., 6] in sample order; a row outside [0, limit) is not written.
__device__ __forceinline__ void emit_ray_rows(const MlpArgs& a, const unsigned long long* mask_row, float* pts, long long first,
                                              long long limit, long long ray, int lane) {
    long long out = first;
    const int words = (a.N + 63) >> 6;
    for (int q = 0; q < words; ++q) {
        const unsigned long long m = mask_row[q];
        const int i = q * 64 + lane;
        if (((m >> lane) & 1ull) && i < a.N) {
            const long long row = out + __popcll(m & ((1ull << lane) - 1ull));
            if (row >= 0 && row < limit) {
                const PointIn pt = fetch_point_rays<true>(a, ray * a.N + i, RaySample{ray, i});
                float* o = pts + row * 6;
                o[0] = pt.x; o[1] = pt.y; o[2] = pt.z; o[3] = pt.d1; o[4] = pt.d2; o[5] = pt.d3;
            }
        }
        out += __popcll(m);
    }
}
