// occ_grid_device.h -- the occupancy grid as a kernel sees it, the test of one point against it and the mark of one ray
// (mark_ray), shared by the mark kernel (occupancy.hip) and the masked guided sampler (guided_masked.hip); and where a ray's
// live count goes for the scan that follows a mark (nerf_amd_launch_occ_scan, occupancy.hip).  Layout of the bits:
// include/nerf_amd.h.
#pragma once
#include "nerf_device.h"

struct OccGrid {
    const unsigned* bits;
    int cells[3];                              // cells per axis
    long long wz;                              // words per z row
    float lo[3], inv_step[3];
    int outside_live;
};

// the grid of R = (nx, ny, nz) grid points as the kernels take it (host)
inline OccGrid occ_grid_args(const unsigned* bits, long long nx, long long ny, long long nz, const float* h_lo,
                             const float* h_inv_step, int outside_live) {
    OccGrid g;
    g.bits = bits;
    g.cells[0] = (int)(nx - 1); g.cells[1] = (int)(ny - 1); g.cells[2] = (int)(nz - 1);
    g.wz = (nz - 1 + 31) >> 5;
    for (int a = 0; a < 3; ++a) { g.lo[a] = h_lo[a]; g.inv_step[a] = h_inv_step[a]; }
    g.outside_live = outside_live;
    return g;
}

// the rays' live counts, int[B]: the head of the mark workspace (nerf_amd_occ_workspace_bytes), where the scan reads them
inline int* occ_ws_counts(void* ws) { return reinterpret_cast<int*>(ws); }

__device__ __forceinline__ bool sample_live(const OccGrid& g, float x, float y, float z) {
    const float v[3] = {x, y, z};
    long long c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float f = floorf(mul_rn(sub_rn(v[a], g.lo[a]), g.inv_step[a]));
        if (!(f >= 0.f && f < (float)g.cells[a])) return g.outside_live != 0;       // also NaN
        c[a] = (long long)f;
    }
    const unsigned word = g.bits[(c[0] * g.cells[1] + c[1]) * g.wz + (c[2] >> 5)];
    return (word >> (c[2] & 31)) & 1u;
}

// One wavefront, one ray: the mark of its M samples.  point_of(i) is sample i's point (anything with x, y, z); its cell's
// bit, one ballot per 64 samples -> mask_row[ceil(M / 64)], and the ray's live count -> *count_out.
template <class PointOf>
__device__ __forceinline__ void mark_ray(const OccGrid& g, int M, int lane, PointOf point_of, unsigned long long* mask_row,
                                         int* count_out) {
    const int words = (M + 63) >> 6;
    int cnt = 0;
    for (int q = 0; q < words; ++q) {
        const int i = q * 64 + lane;
        bool live = false;
        if (i < M) {
            const auto pt = point_of(i);
            live = sample_live(g, pt.x, pt.y, pt.z);
        }
        const unsigned long long m = __ballot(live);
        if (lane == 0) mask_row[q] = m;
        cnt += __popcll(m);
    }
    if (lane == 0) *count_out = cnt;
}
