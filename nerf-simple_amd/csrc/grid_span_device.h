// grid_span_device.h -- a ray against the occupancy grid's cells: the interval between its first and its last live cell
// (include/nerf_amd.h, "grid span"; tests/grid_span_model.py restates it op for op).  Device code only,
// no kernel: grid_span.hip launches it, and a fused variant can include it.
// The ray is clipped to the grid's bounds by the scene box's slab routine (ray_box_device.h, not restated), the clipped
// interval [a, b] is cut into K segments, and a segment is live iff one of the 8 cells spanned by its two end points' cell
// indices has its bit set.  With K >= 2 max(cells per axis) a segment covers at most half a cell per axis, so every cell it
// crosses is among the 8: the interval [first live segment's start, last live segment's end] is conservative.
// Every operation is one IEEE fp32 operation with its own rounding, as in ray_box_device.h.  A cell index is CLAMPED into
// [0, C - 1] by comparisons that send a NaN to 0 before any address is formed: no ray reads outside `bits`.
#pragma once
#include "ray_box_device.h"
#include "occ_grid_device.h"

// floor(fl(fl(p - lo) * inv_step)) clamped into [0, C - 1]; NaN -> 0, anything at or beyond C - 1 (also +inf) -> C - 1
__device__ __forceinline__ int span_cell(float p, float lo, float inv_step, int C) {
    const float f = floorf(mul_rn(sub_rn(p, lo), inv_step));
    return f >= 1.0f ? (f < (float)(C - 1) ? (int)f : C - 1) : 0;
}

// edge j of the K segments of [a, b], len = fl(b - a): e_j = fl(a + fl(len * fl(j / K))); the ends are a and b themselves, so
// an all-live grid gives the grid's own box
__device__ __forceinline__ float span_edge(float a, float b, float len, int j, int K) {
    if (j <= 0) return a;
    if (j >= K) return b;
    return add_rn(a, mul_rn(len, __fdiv_rn((float)j, (float)K)));
}

// the cell indices of the ray's point at parameter e
__device__ __forceinline__ void span_cells_at(const OccGrid& g, const float* __restrict__ ray, float e, int c[3]) {
#pragma unroll
    for (int x = 0; x < 3; ++x) c[x] = span_cell(add_rn(ray[x], mul_rn(e, ray[3 + x])), g.lo[x], g.inv_step[x], g.cells[x]);
}

// is segment [e0, e1] live: any bit among the 8 cells (c0 | c1)_x x (c0 | c1)_y x (c0 | c1)_z
__device__ __forceinline__ bool span_segment_live(const OccGrid& g, const float* __restrict__ ray, float e0, float e1) {
    int c0[3], c1[3];
    span_cells_at(g, ray, e0, c0);
    span_cells_at(g, ray, e1, c1);
    unsigned any = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const long long cx = (k & 4) ? c1[0] : c0[0], cy = (k & 2) ? c1[1] : c0[1];
        const int cz = (k & 1) ? c1[2] : c0[2];
        any |= (g.bits[(cx * g.cells[1] + cy) * g.wz + (cz >> 5)] >> (cz & 31)) & 1u;
    }
    return any != 0;
}

// One wavefront, one ray: [t0, t1] and hit of the ray (o, d) = ray[0..5] against the grid, K = probes segments.  Lane l of
// chunk q owns segment 64 q + l and recomputes both of its edges; one ballot per chunk.  The chunks are searched upward for
// the first live segment and downward for the last, and the ones between are not looked at: the result is that of
// looking at all of them.  Every lane returns the same value.
// (Stepping the two searches together, sixteen loads in flight per step, was built and measured: 0.838 ms against this
// form's 0.790 ms at 640,000 x 128 -- the probes are bound by their arithmetic, not by memory round trips, and the paired
// form probes a found side again.  DESIGN.md section 39.)
__device__ __forceinline__ BoxSpan grid_span(const float* __restrict__ ray, const OccGrid& g, const RayBox& bounds, int K,
                                             float tn, float tf, int lane) {
    BoxSpan s = ray_box_span(ray, bounds, tn, tf);
    if (!s.hit) return s;                      // a slab miss (any NaN component): no loads, [tn, tf]
    const float a = s.t0, b = s.t1, len = sub_rn(b, a);
    const int chunks = K >> 6;
    int q0 = 0;
    unsigned long long m0 = 0;
    for (; q0 < chunks; ++q0) {
        const int j = q0 * 64 + lane;
        m0 = __ballot(span_segment_live(g, ray, span_edge(a, b, len, j, K), span_edge(a, b, len, j + 1, K)));
        if (m0) break;
    }
    if (!m0) {                                 // no live segment: the ray keeps the whole interval
        s.hit = 0; s.t0 = tn; s.t1 = tf;
        return s;
    }
    int q1 = chunks - 1;
    unsigned long long m1 = m0;
    for (; q1 > q0; --q1) {
        const int j = q1 * 64 + lane;
        m1 = __ballot(span_segment_live(g, ray, span_edge(a, b, len, j, K), span_edge(a, b, len, j + 1, K)));
        if (m1) break;
    }
    if (q1 == q0) m1 = m0;
    const int j0 = q0 * 64 + __builtin_ctzll(m0), j1 = q1 * 64 + 63 - __builtin_clzll(m1);
    s.t0 = span_edge(a, b, len, j0, K);
    s.t1 = span_edge(a, b, len, j1 + 1, K);
    return s;
}
