// ray_box_device.h -- a ray against an axis-aligned scene box: the slab test and the clipped sampling interval
// (include/nerf_amd.h, "scene box"; tests/box_model.py restates it op for op).  Device code only, no
// kernel: ray_box.hip launches it, and a fused variant can include it.
// Every operation is one IEEE fp32 operation with its own rounding (nerf_device.h: sub_rn / mul_rn / add_rn -- hipcc's
// __fsub_rn and friends are plain operators and contract; __fdiv_rn is the correctly rounded division); min and max are
// written as comparisons so that a NaN on either side comes out and the final `t0 < t1` is false for it.
#pragma once
#include "nerf_device.h"

struct RayBox {
    float lo[3], hi[3];          // lo < hi, finite (checked on the host)
};
struct BoxSpan {
    float t0, t1;                // the interval the ray's samples are placed in
    int hit;                     // 1: [t0, t1] is the clipped interval; 0: the ray misses and keeps [tn, tf]
};

__device__ __forceinline__ float box_max(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float box_min(float a, float b) { return (a < b || a != a) ? a : b; }

// (o, d): the ray as render_nerf takes it, d un-normalised.  Per axis: d != 0 -- the two plane crossings (lo - o) / d and
// (hi - o) / d, ordered; d == 0 (either sign) -- nothing if lo <= o <= hi, a miss otherwise (also for a NaN origin).
__device__ __forceinline__ BoxSpan ray_box_span(const float* __restrict__ ray, const RayBox& box, float tn, float tf) {
    float t0 = tn, t1 = tf;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float o = ray[a], d = ray[3 + a];
        if (d != 0.0f) {         // true for a NaN d: it reaches t0 / t1 and fails the comparison below
            const float ta = __fdiv_rn(sub_rn(box.lo[a], o), d), tb = __fdiv_rn(sub_rn(box.hi[a], o), d);
            t0 = box_max(t0, box_min(ta, tb));
            t1 = box_min(t1, box_max(ta, tb));
        } else {
            inside = inside && (o >= box.lo[a]) && (o <= box.hi[a]);
        }
    }
    BoxSpan s;
    s.hit = (inside && t0 < t1) ? 1 : 0;
    s.t0 = s.hit ? t0 : tn;
    s.t1 = s.hit ? t1 : tf;
    return s;
}

// unit position c (what the jitter rule forms on the bins linspace(0, 1, N + 1)) -> the sample position in [t0, t1]
__device__ __forceinline__ float box_place(const BoxSpan& s, float c) {
    const float t = add_rn(s.t0, mul_rn(sub_rn(s.t1, s.t0), c));
    return t < s.t1 ? t : s.t1;  // one rounding may carry the last position past t1; a NaN c gives t1
}
