// ray_box.hip -- sample placement inside a scene box (include/nerf_amd.h, "scene box").  Generalises the
// reference's linspace(tn, tf, N + 1) bins (utils/rendering.py:24-30) to a per-ray interval; not in the reference.
//
//   box_positions_kernel -- one wavefront per ray, four rays per block (the masked kernels' shape).  Every lane reads the
//       ray's six floats (one address per wave: a broadcast) and forms the ray's interval (ray_box_device.h: ray_box_span);
//       lane l then places samples l, l + 64, ...: the unit position c is the position the jitter rule forms on the unit
//       bins (nerf_device.h: fetch_point_rays, so u / given positions / the counter RNG with its seed in memory all work
//       and nothing of the rule is restated here), ts = min(t0 + (t1 - t0) c, t1).  A wave's stores are 64 consecutive
//       floats of the ray's row; lane 0 writes span and hit.
// The kernel moves 24 B in and 4 N (+ 12) B out per ray and computes next to nothing: it is bound by its stores.  No LDS,
// no atomics, no scratch; every output element is written by exactly one lane: two runs write the same bytes.
#include "ray_box_device.h"
#include "occ_scan_device.h"
#include "launchers.h"

namespace {

__global__ __launch_bounds__(MASKED_THREADS) void box_positions_kernel(MlpArgs a, RayBox box, float tn, float tf,
                                                                       float* __restrict__ ts, float* __restrict__ span,
                                                                       int* __restrict__ hit, long long B) {
    const long long ray = (long long)blockIdx.x * MASKED_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= B) return;                      // whole wave leaves together; no barrier below
    const int lane = threadIdx.x & 63;
    const BoxSpan s = ray_box_span(a.rays + ray * 6, box, tn, tf);
    if (lane == 0) {
        if (span) { span[2 * ray] = s.t0; span[2 * ray + 1] = s.t1; }
        if (hit) hit[ray] = s.hit;
    }
    for (int i = lane; i < a.N; i += 64) {
        const float c = fetch_point_rays<false>(a, ray * a.N + i, RaySample{ray, i}).t;
        ts[ray * a.N + i] = box_place(s, c);   // a plain store: the next launch reads it, from L2 at a training batch's size
    }
}

}  // namespace

extern "C" int nerf_amd_launch_box_positions(const MlpArgs* a, const float* h_lo, const float* h_hi, float tn, float tf,
                                             float* ts, float* span, int* hit, long long B, hipStream_t s) {
    RayBox box;
    for (int i = 0; i < 3; ++i) { box.lo[i] = h_lo[i]; box.hi[i] = h_hi[i]; }
    (void)hipGetLastError();
    const long long blocks = (B + MASKED_RAYS_PER_BLOCK - 1) / MASKED_RAYS_PER_BLOCK;
    hipLaunchKernelGGL(box_positions_kernel, dim3((unsigned)blocks), dim3(MASKED_THREADS), 0, s, *a, box, tn, tf, ts, span, hit, B);
    return (int)hipGetLastError();
}
