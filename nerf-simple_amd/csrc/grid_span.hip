// grid_span.hip -- sample placement between a ray's first and last live cell of an occupancy grid (include/nerf_amd.h,
// "grid span").  The scene box's successor: the interval is cut per ray from the grid's bits, read
// in place, so a grid update between two launches (or two replays of a captured graph) simply takes effect.
//
//   span_positions_kernel -- one wavefront per ray, four rays per block (box_positions_kernel's shape).  Every lane reads
//       the ray's six floats (a broadcast), the wave probes K segments of the ray's clipped interval 64 at a time
//       (grid_span_device.h: grid_span; eight bit loads per segment, one ballot per chunk, the chunks between the first and
//       the last live one skipped), and lane l then places samples l, l + 64, ... by the box's rule (ray_box_device.h:
//       box_place) on the unit position the jitter rule forms (nerf_device.h: fetch_point_rays -- nothing of the rule is
//       restated here).  Lane 0 writes span and hit.
// The grid's words are read-only and shared by every ray: at a training grid's size (129^3: 260 KB) they sit in L2.  No LDS,
// no atomics, no scratch; every output element is written by exactly one lane: two runs write the same bytes.
#include "grid_span_device.h"
#include "occ_scan_device.h"
#include "launchers.h"

namespace {

__global__ __launch_bounds__(MASKED_THREADS) void span_positions_kernel(MlpArgs a, OccGrid g, RayBox bounds, int probes, float tn,
                                                                        float tf, float* __restrict__ ts,
                                                                        float* __restrict__ span, int* __restrict__ hit,
                                                                        long long B) {
    const long long ray = (long long)blockIdx.x * MASKED_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= B) return;                      // whole wave leaves together; no barrier below
    const int lane = threadIdx.x & 63;
    const BoxSpan s = grid_span(a.rays + ray * 6, g, bounds, probes, tn, tf, lane);
    if (lane == 0) {
        if (span) { span[2 * ray] = s.t0; span[2 * ray + 1] = s.t1; }
        if (hit) hit[ray] = s.hit;
    }
    for (int i = lane; i < a.N; i += 64) {
        const float c = fetch_point_rays<false>(a, ray * a.N + i, RaySample{ray, i}).t;
        ts[ray * a.N + i] = box_place(s, c);
    }
}

}  // namespace

extern "C" int nerf_amd_launch_span_positions(const MlpArgs* a, const unsigned* bits, long long nx, long long ny, long long nz,
                                              const float* h_lo, const float* h_hi, const float* h_inv_step, int probes,
                                              float tn, float tf, float* ts, float* span, int* hit, long long B, hipStream_t s) {
    const OccGrid g = occ_grid_args(bits, nx, ny, nz, h_lo, h_inv_step, 0);
    RayBox bounds;
    for (int i = 0; i < 3; ++i) { bounds.lo[i] = h_lo[i]; bounds.hi[i] = h_hi[i]; }
    (void)hipGetLastError();
    const long long blocks = (B + MASKED_RAYS_PER_BLOCK - 1) / MASKED_RAYS_PER_BLOCK;
    hipLaunchKernelGGL(span_positions_kernel, dim3((unsigned)blocks), dim3(MASKED_THREADS), 0, s, *a, g, bounds, probes, tn, tf,
                       ts, span, hit, B);
    return (int)hipGetLastError();
}
