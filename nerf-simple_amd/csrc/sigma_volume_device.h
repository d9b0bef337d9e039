// sigma_volume_device.h -- the sigma volume of grid-guided sampling as a kernel sees it and the look-up of one point in it
// (include/nerf_amd.h, "grid-guided fine sampling", step 2), shared by guided_sample.hip and guided_masked.hip.
#pragma once
#include "nerf_device.h"

struct SigmaVolume {                           // V[n0, n1, n2], C order
    long long n[3];
    float lo[3], inv_step[3];
};

inline SigmaVolume sigma_volume_args(long long nx, long long ny, long long nz, const float* h_lo, const float* h_inv_step) {
    SigmaVolume g;
    g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
    for (int a = 0; a < 3; ++a) { g.lo[a] = h_lo[a]; g.inv_step[a] = h_inv_step[a]; }
    return g;
}

// the look-up of one point: max over the 8 corners of its cell, NaN corners skipped; -inf outside the grid
__device__ __forceinline__ float volume_value(const SigmaVolume& g, const float* __restrict__ vol, float x, float y, float z) {
    const float p[3] = {x, y, z};
    long long c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float f = floorf(mul_rn(sub_rn(p[a], g.lo[a]), g.inv_step[a]));
        if (!(f >= 0.f && f < (float)(g.n[a] - 1))) return -__builtin_inff();       // also NaN
        c[a] = (long long)f;
        if (c[a] < 0 || c[a] > g.n[a] - 2) return -__builtin_inff();               // (float)(n - 1) may round up: never past the volume
    }
    const float* base = vol + (c[0] * g.n[1] + c[1]) * g.n[2] + c[2];
    const long long sy = g.n[2], sx = g.n[1] * g.n[2];
    float m = -__builtin_inff();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float v = base[(k >> 2) * sx + ((k >> 1) & 1) * sy + (k & 1)];
        if (v > m) m = v;                      // false for a NaN corner
    }
    return m;
}

struct VolumeSamples {                         // a ray's positions and looked-up values (LDS), as composite_ray reads them
    const float* ts;
    const float* sigma;
    __device__ __forceinline__ float t(int i) const { return ts[i]; }
    __device__ __forceinline__ f32x4 c(int i) const { return f32x4{0.f, 0.f, 0.f, sigma[i]}; }
};
