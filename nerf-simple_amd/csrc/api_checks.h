// api_checks.h -- host-side argument rules shared by the sources that implement the C ABI (include/nerf_amd.h): api.hip and
// the self-contained entry points in occupancy_graph.hip, occupancy_hier.hip and occupancy_terminate.hip.  Host code only.
#pragma once
#include "nerf_device.h"
#include "../../include/nerf_amd.h"

inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// the jitter arguments of every rays-mode entry point: explicit u / ts, the counter RNG, or the counter RNG with its seed
// offset in device memory (then `u` is that address).  With TS_GIVEN the kernels read the positions through `u` whatever
// the other flags say, so `u` is required then.
inline bool bad_jitter(uint32_t flags, const float* u, const float* tbins) {
    if (flags & ~(NERF_AMD_TS_GIVEN | NERF_AMD_DEVICE_RNG | NERF_AMD_SEED_IN_MEMORY)) return true;     // unknown bits
    if (flags & NERF_AMD_SEED_IN_MEMORY) {
        if (!(flags & NERF_AMD_DEVICE_RNG) || (flags & NERF_AMD_TS_GIVEN) || !u) return true;
        if (misaligned(u, 8)) return true;                                     // the kernels load it as one 64-bit word
    } else if ((!(flags & NERF_AMD_DEVICE_RNG) || (flags & NERF_AMD_TS_GIVEN)) && !u) {
        return true;
    }
    return !(flags & NERF_AMD_TS_GIVEN) && !tbins;
}

// the rays and jitter of a rays-mode launch whose kernels form the sample positions themselves
inline MlpArgs rays_args(const float* rays, const float* u, const float* tbins, uint32_t flags, uint64_t seed, int64_t ray_id0,
                         int64_t B, int N) {
    MlpArgs a{};
    a.rays = rays; a.u = u; a.tbins = tbins;
    a.P = B * (int64_t)N; a.N = N; a.flags = flags; a.seed = seed; a.ray_id0 = ray_id0;
    return a;
}
