// sigma_noise_device.h -- the sigma-noise regulariser (the NeRF paper's raw_noise_std; the reference leaves it as
// `## TODO add gaussian noise regularizer`, utils/rendering.py:63): sigma' = sigma + std z in front of the softplus, z a
// standard normal from the counter RNG.  Written ONCE: nerf_amd_sigma_noise and the training head (composite_head.hip) call
// the routine below, and so do their masked counterparts (masked_controls.hip, occupancy_train.hip), so all write the same
// bits for the same (key, sample).
//
// Key: (noise_seed + the step's offset in memory) ^ NOISE_KEY -- the offset goes in front of the xor, as in the sampler's
// seed (composite.hip, the coarse head), so a replayed graph at step k draws what an eager call with noise_seed + k draws.
// Counters: sample = (ray_id0 + ray) N + i owns the words 2 sample and 2 sample + 1, so the stream depends on neither the
// batching nor the sharding of the rays and shares nothing with the stratified jitter (key: the bare seed).
//
// Box-Muller, every step one explicitly rounded op or a named library function (no contraction left to the compiler):
//   u1 = ((word1 >> 8) + 1) 2^-24  in (0, 1]   (exact: a 24-bit integer + 1, times a power of two)
//   u2 =  (word2 >> 8)      2^-24  in [0, 1)   (exact)
//   z  = mul_rn(sqrt_rn(mul_rn(-2, logf(u1))), cospif(mul_rn(2, u2)))      (2 u2 is exact: cos(2 pi u2) with no rounded 2 pi)
// |z| <= sqrt(2 * 24 ln 2) = 5.77; u1 = 1 gives z = +-0.
#pragma once
#include "composite_backward_device.h"
#include "sample_pdf_device.h"

namespace nerf_noise {

using nerf_pdf::NOISE_KEY;

// the launch's key; `seed_mem` (NERF_AMD_SEED_IN_MEMORY) is the device address of the 64-bit step offset, or NULL
__device__ __forceinline__ unsigned long long noise_key(unsigned long long seed, const unsigned long long* seed_mem) {
    if (seed_mem) {
        const unsigned long long v = *seed_mem;
        // wave-uniform by construction: keep it in scalar registers whatever load the compiler picked
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        seed += ((unsigned long long)hi << 32) | lo;
    }
    return seed ^ NOISE_KEY;
}

__device__ __forceinline__ float standard_normal(unsigned long long key, unsigned long long sample) {
    const unsigned w1 = philox_word(key, 2ull * sample), w2 = philox_word(key, 2ull * sample + 1ull);
    const float u1 = mul_rn((float)((w1 >> 8) + 1u), 1.0f / 16777216.0f);
    const float u2 = mul_rn((float)(w2 >> 8), 1.0f / 16777216.0f);
    const float r = sqrt_rn(mul_rn(-2.0f, logf(u1)));
    return mul_rn(r, cospif(mul_rn(2.0f, u2)));
}

// sigma' of one sample: two separately rounded ops (d sigma' / d sigma = 1)
__device__ __forceinline__ float noisy_sigma(float sigma, float std, unsigned long long key, unsigned long long sample) {
    return add_rn(sigma, mul_rn(std, standard_normal(key, sample)));
}

// A sample source (DenseSamples, MaskedSamplesBwd) with the routine above applied to sigma as a chunk is loaded, for the
// training heads (composite_head.hip, occupancy_train.hip): the forward sweep keeps sigma'-derived values per chunk and the
// backward sweep reuses them, so each sample's noise is generated once.  The noise goes only where the source returned a
// row: every sample of a dense ray, and of a masked one the kept samples -- a dead or over-capacity sample stays
// (0, 0, 0, -inf) whatever std is (-inf + NaN would not), so its alpha and w are exactly 0.  The counter is the ORIGINAL
// sample index: a live sample draws what the dense stage gives that sample.
template <class Src>
struct Noisy {
    Src src;
    float std;
    unsigned long long key, sample0;       // sample0 = (ray_id0 + ray) N
    __device__ __forceinline__ nerf_composite::BwdSample chunk(int ch, int i, int lane, bool valid, int N) {
        nerf_composite::BwdSample s = src.chunk(ch, i, lane, valid, N);
        if (s.row >= 0) s.c[3] = noisy_sigma(s.c[3], std, key, sample0 + (unsigned long long)i);
        return s;
    }
};

}  // namespace nerf_noise
