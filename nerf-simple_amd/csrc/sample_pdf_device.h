// sample_pdf_device.h -- the per-ray body of hierarchical sample placement (BASELINE config 4), shared by
// sample_pdf.hip (positions and weights read from HBM), the guided samplers and the coarse training heads (composite.hip,
// composite_head.hip, occupancy_train.hip: weights handed over from the compositor's registers through the wave's LDS
// slice; the two dense ones through sample_behind_walk below), and the launchers' Nf -> E dispatch.  ABSENT from the reference
// (README.md:3, configs/lego.yaml:7): parity UNPINNED; the NeRF paper's sample_pdf over interior bins, checked
// against oracle/nerf_oracle.sample_pdf.
//
//   mids  = (ts[1:] + ts[:-1]) / 2                      Nc-1 bin edges
//   pdf   = (w[1:-1] + 1e-5) / sum                      Nc-2 bins
//   cdf   = [0, cumsum(pdf)]                            Nc-1 values
//   z     = inverse-cdf(u), linear inside a bin         Nf new positions
//   out   = sort(concat(ts, z))                         Nc+Nf positions per ray
//
// One wavefront per ray.  The cdf is a wave-level inclusive sum scan; each lane inverts it for its own u by
// binary search.  Only the Nf new positions are unsorted (the coarse ones already are), so they alone are
// sorted -- a bitonic network held in registers, E = ceil_pow2(Nf)/64 keys per lane, strides below 64 by wave
// shuffle, larger strides between a lane's own registers, no LDS traffic -- and the two sorted lists are
// merged by rank: a coarse position lands at i + #{z < ts[i]}, a new one at j + #{ts <= z[j]} (two binary
// searches per element).  Nc <= 256, Nf <= 512, Nc + Nf <= 512.
#pragma once
#include "launchers.h"
#include "nerf_device.h"

namespace nerf_pdf {

constexpr int MAXC = 256;
constexpr int MAXM = 512;
// the sizes the sampler serves, for Nc > 0 and Nf >= 0: the one statement of the rule, for the launchers and the C ABI
__host__ __device__ constexpr bool unsupported_sizes(int Nc, int Nf) { return Nc < 3 || Nc > MAXC || Nc + Nf > MAXM; }
constexpr unsigned long long RNG_KEY = 0x9e3779b97f4a7c15ull;     // the sampler's counter-RNG key: seed ^ RNG_KEY
// the sigma-noise regulariser's key ("noise:v1"): noise_seed ^ NOISE_KEY (sigma_noise_device.h); apart from RNG_KEY, from the
// ray selection's key (select.hip SEL_KEY) and from the stratified jitter's, which is the bare seed
constexpr unsigned long long NOISE_KEY = 0x6e6f6973653a7631ull;

// keys per lane of the register sort for Nf new samples: ceil_pow2(Nf) / 64 (1, 2, 4 or 8)
__host__ __device__ constexpr int keys_per_lane(int Nf) { return Nf <= 64 ? 1 : Nf <= 128 ? 2 : Nf <= 256 ? 4 : 8; }

// the LDS one wave works in (E = keys_per_lane)
template <int E>
struct WaveLds {
    float cdf[MAXC];
    float bins[MAXC];
    float ts[MAXC];           // the ray's Nc coarse positions: the caller fills it
    float z[E * 64];
    float all[MAXM];
};

// ascending bitonic sort of E*64 keys held as v[e] = key (e*64 + lane), by one wave
template <int E>
__device__ __forceinline__ void wave_bitonic_sort(float (&v)[E], int lane) {
#pragma unroll
    for (int k = 2; k <= E * 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j >= 64) {
                const int de = j >> 6;                 // partner register: e ^ de
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if ((e & de) == 0) {
                        const bool up = (((e * 64) & k) == 0);          // k >= 128 here: lane bits do not matter
                        const float a = v[e], b = v[e ^ de];
                        const float lo = fminf(a, b), hi = fmaxf(a, b);
                        v[e] = up ? lo : hi;
                        v[e ^ de] = up ? hi : lo;
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int i = e * 64 + lane;
                    const bool up = (i & k) == 0;
                    const float other = __shfl_xor(v[e], j);
                    const bool lower = (lane & j) == 0;                   // this lane holds the lower index of the pair
                    v[e] = (lower == up) ? fminf(v[e], other) : fmaxf(v[e], other);
                }
            }
        }
    }
}

// One ray: s.ts[0..Nc) holds its coarse positions (written by this wave and fenced), rw[0..Nc) its weights (any
// address space).  Jitter: u[ray * Nf + j], or with device_rng the counter RNG keyed (seed ^ RNG_KEY,
// (ray_id0 + ray) * Nf + j) -- the caller resolves a seed held in device memory first.  Writes out[0..Nc+Nf).
template <int E>
__device__ __forceinline__ void sample_ray(WaveLds<E>& s, const float* rw, int Nc, int Nf, int lane, const float* u,
                                           bool device_rng, unsigned long long seed, long long ray_id0, long long ray,
                                           float* __restrict__ out) {
    float* cdf = s.cdf;
    float* bins = s.bins;
    const float* cts = s.ts;
    float* zs = s.z;
    float* all = s.all;
    const int nb = Nc - 1;                             // bin edges (mids); nb-1 bins

    for (int i = lane; i < nb; i += 64) bins[i] = 0.5f * (cts[i + 1] + cts[i]);
    // inclusive scan of (w[1:-1] + 1e-5) in chunks of 64, cdf[0] = 0
    float carry = 0.f;
    for (int base = 0; base < nb - 1; base += 64) {
        const int i = base + lane;
        float v = i < nb - 1 ? rw[i + 1] + 1e-5f : 0.f;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float up = __shfl_up(v, off);
            if (lane >= off) v += up;
        }
        if (i < nb - 1) cdf[i + 1] = carry + v;
        carry += __shfl(v, 63);
    }
    if (lane == 0) cdf[0] = 0.f;
    const float total = carry;
    wave_lds_fence();

    // inverse cdf for each new sample: key j = e*64 + lane, +inf beyond Nf
    float z[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int j = e * 64 + lane;
        z[e] = __builtin_inff();
        if (j < Nf) {
            float uu;
            if (device_rng) uu = philox_uniform(seed ^ RNG_KEY, (unsigned long long)((ray_id0 + ray) * Nf + j));
            else uu = u[ray * Nf + j];
            const float target = uu * total;           // cdf kept un-normalised: compare against u * sum
            // searchsorted(cdf, target, side='right') over cdf[0..nb-1]
            int lo = 0, hi = nb;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (cdf[mid] <= target) lo = mid + 1; else hi = mid;
            }
            const int below = lo - 1 > 0 ? lo - 1 : 0;
            const int above = lo < nb - 1 ? lo : nb - 1;
            const float c0 = cdf[below] / total, c1 = cdf[above] / total;
            float denom = c1 - c0;
            if (denom < 1e-5f) denom = 1.f;
            const float tt = (uu - c0) / denom;
            z[e] = bins[below] + tt * (bins[above] - bins[below]);
        }
    }
    wave_bitonic_sort<E>(z, lane);
#pragma unroll
    for (int e = 0; e < E; ++e) zs[e * 64 + lane] = z[e];
    wave_lds_fence();

    // merge by rank: coarse position i -> i + #{z < ts[i]};  new position j -> j + #{ts <= z[j]}
    for (int i = lane; i < Nc; i += 64) {
        const float t = cts[i];
        int lo = 0, hi = Nf;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (zs[mid] < t) lo = mid + 1; else hi = mid;
        }
        all[i + lo] = t;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int j = e * 64 + lane;
        if (j < Nf) {
            int lo = 0, hi = Nc;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (cts[mid] <= z[e]) lo = mid + 1; else hi = mid;
            }
            all[j + lo] = z[e];
        }
    }
    wave_lds_fence();
    const int M = Nc + Nf;
    for (int i = lane; i < M; i += 64) out[i] = all[i];
}

// The sampler behind a dense walk of the same wave (composite_backward_kernel<E>, composite.hip; dense_head_kernel<.., E>,
// composite_head.hip): the walk's PdfSink left the ray's positions in s.ts and its weights in rw, both LDS.  Fences them,
// resolves a seed whose offset is held in device memory (p.seed_in_mem: p.u is its address) and places the samples --
// nerf_amd_sample_pdf's body, same draws.
template <int E>
__device__ __forceinline__ void sample_behind_walk(WaveLds<E>& s, const float* rw, int Nc, int lane, const DensePdfArgs& p,
                                                   long long ray_id0, long long ray) {
    wave_lds_fence();
    unsigned long long seed = p.seed;
    if (p.seed_in_mem) {
        const unsigned long long v = *reinterpret_cast<const unsigned long long*>(p.u);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        seed += ((unsigned long long)hi << 32) | lo;
    }
    sample_ray<E>(s, rw, Nc, p.Nf, lane, p.u, p.device_rng != 0, seed, ray_id0, ray, p.ts_out + ray * (Nc + p.Nf));
}

// Host: Nf -> the compile-time E of a launch, the one place keys_per_lane is switched over.  f is called once with
// std::integral_constant<int, E>, e.g. with_keys_per_lane(Nf, [&](auto e) { launch(kernel<e()>) ... });
template <class F>
inline void with_keys_per_lane(int Nf, F&& f) {
    switch (keys_per_lane(Nf)) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        default: f(std::integral_constant<int, 8>{}); break;
    }
}

}  // namespace nerf_pdf
