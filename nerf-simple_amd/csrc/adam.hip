// adam.hip -- the optimizer step of the training loop (reference train.py:43,55-57:
// torch.optim.Adam(lr=5e-4, betas=(0.9,0.999), eps=1e-8) + per-step exponential LR
// decay) as ONE kernel over the flat fp32 parameter vector (state_dict order),
// SURVEY.md section 8f, N3.  The 24 tensors are views of that vector on the Python
// side, so there is no per-tensor launch; the packed MFMA weight images are
// re-derived from the same vector right after (nerf_amd_pack_weights).
//
// Per element, exactly torch's single-tensor Adam (no amsgrad, no weight decay):
//   m = b1 m + (1-b1) g ;  v = b2 v + (1-b2) g^2
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
#include "nerf_device.h"
#include "launchers.h"

namespace {
// The element update every Adam kernel of this file applies, on the gradient value `gi` its caller has formed.
__device__ __forceinline__ void adam_element(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, long long i,
                                             float gi, float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt) {
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] -= (lr / bc1) * (mi / denom);
}
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long long n, float lr, float b1, float b2, float eps,
                            float bc1, float bc2_sqrt) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        adam_element(p, m, v, i, g[i], lr, b1, b2, eps, bc1, bc2_sqrt);
    }
}
// The same update with its step-dependent scalars read from device memory
// (hyper = {lr, beta1, beta2, eps, 1 - beta1^t, sqrt(1 - beta2^t)}), so the launch can live
// inside a captured hipGraph that is replayed with a new learning rate / step count.
__global__ void adam_hyper_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                  float* __restrict__ v, long long n, const float* __restrict__ hyper) {
    const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], bc1 = hyper[4], bc2_sqrt = hyper[5];
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        adam_element(p, m, v, i, g[i], lr, b1, b2, eps, bc1, bc2_sqrt);
    }
}
// The step's scalars from a ring in pinned HOST memory (8 floats per slot, written by the host before it launches the
// step) into the device vector the other kernels read, as a kernel: slot = *counter % slots, then *counter += 1.  A
// replayed hipGraph can so begin with its own parameters' upload -- a stream-ordered hipMemcpyAsync between two graph
// launches costs ~20 us of idle GPU at the seam (copy engine start + the launch behind it), a kernel node 2 us.
__global__ void hyper_fetch_kernel(const float* ring, int slots, float* __restrict__ hyper, unsigned* __restrict__ counter) {
    const unsigned c = *counter;
    const float v = __builtin_nontemporal_load(ring + (size_t)(c % (unsigned)slots) * 8 + threadIdx.x);
    __syncthreads();                       // every thread has read the counter
    hyper[threadIdx.x] = v;
    if (threadIdx.x == 0) *counter = c + 1;
}

// ---- the gradient guard: global-norm clipping and the non-finite step guard (include/nerf_amd.h) ----------------------------
// norm = fl32(sqrt(sum g_i^2)), every square and the sum in double (a square of an fp32 value is exact in double, and the
// sum of n of them neither overflows nor underflows), in ONE fixed order whatever n is: element i belongs to thread
// i % GUARD_SPAN (block (i % GUARD_SPAN) / GUARD_THREADS), a thread adds its elements in ascending order, a wave and then a
// block add by a fixed tree, and the finish adds the GUARD_BLOCKS block sums in index order.  No atomics: two runs write the
// same bytes.
// 256 workgroups of 1024 threads: one per CU, four waves per SIMD, and at the network's 595,844 elements (1,191,688 for the
// pair) a thread owns two or three (four or five) of them -- the kernel is the latency of a few loads, so GUARD_UNROLL of them are in
// flight at once (an element past the end adds +0.0, which changes no bit of a sum of squares).
constexpr int GUARD_BLOCKS = GRAD_GUARD_BLOCKS, GUARD_THREADS = 1024, GUARD_SPAN = GUARD_BLOCKS * GUARD_THREADS, GUARD_UNROLL = 4;
__global__ __launch_bounds__(GUARD_THREADS) void grad_norm_partial_kernel(const float* __restrict__ g, long long n,
                                                                          double* __restrict__ partial) {
    __shared__ double waves[GUARD_THREADS / 64];
    double acc = 0.0;
    for (long long i = blockIdx.x * (long long)GUARD_THREADS + threadIdx.x; i < n; i += (long long)GUARD_UNROLL * GUARD_SPAN) {
        float x[GUARD_UNROLL];
#pragma unroll
        for (int k = 0; k < GUARD_UNROLL; ++k) {
            const long long j = i + (long long)k * GUARD_SPAN;
            x[k] = j < n ? g[j] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < GUARD_UNROLL; ++k) {
            const double d = (double)x[k];
            acc += d * d;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = waves[0];
        for (int w = 1; w < GUARD_THREADS / 64; ++w) s += waves[w];
        partial[blockIdx.x] = s;
    }
}
// The finish: the block sums in index order, the norm, the verdict and the running totals into the guard record
// (8 words: max_norm [input], norm, coef, skip, steps seen, steps skipped, steps clipped, 0).  coef is torch's
// clip_grad_norm_ rule, three fp32 operations each rounded on its own: min(1, max_norm / (norm + 1e-6)).
__global__ __launch_bounds__(GUARD_BLOCKS) void grad_guard_finish_kernel(const double* __restrict__ partial, unsigned* guard) {
    __shared__ double sums[GUARD_BLOCKS];
    sums[threadIdx.x] = partial[threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < GUARD_BLOCKS; ++b) s += sums[b];
    const float max_norm = __uint_as_float(guard[0]);
    const float norm = (float)sqrt(s);
    const bool skip = !(fabsf(norm) <= 3.402823466e38f);                 // NaN or inf: a non-finite element, or a norm beyond fp32
    const float coef = skip ? 0.f : fminf(1.f, __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f)));
    guard[1] = __float_as_uint(norm);
    guard[2] = __float_as_uint(coef);
    guard[3] = skip ? 1u : 0u;
    guard[4] = guard[4] + 1u;
    guard[5] = guard[5] + (skip ? 1u : 0u);
    guard[6] = guard[6] + ((!skip && coef < 1.f) ? 1u : 0u);
    guard[7] = 0u;
}
// adam_hyper_kernel on coef g (one rounded product per element; the gradient as it is where coef == 1), nothing at all when
// the record's skip word is set.
__global__ void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                    float* __restrict__ v, long long n, const float* __restrict__ hyper,
                                    const unsigned* __restrict__ guard) {
    if (guard[3] != 0u) return;
    const float coef = __uint_as_float(guard[2]);
    const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], bc1 = hyper[4], bc2_sqrt = hyper[5];
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float gi = g[i];
        adam_element(p, m, v, i, coef == 1.f ? gi : __fmul_rn(gi, coef), lr, b1, b2, eps, bc1, bc2_sqrt);
    }
}
}  // namespace

extern "C" int nerf_amd_launch_grad_guard(const float* grads, long long n, double* partial, unsigned* guard, hipStream_t stream) {
    (void)hipGetLastError();
    // every block writes its sum (0 where it owns no element), so the finish reads nothing stale: n == 0 launches too
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(GUARD_BLOCKS), dim3(GUARD_THREADS), 0, stream, grads, n, partial);
    hipLaunchKernelGGL(grad_guard_finish_kernel, dim3(1), dim3(GUARD_BLOCKS), 0, stream, (const double*)partial, guard);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_adam_guarded(float* params, const float* grads, float* m, float* v, long long n,
                                            const float* hyper, const unsigned* guard, hipStream_t stream) {
    (void)hipGetLastError();
    if (n == 0) return 0;
    long long grid = (n + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(adam_guarded_kernel, dim3((unsigned)grid), dim3(256), 0, stream, params, grads, m, v, n, hyper, guard);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_hyper_fetch(const float* ring_host, int slots, float* hyper, unsigned* counter, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(hyper_fetch_kernel, dim3(1), dim3(8), 0, stream, ring_host, slots, hyper, counter);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_adam_hyper(float* params, const float* grads, float* m, float* v, long long n,
                                          const float* hyper, hipStream_t stream) {
    (void)hipGetLastError();
    if (n == 0) return 0;
    long long grid = (n + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(adam_hyper_kernel, dim3((unsigned)grid), dim3(256), 0, stream, params, grads, m, v, n, hyper);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_adam(float* params, const float* grads, float* m, float* v, long long n, float lr,
                                    float b1, float b2, float eps, float bc1, float bc2_sqrt, hipStream_t stream) {
    (void)hipGetLastError();
    if (n == 0) return 0;
    long long grid = (n + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)grid), dim3(256), 0, stream, params, grads, m, v, n, lr, b1, b2,
                       eps, bc1, bc2_sqrt);
    return (int)hipGetLastError();
}
