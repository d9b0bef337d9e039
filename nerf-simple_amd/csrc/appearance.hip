// appearance.hip -- the per-image colour correction trained beside the network: image m of M holds theta[m] = (a[3], b[3]),
// and a ray of it is compared with its pixel behind  c' = (1 + a) rgb + b  (appearance_device.h: the three-op map and its
// backward; the contract is include/nerf_amd.h).  Four small stages; the training head is their composition:
//
//   gather            theta_ray[i] = theta[ids[i] / HW] (a row of NaN for an id outside [0, M HW)); keeps a copy of the ids
//   apply             c' = (1 + a) rgb + b per ray
//   apply_backward    g_rgb = g fl(1 + a),  the ray's row of d loss / d theta = (g rgb, g)
//   reduce            g_theta[m] = sum of the rows of image m, + reg theta[m] (the ridge), or zeros for a frozen image
//   head              compositor -> apply -> MSE gradient -> apply_backward -> compositor backward: BY DEFINITION that
//                     composition, in one launch: dense_head_kernel<.., AFFINE> (composite_head.hip)
//
// The reduction is ONE launch without atomics or a workspace, as camera.hip's: a block per image walks the B ids, every
// thread sums its own rows in row order, the block's 256 partial sums are folded by a fixed shuffle tree and a fixed LDS
// order -- two runs write the same bytes.  An id outside [0, M HW) matches no image.
#include "appearance_device.h"
#include "launchers.h"

namespace {

using namespace nerf_appearance;
constexpr int THREADS = 256;

// ---- the stages ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void appearance_gather_kernel(const float* __restrict__ theta, const long long* __restrict__ ids,
                                                                    long long* __restrict__ ids_copy, long long HW,
                                                                    float* __restrict__ theta_ray, long long B, long long M) {
    const long long i = blockIdx.x * (long long)THREADS + threadIdx.x;
    if (i >= B) return;
    const long long id = ids[i];
    if (ids_copy) ids_copy[i] = id;
    const Row r = (id < 0 || id >= M * HW) ? nan_row() : load_row(theta + (id / HW) * 6);
    store_row(theta_ray + i * 6, r.a, r.b);
}

// out may be rgb: every thread reads its own ray before it writes it
__global__ __launch_bounds__(THREADS) void appearance_apply_kernel(const float* rgb, const float* __restrict__ theta_ray,
                                                                   long long theta_stride, float* out, long long B) {
    const long long i = blockIdx.x * (long long)THREADS + threadIdx.x;
    if (i >= B) return;
    const Row r = load_row(theta_ray + i * theta_stride);
    float gain[3];
    gains(r, gain);
    const float c0 = rgb[i * 3 + 0], c1 = rgb[i * 3 + 1], c2 = rgb[i * 3 + 2];
    out[i * 3 + 0] = apply(gain[0], c0, r.b[0]);
    out[i * 3 + 1] = apply(gain[1], c1, r.b[1]);
    out[i * 3 + 2] = apply(gain[2], c2, r.b[2]);
}

// g_rgb may be g_out (the same reason)
__global__ __launch_bounds__(THREADS) void appearance_apply_backward_kernel(const float* g_out, const float* __restrict__ rgb,
                                                                            const float* __restrict__ theta_ray,
                                                                            long long theta_stride, float* g_rgb,
                                                                            float* __restrict__ g_theta_ray, long long B) {
    const long long i = blockIdx.x * (long long)THREADS + threadIdx.x;
    if (i >= B) return;
    const Row r = load_row(theta_ray + i * theta_stride);
    float gain[3], g_c[3], g_a[3];
    gains(r, gain);
    const float g[3] = {g_out[i * 3 + 0], g_out[i * 3 + 1], g_out[i * 3 + 2]};
    const float c[3] = {rgb[i * 3 + 0], rgb[i * 3 + 1], rgb[i * 3 + 2]};
    apply_backward(g, c, gain, g_c, g_a);
    g_rgb[i * 3 + 0] = g_c[0]; g_rgb[i * 3 + 1] = g_c[1]; g_rgb[i * 3 + 2] = g_c[2];
    store_row(g_theta_ray + i * 6, g_a, g);
}

__global__ __launch_bounds__(THREADS) void appearance_reduce_kernel(const float* __restrict__ g_theta_ray,
                                                                    const long long* __restrict__ ids, long long HW_,
                                                                    const float* __restrict__ theta, float reg,
                                                                    const int* __restrict__ frozen, float* __restrict__ g_theta,
                                                                    long long B) {
    const long long m = blockIdx.x;
    const unsigned long long HW = (unsigned long long)HW_, lo = (unsigned long long)m * HW;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long long i = threadIdx.x; i < B; i += THREADS) {
        const unsigned long long pix = (unsigned long long)ids[i] - lo;        // a bad id wraps far past HW
        if (pix >= HW) continue;
        const Row r = load_row(g_theta_ray + i * 6);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[k] = add_rn(acc[k], r.a[k]);
            acc[3 + k] = add_rn(acc[3 + k], r.b[k]);
        }
    }
    __shared__ float part[THREADS / 64][6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[k] = add_rn(acc[k], __shfl_down(acc[k], d, 64));
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) part[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float t[6];
    const bool hold = frozen && frozen[m] != 0;    // a frozen image: exactly zero, no ridge
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        t[k] = part[0][k];
#pragma unroll
        for (int v = 1; v < THREADS / 64; ++v) t[k] = add_rn(t[k], part[v][k]);
        // the ridge (reg / 2) ||theta||^2 reaches every row, with or without a ray in the batch
        t[k] = hold ? 0.f : add_rn(t[k], mul_rn(reg, theta[m * 6 + k]));
    }
    store_row(g_theta + m * 6, t, t + 3);
}

inline dim3 per_element(long long n) { return dim3((unsigned)((n + THREADS - 1) / THREADS)); }

}  // namespace

// B, M >= 1 and below 2^31 (api.hip refuses the rest): the grids fit
extern "C" int nerf_amd_launch_appearance_gather(const float* theta, const long long* ids, long long* ids_copy, long long HW,
                                                 float* theta_ray, long long B, long long M, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(appearance_gather_kernel, per_element(B), dim3(THREADS), 0, stream, theta, ids, ids_copy, HW, theta_ray, B, M);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_appearance_apply(const float* rgb, const float* theta_ray, long long theta_stride, float* out,
                                                long long B, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(appearance_apply_kernel, per_element(B), dim3(THREADS), 0, stream, rgb, theta_ray, theta_stride, out, B);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_appearance_apply_backward(const float* g_out, const float* rgb, const float* theta_ray,
                                                         long long theta_stride, float* g_rgb, float* g_theta_ray, long long B,
                                                         hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(appearance_apply_backward_kernel, per_element(B), dim3(THREADS), 0, stream, g_out, rgb, theta_ray,
                       theta_stride, g_rgb, g_theta_ray, B);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_appearance_reduce(const float* g_theta_ray, const long long* ids, long long HW, const float* theta,
                                                 float reg, const int* frozen, float* g_theta, long long B, long long M,
                                                 hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(appearance_reduce_kernel, dim3((unsigned)M), dim3(THREADS), 0, stream, g_theta_ray, ids, HW, theta, reg,
                       frozen, g_theta, B);
    return (int)hipGetLastError();
}
