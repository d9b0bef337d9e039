// camera.hip -- the camera optimiser's three kernels: rays formed on the device from (stored pose, learnable correction,
// pixel), the reduction of d loss / d rays to one 6-vector per image, and the corrected poses themselves.  The per-pose
// routine (exponential map, thresholds, operation order) is camera_device.h; the contract is include/nerf_amd.h.
//
//   global ray id r = m H W + h W + w  (the row of RayGenerator's table);  ray = [t, R dir_cam(h, w)]
//   backward: g_tau[m] = sum g_o,  g_w[m] = J^T sum (y x g_d)  over the batch rows of image m, y = the row's direction
//
// The backward is ONE launch without atomics or a workspace: a block per image walks the B ids (32 KiB at B = 4096, read
// from L2), every thread sums its own rows in row order, the block's 256 partial sums are folded by a fixed shuffle tree
// and a fixed LDS order -- two runs write the same bytes -- and thread 0 applies the 3x3 once.  An id outside
// [0, M H W) matches no image; an image without a row writes zeros.
#include "camera_device.h"
#include "launchers.h"

namespace {

using namespace nerf_camera;
constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void camera_rays_kernel(const float* __restrict__ poses, const float* __restrict__ xi,
                                                              const long long* __restrict__ ids, long long* __restrict__ ids_copy,
                                                              int H, int W, float f, float* __restrict__ rays, long long B, long long M) {
    const long long i = blockIdx.x * (long long)THREADS + threadIdx.x;
    if (i >= B) return;
    const long long id = ids[i];
    if (ids_copy) ids_copy[i] = id;
    const long long HW = (long long)H * W;
    float2* o = reinterpret_cast<float2*>(rays + i * 6);
    if (id < 0 || id >= M * HW) {
        const float nan = __builtin_nanf("");
        o[0] = o[1] = o[2] = make_float2(nan, nan);
        return;
    }
    const long long m = id / HW;
    const int pix = (int)(id - m * HW), h = pix / W, w = pix - h * W;
    const Pose p = corrected_pose(poses + m * 12, xi ? xi + m * 6 : nullptr);
    float y[3];
    world_direction(p, H, W, f, h, w, y);
    o[0] = make_float2(p.t[0], p.t[1]);
    o[1] = make_float2(p.t[2], y[0]);
    o[2] = make_float2(y[1], y[2]);
}

__global__ __launch_bounds__(THREADS) void camera_backward_kernel(const float* __restrict__ poses, const float* __restrict__ xi,
                                                                  const long long* __restrict__ ids,
                                                                  const float* __restrict__ d_rays, int H, int W, float f,
                                                                  float* __restrict__ g_xi, long long B) {
    const long long m = blockIdx.x;
    const unsigned long long HW = (unsigned long long)H * W, lo = (unsigned long long)m * HW;
    const float* xm = xi ? xi + m * 6 : nullptr;
    const Pose p = corrected_pose(poses + m * 12, xm);
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long long i = threadIdx.x; i < B; i += THREADS) {
        const unsigned long long pix = (unsigned long long)ids[i] - lo;        // a bad id wraps far past HW
        if (pix >= HW) continue;
        const int h = (int)((unsigned)pix / (unsigned)W), w = (int)pix - h * W;
        const float2* g2 = reinterpret_cast<const float2*>(d_rays + i * 6);
        const float2 g01 = g2[0], g23 = g2[1], g45 = g2[2];
        const float gd[3] = {g23.y, g45.x, g45.y};
        float y[3], s[3];
        world_direction(p, H, W, f, h, w, y);
        cross(y, gd, s);
        acc[0] = add_rn(acc[0], s[0]); acc[1] = add_rn(acc[1], s[1]); acc[2] = add_rn(acc[2], s[2]);
        acc[3] = add_rn(acc[3], g01.x); acc[4] = add_rn(acc[4], g01.y); acc[5] = add_rn(acc[5], g23.x);
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
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        t[k] = part[0][k];
#pragma unroll
        for (int v = 1; v < THREADS / 64; ++v) t[k] = add_rn(t[k], part[v][k]);
    }
    float gw[3] = {t[0], t[1], t[2]};
    if (xm) {
        const float w[3] = {xm[0], xm[1], xm[2]};
        left_jacobian_transposed(w, t, gw);
    }
    float2* o = reinterpret_cast<float2*>(g_xi + m * 6);
    o[0] = make_float2(gw[0], gw[1]);
    o[1] = make_float2(gw[2], t[3]);
    o[2] = make_float2(t[4], t[5]);
}

__global__ __launch_bounds__(THREADS) void camera_poses_kernel(const float* __restrict__ poses, const float* __restrict__ xi,
                                                               float* __restrict__ out, long long M) {
    const long long m = blockIdx.x * (long long)THREADS + threadIdx.x;
    if (m >= M) return;
    const Pose p = corrected_pose(poses + m * 12, xi ? xi + m * 6 : nullptr);
    float4* o = reinterpret_cast<float4*>(out + m * 12);
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = make_float4(p.r[3 * r], p.r[3 * r + 1], p.r[3 * r + 2], p.t[r]);
}

}  // namespace

// B, M >= 1 and below 2^31 (api.hip refuses the rest): the grids fit
extern "C" int nerf_amd_launch_camera_rays(const float* poses, const float* xi, const long long* ids, long long* ids_copy, int H,
                                           int W, float f, float* rays, long long B, long long M, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(camera_rays_kernel, dim3((unsigned)((B + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, poses, xi, ids,
                       ids_copy, H, W, f, rays, B, M);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_camera_rays_backward(const float* poses, const float* xi, const long long* ids, const float* d_rays,
                                                    int H, int W, float f, float* g_xi, long long B, long long M,
                                                    hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(camera_backward_kernel, dim3((unsigned)M), dim3(THREADS), 0, stream, poses, xi, ids, d_rays, H, W, f, g_xi, B);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_camera_poses(const float* poses, const float* xi, float* out, long long M, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(camera_poses_kernel, dim3((unsigned)((M + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, poses, xi, out, M);
    return (int)hipGetLastError();
}
