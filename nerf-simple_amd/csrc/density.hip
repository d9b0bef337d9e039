// density.hip -- the sigma-only network: raw sigma of query points or of a grid generated in the kernel, on
// v_mfma_f32_16x16x32_bf16 (and, built with -DNERF_HALF, on ..._f16).  Not in the reference (its only way to sigma is the
// whole Nerf.forward, reference utils/nets.py:34-43).
//
// sigma does not depend on the view direction: sigma_fc reads h8 before the direction concat (reference utils/nets.py:36-40).
// The sigma network is therefore internal layers L0..L7 and the one 16-row tile of L8 that holds row 256 (nerf_layout.h):
// 1936 of the 2344 MFMAs of a wave-tile (82.6 %), no direction features, no colour layers.
//
// The kernel is an instantiation of the chain of mlp16_chain.h -- the code mlp_bf16_16.hip runs, not a copy of it -- on a
// shorter plan over the same packed 16-bit image of nerf_amd_pack_weights: 30 chunks per 256-point tile
//   L0 (16 tiles, K = 64: one chunk) | L1..L7 (4 chunks of four 16-row tiles each) | the sigma tile of L8 (one chunk).
// Fragment order, bias-initialised accumulators, k-step order, ReLU / pack conversion, the in-kernel encoder and the
// range guard are therefore the forward's, and sigma equals column 3 of nerf_amd_mlp_forward's output on the same
// points bit for bit.  What is this file's own: the plan, the input fetch and the one-float output (and, kept equal to
// mlp_bf16_16.hip's by hand, the kernel prologue and the posx encoder block: mlp16_chain.h says why).
// Inputs: explicit points (any row stride >= 3) or grid point p of an [Rx, Ry, Rz] grid (C order, z fastest) with
// coordinates x_a(i) = fl(lo_a + fl(i s_a)), formed here -- no input buffer.
#include "nerf_device.h"
#include "launchers.h"

using namespace nerf_layout;

#ifdef NERF_HALF
typedef _Float16 elem_t;
#define NERF_MFMA __builtin_amdgcn_mfma_f32_16x16x32_f16
#define DENSITY_KERNEL nerf_density_f16_kernel
#define DENSITY_LAUNCH nerf_amd_launch_density_f16
#else
typedef __bf16 elem_t;
#define NERF_MFMA __builtin_amdgcn_mfma_f32_16x16x32_bf16
#define DENSITY_KERNEL nerf_density_bf16_kernel
#define DENSITY_LAUNCH nerf_amd_launch_density_bf16
#endif
#include "mlp16_chain.h"

namespace {

constexpr int SIGMA_LAYER = 8;

// chunk sequence: L0 in one chunk, L1..L7 in four, then of L8 the sigma tile alone -- the folded view of the layer table
// (nerf_layout.h: row tile 16 of L8, its weights and its bias row), which coincides with the plain one below L8
struct SigmaPlan {
    static constexpr int LAYERS = SIGMA_LAYER + 1;   // the sigma tile ends the sequence
    static constexpr bool SAVE = false;
    static constexpr int tpc(int L) { return L == 0 ? 16 : 4; }
    static constexpr int mt(int L) { return fold_mt(L); }
    static constexpr int layer_off_kib(int L) { return fold_layer_off_kib(L); }
    static constexpr int bias_off(int L) { return fold_bias_off(L); }
};
static_assert(NUM_CHUNKS<SigmaPlan> == 30 && plan_fits<SigmaPlan>(), "chunks per tile / weight buffer, parity");
static_assert(tile_mfmas<SigmaPlan>() == 1936, "L0..L7 + the sigma tile of L8");

constexpr int LDS_POSX = LDS_CHAIN_END;
constexpr int LDS_TOTAL = LDS_POSX + WAVES * NCB * 2048;
static_assert(LDS_TOTAL <= 160 * 1024, "LDS budget");

struct State {
    using Plan = SigmaPlan;          // the chain instantiated for this state (mlp16_chain.h)
    ex8 X[NCB][8], Y[NCB][8];        // [column block][k-step of 32]
    f32x4 pend[NCB][2];               // [column block][tile of the pending pair]
    float sigma[NCB];
    bool bad;                         // range guard: a non-finite accumulator was seen
    WFrag* wf;                        // the coming chunk's first weight fragments (outlive a tile)
};

// posx of this lane's two points (nerf_layout::posx_col_f32), exactly as mlp_bf16_16.hip stage_inputs forms them
template <bool GRID>
__device__ __forceinline__ void stage_inputs(const Ctx& c, const DensityArgs& a, long long tile_base) {
    const int col = c.lane & 15, g = c.lane >> 4;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        long long p = tile_base + c.wave * (16 * NCB) + cb * 16 + col;
        if (p >= a.P) p = a.P - 1;                 // lanes past the end use the last point (results dropped)
        float xyz[3];
        if constexpr (GRID) {
            const long long k = p % a.nz, r = p / a.nz;
            const long long j = r % a.ny, i = r / a.ny;
            const long long ijk[3] = {i, j, k};
#pragma unroll
            for (int cd = 0; cd < 3; ++cd) xyz[cd] = add_rn(a.lo[cd], mul_rn((float)ijk[cd], a.step[cd]));
        } else {
            const float* v = a.pts + p * a.stride;
            xyz[0] = v[0]; xyz[1] = v[1]; xyz[2] = v[2];
        }
        float v[16];
#pragma unroll
        for (int cd = 0; cd < 3; ++cd) {
            const TwoF q = to_revolutions(xyz[cd]);
#pragma unroll
            for (int jj = 0; jj < 5; ++jj) v[cd * 5 + jj] = enc_lane(q, 5 * g + jj);
        }
        v[15] = g == 0 ? xyz[0] : g == 1 ? xyz[1] : g == 2 ? xyz[2] : 0.f;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            u32x4 r;
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = pack2<false>(v[8 * e + 2 * i], v[8 * e + 2 * i + 1]);
            lds_store<u32x4>(c.b_posx, cb * 2048 + e * 1024, r);
        }
    }
}

template <bool GRID>
__device__ __forceinline__ void run_tile(const Ctx& c, const DensityArgs& a, long long tile_base, State& st) {
    stage_inputs<GRID>(c, a, tile_base);
    run_layer<0>(c, st, st.X, st.X);
    run_layer<1>(c, st, st.X, st.Y);
    run_layer<2>(c, st, st.Y, st.X);
    run_layer<3>(c, st, st.X, st.Y);
    run_layer<4>(c, st, st.Y, st.X);
    run_layer<5>(c, st, st.X, st.Y);
    run_layer<6>(c, st, st.Y, st.X);
    run_layer<7>(c, st, st.X, st.Y);
    run_layer<8>(c, st, st.Y, st.X);
    epilogue_piece<SIGMA_LAYER, 8>(0, st.pend, st.X, st);     // the sigma tile (pair 8) is still pending
    for (int cb_ = 1; cb_ < NCB; ++cb_) epilogue_piece<SIGMA_LAYER, 8>(4 * cb_, st.pend, st.X, st);
}

template <bool GRID>
__global__ __launch_bounds__(WAVES * 64, WAVES / 4) void DENSITY_KERNEL(DensityArgs a, long long ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    (void)smem;
    using P = SigmaPlan;
    Ctx c;                                              // as mlp_bf16_16.hip kernel_body, without posd
    c.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    c.lane = threadIdx.x & 63;
    const char* img = reinterpret_cast<const char*>(a.packed);
    c.wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(img), 0, (int)B16_IMAGE_BYTES, 0x00020000);
    c.wave_goff = c.wave * 1024;
    c.lane16 = c.lane * 16;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        c.b_wread[p] = LDS_W0 + p * LDS_WBUF + c.lane * 16;
        c.s_wdst[p] = LDS_W0 + p * LDS_WBUF + c.wave * 1024;
    }
    c.b_bias = (c.lane >> 4) * 16;
    c.b_posx = LDS_POSX + c.wave * (NCB * 2048) + c.lane * 16;
    {
        const float* bsrc = reinterpret_cast<const float*>(img + (long long)B16_WEIGHT_KIB * 1024);
        for (int i = threadIdx.x; i < B16_BIAS_FLOATS; i += WAVES * 64) lds_store<float>(i * 4, LDS_BIAS, bsrc[i]);
        Stage<P, NUM_CHUNKS<P> - 1>::issue(c);         // chunk 0
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    WFrag wf;
    {
        constexpr int F0 = chunk_tiles<P>(0) * (layer_desc(0).chain_k / 32 + layer_desc(0).extra_slots / 32);
#pragma unroll
        for (int f = 0; f < 4 && f < F0; ++f) wf.a[f] = lds_load<ex8>(c.b_wread[0], f * 1024);
        wf.bias0 = lds_load<f32x4>(c.b_bias, LDS_BIAS + P::bias_off(0) * 4);
    }
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long tile_base = tile * TILE_PTS;
        asm volatile("" : "+s"(c.wave_goff));
        State st;
        st.wf = &wf;
        st.bad = false;
        run_tile<GRID>(c, a, tile_base, st);
        bool bad = st.bad;
        if (c.lane < 16) {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const long long p = tile_base + c.wave * (16 * NCB) + cb * 16 + c.lane;
                if (p < a.P) {
                    a.sigma[p] = st.sigma[cb];
                    bad |= !(__builtin_fabsf(st.sigma[cb]) < __builtin_inff());
                }
            }
        }
        flag_nonfinite(c, bad);
    }
}

}  // namespace

// grid mode: a.pts == NULL (a.ny, a.nz, a.lo, a.step describe the grid); points mode: a.pts, a.stride
extern "C" int DENSITY_LAUNCH(const DensityArgs* args, hipStream_t stream) {
    (void)hipGetLastError();
    const DensityArgs a = *args;
    if (a.P <= 0) return 0;
    const long long ntiles = (a.P + TILE_PTS - 1) / TILE_PTS;
    const int cus = device_cus();
    const long long grid = ntiles < cus ? ntiles : cus;
    auto kern = a.pts ? DENSITY_KERNEL<false> : DENSITY_KERNEL<true>;
    const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(kern), LDS_TOTAL);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(WAVES * 64), LDS_TOTAL, stream, a, ntiles);
    return (int)hipGetLastError();
}

#ifndef NERF_HALF
// ---- grid points for the fp32 fallback (built once, with the bf16 kernel) ---------------------------------------------
// pts6[n, 6] = (x(i), y(j), z(k), 0, 0, 1) of grid points first .. first + n - 1, the coordinates formed as the density
// kernel forms them; the existing forward then runs on them (nerf_amd_mlp_forward, or the layer-by-layer path of other
// network sizes)
namespace {
__global__ __launch_bounds__(256) void nerf_grid_points_kernel(DensityArgs a, long long first, long long n, float* pts6) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const long long p = first + q;
    const long long k = p % a.nz, r = p / a.nz;
    const long long j = r % a.ny, i = r / a.ny;
    float* o = pts6 + q * 6;
    o[0] = add_rn(a.lo[0], mul_rn((float)i, a.step[0]));
    o[1] = add_rn(a.lo[1], mul_rn((float)j, a.step[1]));
    o[2] = add_rn(a.lo[2], mul_rn((float)k, a.step[2]));
    o[3] = 0.f;
    o[4] = 0.f;
    o[5] = 1.f;
}
}  // namespace

extern "C" int nerf_amd_launch_grid_points(const DensityArgs* args, long long first, long long n, float* pts6, hipStream_t stream) {
    (void)hipGetLastError();
    if (n <= 0) return 0;
    hipLaunchKernelGGL(nerf_grid_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, *args, first, n, pts6);
    return (int)hipGetLastError();
}
#endif
