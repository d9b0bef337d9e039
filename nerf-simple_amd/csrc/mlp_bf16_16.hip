// mlp_bf16_16.hip -- the fused 16-bit MLP: sampling + positional encoding + 12 dense layers in
// one launch, on v_mfma_f32_16x16x32_bf16 (and, built with -DNERF_HALF, on ..._f16).
// Replaces reference utils/rendering.py:24-40 + utils/xyz.py:6-36 + utils/nets.py:34-43.
//
// H^T = W . X^T: output features on MFMA rows, points on MFMA columns / lanes (nerf_layout.h).
// The MFMA chain itself -- the chunk sequence, chunk_step and its schedule, the epilogues, the range flag -- is
// mlp16_chain.h, shared with density.hip; its header describes it.  This file is the chain's full instantiation:
//   * the plan: all 11 layers, weight chunks of four 16-row tiles (eight for the K = 64 first layer): 38 chunks per
//     tile, 34 in fp16;
//   * the sigma head rides as row 256 of the layers_2 product, the rgb head is one 16-row tile; the fp16 build
//     has no layers_2 product (folded into the colour layer by the packer) and keeps that row's tile as layer 8;
//   * a workgroup = 8 waves = a 256-point tile, persistent over tiles;
//   * the inputs of a tile (stage_inputs): sampling along the rays or explicit points, jitter, posx and the direction
//     features; SAVE: the training forward, which also stores every layer's activations and ReLU masks;
//   * COMP (the render path): compositing (utils/rendering.py:47-85) runs in the same launch.  A
//     workgroup owns a contiguous range of RAYS; each tile drops its 256 x (rgb, sigma, t) into an
//     LDS ring of 1024 samples, and whenever 8 rays are complete (or the ring is full) every wave
//     composites one ray with the routine composite.hip uses (composite_device.h): bit-identical
//     pixels, and raw[B,N,4] / ts[B,N] (20 B per sample) never go to HBM.
// The chip is power/DVFS-limited on this kernel and holds a higher clock on the 16x16x32 shape
// than on 32x32x16 at equal cycles per FLOP (MI355X_MICROARCH.md, DVFS give-back item 7).
#include "composite_device.h"
#include "launchers.h"

using namespace nerf_layout;

// The same source builds the bf16 kernel (default) and, with -DNERF_HALF, the
// fp16 one (v_mfma_f32_16x16x32_f16: same cycles, 11-bit mantissa instead of 8).
#ifdef NERF_HALF
typedef _Float16 elem_t;
#define NERF_MFMA __builtin_amdgcn_mfma_f32_16x16x32_f16
#define NERF_KERNEL nerf_mlp_f16_16_kernel
#define NERF_LAUNCH nerf_amd_launch_mlp_f16_16
#else
typedef __bf16 elem_t;
#define NERF_MFMA __builtin_amdgcn_mfma_f32_16x16x32_bf16
#define NERF_KERNEL nerf_mlp_bf16_16_kernel
#define NERF_LAUNCH nerf_amd_launch_mlp_bf16_16
#endif
#include "mlp16_chain.h"

namespace {

// The fp16 build runs the folded view of the layer table (nerf_layout.h): layer 8 is its sigma tile alone (one 8 KiB
// chunk, 16 MFMAs) and the colour layer takes h8 through the pre-multiplied Wc[:, :256] W2 -- layers_2's 256 MFMAs and
// four of its five chunk barriers are gone, 2088 MFMAs and 34 chunks per tile.  The bf16 build, whose image and
// instantiations are shared with training (h9 is saved for dW), runs the table as it stands.
#ifdef NERF_HALF
constexpr bool FOLD = true;
#else
constexpr bool FOLD = false;
#endif
struct MlpPlan {
    static constexpr int LAYERS = NUM_LAYERS;
    static constexpr bool SAVE = !FOLD;              // the training forward exists in bf16 only
    // 16-row output tiles per weight chunk: 4 (64 rows, 8..40 KiB), and 8 for the K = 64 first layer, whose
    // tiles are two fragments each (one barrier per 16 MFMAs otherwise).  The chunk count stays even.
    static constexpr int tpc(int L) { return L == 0 ? 8 : 4; }
    // the 16-row tiles of layer L this build streams, where they start in the image and in the bias table
    static constexpr int mt(int L) { return FOLD ? fold_mt(L) : b16_mt(L); }
    static constexpr int layer_off_kib(int L) { return FOLD ? fold_layer_off_kib(L) : b16_layer_off_kib(L); }
    static constexpr int bias_off(int L) { return FOLD ? fold_bias_off(L) : b16_bias_off(L); }
};
static_assert(NUM_CHUNKS<MlpPlan> == (FOLD ? 34 : 38) && plan_fits<MlpPlan>(), "chunks per tile / weight buffer, parity");

constexpr int LDS_POSD = LDS_CHAIN_END;
constexpr int LDS_POSX = LDS_POSD + WAVES * NCB * 1024;
constexpr int LDS_TOTAL = LDS_POSX + WAVES * NCB * 2048;
// COMP only: the sample ring behind everything else (16 B + 4 B per sample)
constexpr int RING_PTS = 1024;
constexpr int LDS_RING_RAW = LDS_TOTAL;
constexpr int LDS_RING_T = LDS_RING_RAW + RING_PTS * 16;
constexpr int LDS_TOTAL_COMP = LDS_RING_T + RING_PTS * 4;
constexpr int COMP_MAX_N = RING_PTS - TILE_PTS;      // an unfinished ray plus one more tile must fit
static_assert(COMP_MAX_N == FUSED_RENDER_MAX_N, "api.hip routes by this limit");
static_assert(LDS_TOTAL_COMP <= 160 * 1024, "LDS budget");
static_assert((RING_PTS & (RING_PTS - 1)) == 0 && RING_PTS % TILE_PTS == 0, "ring indexing");

static_assert(ACT_TILE_PTS == TILE_PTS && MASK_TILE_PTS == TILE_PTS, "activation blocks and mask tiles are the kernel's tiles");

struct State {
    using Plan = MlpPlan;            // the chain instantiated for this state (mlp16_chain.h)
    ex8 X[NCB][8], Y[NCB][8];        // [column block][k-step of 32]
    f32x4 pend[NCB][2];               // [column block][tile of the pending pair]
    float sigma[NCB], rgb[NCB][3];
    bool bad;                         // range guard: a non-finite accumulator was seen (flag_nonfinite)
    unsigned posd_off[NCB];           // LDS address of this lane's direction fragment (stage_inputs)
    // training forward only (SAVE): where this lane's activations go
    char* acts;
    long long P;
    long long tile;                   // tile index (uniform)
    int loff[NCB];                    // block_lane_offset(lane>>4, point in tile): this lane's granule of
                                      // fragment 0 in the tile's activation block; LOFF_INVALID past the end
    unsigned mb[NCB][2];              // ReLU mask bits being collected [column block][pair group]
    float amax[4];                    // 8-bit storage form: running maximum of the fragment group being finished, by (layer, group) parity
    long long mask_tile;              // byte offset of this tile's dword 0 of layer 0 (nerf_layout::mask_offset_bytes), uniform
    // fused render only (COMP)
    long long p_end;                  // one past this workgroup's last point (uniform)
    unsigned ring_q0;                 // ring slot of the tile's point 0 (uniform)
    WFrag* wf;                        // the coming chunk's first weight fragments (outlive a tile)
};

// SAVE (the training forward, launched in rays mode) also serves Nerf.forward(v) with gradients:
// a.pts != NULL switches the point fetch at run time, so training needs no third instantiation.
template <bool RAYS, int SAVE, bool COMP>
__device__ __forceinline__ void stage_inputs(const Ctx& c, const MlpArgs& a, long long tile_base, State& st) {
    const int col = c.lane & 15, g = c.lane >> 4;
    // Counter-RNG jitter: the four lane groups of a point would each evaluate the same Philox
    // (40 quarter-rate integer multiplies), once per column block.  Instead every lane evaluates
    // it once, for point (lane & 31) of the wave's 32, and the lanes fetch their two points'
    // draws with a wave shuffle: the same numbers for half the work.
    float u_mine = 0.f;
    bool dev_rng = false;
    long long b0 = 0;                                   // divmod(tile_base, N): wave-uniform, once per tile
    int r0 = 0;
    if constexpr (RAYS) {
        b0 = tile_base / a.N;
        r0 = (int)(tile_base - b0 * a.N);
    }
    const long long p_end = COMP ? st.p_end : a.P;
    const int last_local = (int)(p_end - 1 - tile_base);  // lanes past the end use the last point (results dropped)
    // The direction features (posd: 24 sines / cosines, 3 raw coordinates) belong to the RAY:
    // in rays mode they are evaluated once per ray of the tile -- one LDS slot of 64 B per ray, value (group g, slot s)
    // by thread 32 * ray + 8 g + s, two rays per tile at N = 128 -- instead of once per sample, and with them goes
    // the per-sample normalisation of the direction (a square root and three exact divisions).  Every lane then
    // reads its ray's 16-byte fragment (a broadcast within the 16 points of a column block).  Same operations per
    // value as the per-sample form: bit-identical features.  (The training forward keeps the per-sample form: it
    // also serves explicit points, whose directions are per point.)
    constexpr bool RAY_POSD = RAYS && !SAVE;
    if constexpr (RAY_POSD) {
        const int top = last_local < TILE_PTS - 1 ? last_local : TILE_PTS - 1;
        const int nrays = (int)(split_point(b0, r0, top, a.N).b - b0) + 1;          // rays this tile touches (uniform)
        for (int idx = threadIdx.x; idx < nrays * 32; idx += WAVES * 64) {
            const int ray = idx >> 5, slot = idx & 31, gg = slot >> 3, sl = slot & 7;
            const float* rp = a.rays + (b0 + ray) * 6 + 3;
            const float dx = rp[0], dy = rp[1], dz = rp[2];
            const float nrm = norm3(dx, dy, dz);              // as fetch_point_rays normalises: torch.norm bit for bit
            float val = 0.f;
            if (sl < 6) {                                     // posd_col_f32: per coordinate the pair (level g, trig)
                const int cd = sl >> 1;
                const float dc = __fdiv_rn(cd == 0 ? dx : cd == 1 ? dy : dz, nrm);
                val = enc_lane(to_revolutions(dc), 2 * gg + (sl & 1));
            } else if (sl == 6 && gg < 3) {
                val = __fdiv_rn(gg == 0 ? dx : gg == 1 ? dy : dz, nrm);
            }
            lds_store<elem_t>(LDS_POSD + ray * 64 + slot * 2, 0, (elem_t)val);
        }
    }
    if constexpr (RAYS && NCB == 2) {
        dev_rng = (a.flags & NERF_FLAG_DEVICE_RNG) && !(a.flags & NERF_FLAG_TS_GIVEN);
        if (dev_rng) {
            int lm = c.wave * 32 + (c.lane & 31);
            if (lm > last_local) lm = last_local;
            u_mine = device_rng_uniform(a, split_point(b0, r0, lm, a.N));
        }
    }
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        long long p = tile_base + c.wave * (16 * NCB) + cb * 16 + col;
        const bool valid = p < p_end;
        st.loff[cb] = valid ? block_lane_offset(g, c.wave * (16 * NCB) + cb * 16 + col) : LOFF_INVALID;
        if constexpr (SAVE == 2) {
            // 8-bit form: after store_fragment_f8's transpose the lane writes the granule of point 16 (lane >> 5) + col of
            // the wave, not of its own two points
            if (cb == 0)
                st.loff[0] = tile_base + c.wave * 32 + 16 * (c.lane >> 5) + col < p_end ? f8_lane_offset(c.lane, c.wave) : LOFF_INVALID;
        }
        if (!valid) p = p_end - 1;
        PointIn pt;
        st.posd_off[cb] = c.b_posd + cb * 1024;              // per-sample form: this lane's own fragment
        if constexpr (RAYS) {
            const float u_cb = (NCB == 2) ? __shfl(u_mine, cb * 16 + col) : 0.f;
            int lp = c.wave * (16 * NCB) + cb * 16 + col;
            if (lp > last_local) lp = last_local;
            if (SAVE && a.pts) {
                pt = fetch_point_pts(a, p);
            } else {
                const RaySample rs = split_point(b0, r0, lp, a.N);
                if constexpr (RAY_POSD) st.posd_off[cb] = LDS_POSD + (unsigned)(rs.b - b0) * 64 + g * 16;
                pt = fetch_point_rays<!RAY_POSD>(a, p, rs, u_cb, dev_rng);
                if constexpr (COMP) {
                    if (valid && g == 0)
                        lds_store<float>(((st.ring_q0 + c.wave * (16 * NCB) + cb * 16 + col) & (RING_PTS - 1)) * 4, LDS_RING_T, pt.t);
                }
                if (valid && g == 0 && a.ts_out) a.ts_out[p] = pt.t;
            }
        } else {
            pt = fetch_point_pts(a, p);
        }
        {   // posx: 16 slots per lane group (nerf_layout::posx_col_f32)
            const float xyz[3] = {pt.x, pt.y, pt.z};
            float v[16];
#pragma unroll
            for (int cd = 0; cd < 3; ++cd) {
                const TwoF q = to_revolutions(xyz[cd]);
#pragma unroll
                for (int jj = 0; jj < 5; ++jj) v[cd * 5 + jj] = enc_lane(q, 5 * g + jj);
            }
            v[15] = g == 0 ? pt.x : g == 1 ? pt.y : g == 2 ? pt.z : 0.f;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                u32x4 r;
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = pack2<false>(v[8 * e + 2 * i], v[8 * e + 2 * i + 1]);
                lds_store<u32x4>(c.b_posx, cb * 2048 + e * 1024, r);
            }
        }
        if constexpr (!RAY_POSD) {   // posd: 8 slots per lane group (nerf_layout::posd_col_f32)
            const float dd[3] = {pt.d1, pt.d2, pt.d3};
            float v[8];
#pragma unroll
            for (int cd = 0; cd < 3; ++cd) {
                const TwoF q = to_revolutions(dd[cd]);
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) v[cd * 2 + jj] = enc_lane(q, 2 * g + jj);
            }
            v[6] = g == 0 ? pt.d1 : g == 1 ? pt.d2 : g == 2 ? pt.d3 : 0.f;
            v[7] = 0.f;
            u32x4 r;
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = pack2<false>(v[2 * i], v[2 * i + 1]);
            lds_store<u32x4>(c.b_posd, cb * 1024, r);
        }
    }
}

// one tile: prologue (sampling / RNG / encoding into LDS) + the 11 layers; leaves st.rgb / st.sigma
template <bool RAYS, int SAVE, bool COMP>
__device__ __forceinline__ void run_tile(const Ctx& c, const MlpArgs& a, long long tile_base, State& st) {
    stage_inputs<RAYS, SAVE, COMP>(c, a, tile_base, st);
    run_layer<0, SAVE>(c, st, st.X, st.X);
    run_layer<1, SAVE>(c, st, st.X, st.Y);
    run_layer<2, SAVE>(c, st, st.Y, st.X);
    run_layer<3, SAVE>(c, st, st.X, st.Y);
    run_layer<4, SAVE>(c, st, st.Y, st.X);
    run_layer<5, SAVE>(c, st, st.X, st.Y);
    run_layer<6, SAVE>(c, st, st.Y, st.X);
    run_layer<7, SAVE>(c, st, st.X, st.Y);
    // folded (fp16): layer 8 is the sigma tile alone and writes no fragment, the colour layer reads h8 where layer 7 left it
    ex8 (&c_in)[NCB][8] = FOLD ? st.Y : st.X;
    ex8 (&c_out)[NCB][8] = FOLD ? st.X : st.Y;
    run_layer<8, SAVE>(c, st, st.Y, st.X);
    run_layer<9, SAVE>(c, st, c_in, c_out);
    run_layer<10, SAVE>(c, st, c_out, c_in);
    epilogue_piece<10, 0>(0, st.pend, st.X, st);     // the rgb tile is still pending
    for (int cb_ = 1; cb_ < NCB; ++cb_) epilogue_piece<10, 0>(4 * cb_, st.pend, st.X, st);
}

__device__ __forceinline__ bool finite4(float x, float y, float z, float w) {
    // |v| < inf is false for inf and NaN; the sum is non-finite iff any term is (no finite sum of four floats overflows
    // unless a term is already beyond half of FLT_MAX -- which fp16 / bf16 MLP outputs of a usable network never are)
    return __builtin_fabsf(x) + __builtin_fabsf(y) + __builtin_fabsf(z) + __builtin_fabsf(w) < __builtin_inff();
}

struct RingSamples {                         // a ray's samples in the workgroup's LDS ring
    unsigned q0;                              // ring slot of its sample 0
    __device__ __forceinline__ float t(int i) const {
        return lds_load<float>(((q0 + (unsigned)i) & (RING_PTS - 1)) * 4, LDS_RING_T);
    }
    __device__ __forceinline__ f32x4 c(int i) const {
        return lds_load<f32x4>(((q0 + (unsigned)i) & (RING_PTS - 1)) * 16, LDS_RING_RAW);
    }
};

template <bool RAYS, int SAVE, bool COMP>
__device__ __forceinline__ void kernel_body(const MlpArgs& a, long long ntiles) {
    static_assert(!COMP || (RAYS && !SAVE), "the fused render is the rays-mode inference kernel");
    using P = MlpPlan;
    Ctx c;
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
    c.b_posd = LDS_POSD + c.wave * (NCB * 1024) + c.lane * 16;

    {
        const float* bsrc = reinterpret_cast<const float*>(img + (long long)B16_WEIGHT_KIB * 1024);
        for (int i = threadIdx.x; i < B16_BIAS_FLOATS; i += WAVES * 64)
            lds_store<float>(i * 4, LDS_BIAS, bsrc[i]);
        Stage<P, NUM_CHUNKS<P> - 1>::issue(c);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's LDS-DMA pieces have landed
    __syncthreads();
    WFrag wf;                                           // chunk 0's first fragments (chunk_step hands them on)
    {
        constexpr int F0 = chunk_tiles<P>(0) * (layer_desc(0).chain_k / 32 + layer_desc(0).extra_slots / 32);
#pragma unroll
        for (int f = 0; f < 4 && f < F0; ++f) wf.a[f] = lds_load<ex8>(c.b_wread[0], f * 1024);
        wf.bias0 = lds_load<f32x4>(c.b_bias, LDS_BIAS + P::bias_off(0) * 4);
    }

    if constexpr (!COMP) {
        for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
            const long long tile_base = tile * TILE_PTS;
            asm volatile("" : "+s"(c.wave_goff));
            State st;
            st.wf = &wf;
            st.acts = reinterpret_cast<char*>(a.acts);
            st.P = a.P;
            st.mask_tile = SAVE == 2 ? f8_mask_offset_bytes(0, tile, 0, a.P) : mask_offset_bytes(0, tile, 0, a.P);
            st.tile = tile;
            st.bad = false;
            run_tile<RAYS, SAVE, false>(c, a, tile_base, st);
            bool bad = st.bad;
            if (c.lane < 16) {
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    const long long p = tile_base + c.wave * (16 * NCB) + cb * 16 + c.lane;
                    if (p < a.P) {
                        const f32x4 o = {st.rgb[cb][0], st.rgb[cb][1], st.rgb[cb][2], st.sigma[cb]};
                        *reinterpret_cast<f32x4*>(a.raw + p * 4) = o;
                        bad |= !finite4(o[0], o[1], o[2], o[3]);
                    }
                }
            }
            flag_nonfinite(c, bad);
        }
    } else {
        // ---- fused render: this workgroup's contiguous range of rays, tile after tile ----------
        const long long B = a.P / a.N;
        const long long r_lo = (long long)blockIdx.x * B / gridDim.x, r_hi = ((long long)blockIdx.x + 1) * B / gridDim.x;
        const long long range_base = r_lo * a.N;
        const int n_pts = (int)((r_hi - r_lo) * a.N);                 // < 2^31: the launcher returns -2 otherwise
        const nerf_composite::RayOut out{a.rgb, a.disp, a.alpha, a.acc, a.w, a.pixels};
        int next_ray = 0, n_complete = 0;                             // rays composited / completely in the ring (uniform)
        for (int q_tile = 0; q_tile < n_pts; q_tile += TILE_PTS) {
            const long long tile_base = range_base + q_tile;
            asm volatile("" : "+s"(c.wave_goff));
            State st;
            st.wf = &wf;
            st.acts = nullptr;
            st.P = a.P;
            st.mask_tile = 0;
            st.tile = 0;
            st.p_end = range_base + n_pts;
            st.ring_q0 = (unsigned)q_tile & (RING_PTS - 1);
            st.bad = false;
            run_tile<true, false, true>(c, a, tile_base, st);
            bool bad = st.bad;
            if (c.lane < 16) {
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    const int local = c.wave * (16 * NCB) + cb * 16 + c.lane;
                    if (q_tile + local < n_pts) {
                        const f32x4 o = {st.rgb[cb][0], st.rgb[cb][1], st.rgb[cb][2], st.sigma[cb]};
                        lds_store<f32x4>(((st.ring_q0 + local) & (RING_PTS - 1)) * 16, LDS_RING_RAW, o);
                        bad |= !finite4(o[0], o[1], o[2], o[3]);
                    }
                }
            }
            flag_nonfinite(c, bad);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                             // every wave's samples of this tile are in the ring
            asm volatile("" ::: "memory");
            const int done_q = q_tile + TILE_PTS < n_pts ? q_tile + TILE_PTS : n_pts;
            while ((n_complete + 1) * a.N <= done_q) ++n_complete;
            // composite when every wave has a ray, when the ring could not take another tile, or at the end
            if (n_complete - next_ray >= WAVES || done_q + TILE_PTS - next_ray * a.N > RING_PTS || done_q == n_pts) {
                for (int ray = next_ray + c.wave; ray < n_complete; ray += WAVES) {
                    const long long gray = r_lo + ray;
                    const float* d = a.rays + gray * 6 + 3;
                    const float dnorm = nerf_composite::unit_dir_norm(d[0], d[1], d[2], true);
                    const RingSamples src{(unsigned)(ray * a.N) & (RING_PTS - 1)};
                    nerf_composite::composite_ray(src, a.N, c.lane, dnorm, gray, out);
                }
                next_ray = n_complete;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                         // the next tile's prologue rewrites ring slots read above
                asm volatile("" ::: "memory");
            }
        }
    }
}

template <bool RAYS, bool SAVE, bool COMP>
__global__ __launch_bounds__(WAVES * 64, WAVES / 4) void NERF_KERNEL(MlpArgs a, long long ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    (void)smem;
    kernel_body<RAYS, SAVE ? 1 : 0, COMP>(a, ntiles);
}
#ifndef NERF_HALF
// the training forward with the 8-bit storage form of the saved activations (nerf_layout.h; MlpArgs::flags bit
// NERF_FLAG_STORE_E4M3): a kernel of its own name, so the bf16-storage instantiations keep theirs
__global__ __launch_bounds__(WAVES * 64, WAVES / 4) void nerf_mlp_train_e4m3_kernel(MlpArgs a, long long ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    (void)smem;
    kernel_body<true, 2, false>(a, ntiles);
}
#endif

}  // namespace

extern "C" int NERF_LAUNCH(const MlpArgs* args, int rays_mode, hipStream_t stream) {
    (void)hipGetLastError();
    MlpArgs a = *args;
    if (a.P <= 0) return 0;
    const long long ntiles = (a.P + TILE_PTS - 1) / TILE_PTS;
    const int cus = device_cus();
    const long long grid = ntiles < cus ? ntiles : cus;
    hipError_t e = hipSuccess;
    const bool comp = a.rgb || a.disp || a.acc || a.alpha || a.w || a.pixels;
    if (comp) {
        // fused render: rays mode, inference; a ray plus one tile must fit the LDS ring, and a
        // workgroup's share of the points must fit an int
        if (!rays_mode || a.acts || a.N > COMP_MAX_N || a.P / grid + a.N >= (1ll << 31)) return -2;
        auto kern = NERF_KERNEL<true, false, true>;
        e = allow_dynamic_lds(reinterpret_cast<const void*>(kern), LDS_TOTAL_COMP);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(WAVES * 64), LDS_TOTAL_COMP, stream, a, ntiles);
        return (int)hipGetLastError();
    }
#ifdef NERF_HALF
    if (a.acts) return -2;                       // the training forward exists in bf16 only
    auto kern = rays_mode ? NERF_KERNEL<true, false, false> : NERF_KERNEL<false, false, false>;
#else
    if (a.acts && !rays_mode) return -2;          // the training forward is the rays-mode instantiation (a.pts selects points)
    if ((a.flags & NERF_FLAG_STORE_E4M3) && !a.acts) return -2;
    auto kern = a.acts ? ((a.flags & NERF_FLAG_STORE_E4M3) ? nerf_mlp_train_e4m3_kernel : NERF_KERNEL<true, true, false>)
                       : (rays_mode ? NERF_KERNEL<true, false, false> : NERF_KERNEL<false, false, false>);
#endif
    e = allow_dynamic_lds(reinterpret_cast<const void*>(kern), LDS_TOTAL);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(WAVES * 64), LDS_TOTAL, stream, a, ntiles);
    return (int)hipGetLastError();
}
