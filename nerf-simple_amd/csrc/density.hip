// density.hip -- the sigma-only network: raw sigma of query points or of a grid generated in the kernel, on
// v_mfma_f32_16x16x32_bf16 (and, built with -DNERF_HALF, on ..._f16).  Not in the reference (its only way to sigma is the
// whole Nerf.forward, reference utils/nets.py:34-43).
//
// sigma does not depend on the view direction: sigma_fc reads h8 before the direction concat (reference utils/nets.py:36-40).
// The sigma network is therefore internal layers L0..L7 and the one 16-row tile of L8 that holds row 256 (nerf_layout.h):
// 1936 of the 2344 MFMAs of a wave-tile (82.6 %), no direction features, no colour layers.  It runs on the packed 16-bit
// image of nerf_amd_pack_weights with the arithmetic of mlp_bf16_16.hip: the same fragment order, bias-initialised
// accumulators, k-step order, ReLU / pack conversion and in-kernel encoder (to_revolutions, enc_lane) -- so sigma equals
// column 3 of nerf_amd_mlp_forward's output on the same points bit for bit.
//
// The schedule is mlp_bf16_16.hip's inference schedule on a shorter chunk sequence: 30 chunks per 256-point tile
//   L0 (16 tiles, K = 64: one chunk) | L1..L7 (4 chunks of four 16-row tiles each) | the sigma tile of L8 (one chunk);
// weights stream L2 -> LDS by LDS-DMA, double buffered (an even chunk count keeps the buffer parity cyclic over tiles),
// one barrier per chunk three fragments before its end; a workgroup = 8 waves = 256 points, persistent over tiles.
// Inputs: explicit points (any row stride >= 3) or grid point p of an [Rx, Ry, Rz] grid (C order, z fastest) with
// coordinates x_a(i) = fl(lo_a + fl(i s_a)), formed here -- no input buffer.
#include "nerf_device.h"
#include <utility>

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
typedef elem_t ex8 __attribute__((ext_vector_type(8)));
typedef elem_t ex2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int NCB = 2;
constexpr int WAVES = 16 / NCB;
constexpr int TILE_PTS = WAVES * 16 * NCB;
constexpr int SIGMA_LAYER = 8;
constexpr int SIGMA_TILE = 16;                    // L8's 16-row tile that holds row 256 (sigma_fc)

// chunk sequence: L0 in one chunk, L1..L7 in four, the sigma tile of L8 in one
__host__ __device__ constexpr int tpc(int L) { return L == 0 ? 16 : 4; }
__host__ __device__ constexpr int layer_chunks(int L) { return L == SIGMA_LAYER ? 1 : (b16_mt(L) + tpc(L) - 1) / tpc(L); }
__host__ __device__ constexpr int chunk_first(int L) {
    int c = 0;
    for (int i = 0; i < L; ++i) c += layer_chunks(i);
    return c;
}
constexpr int NUM_CHUNKS = chunk_first(SIGMA_LAYER + 1);      // 30
__host__ __device__ constexpr int chunk_layer(int cc) {
    int L = 0;
    while (cc >= layer_chunks(L)) { cc -= layer_chunks(L); ++L; }
    return L;
}
// first 16-row tile of chunk C of layer L
__host__ __device__ constexpr int chunk_rt0(int L, int C) { return L == SIGMA_LAYER ? SIGMA_TILE : C * tpc(L); }
__host__ __device__ constexpr int chunk_tiles(int cc) {
    const int L = chunk_layer(cc), C = cc - chunk_first(L);
    if (L == SIGMA_LAYER) return 1;
    const int left = b16_mt(L) - C * tpc(L);
    return left < tpc(L) ? left : tpc(L);
}
__host__ __device__ constexpr int chunk_kib(int cc) { return chunk_tiles(cc) * b16_ks(chunk_layer(cc)); }
__host__ __device__ constexpr int chunk_off_kib(int cc) {
    const int L = chunk_layer(cc), C = cc - chunk_first(L);
    return b16_layer_off_kib(L) + chunk_rt0(L, C) * b16_ks(L);
}
__host__ __device__ constexpr int sigma_mfmas_per_wave_tile() {
    int m = 0;
    for (int cc = 0; cc < NUM_CHUNKS; ++cc) m += chunk_tiles(cc) * b16_ks(chunk_layer(cc)) * NCB;
    return m;
}
static_assert(NUM_CHUNKS == 30 && NUM_CHUNKS % 2 == 0, "the double buffer's parity is cyclic over tiles");
static_assert(sigma_mfmas_per_wave_tile() == 1936, "L0..L7 + the sigma tile of L8");

constexpr int LDS_WBUF = 40 * 1024;
constexpr int LDS_BIAS = 0;
constexpr int LDS_W0 = 10 * 1024;
constexpr int LDS_POSX = LDS_W0 + 2 * LDS_WBUF;
constexpr int LDS_TOTAL = LDS_POSX + WAVES * NCB * 2048;
static_assert(B16_BIAS_FLOATS * 4 <= LDS_W0, "bias table");
static_assert(LDS_TOTAL <= 160 * 1024, "LDS budget");
__host__ __device__ constexpr bool chunks_fit() {
    for (int cc = 0; cc < NUM_CHUNKS; ++cc)
        if (chunk_kib(cc) * 1024 > LDS_WBUF) return false;
    return true;
}
static_assert(chunks_fit(), "a chunk fits its weight buffer");

typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(3))) void lds_void;
template <class T>
__device__ __forceinline__ T lds_load(unsigned base, int imm) {
    return *reinterpret_cast<const __attribute__((address_space(3))) T*>(reinterpret_cast<lds_char*>(0) + base + imm);
}
template <class T>
__device__ __forceinline__ void lds_store(unsigned base, int imm, const T& v) {
    *reinterpret_cast<__attribute__((address_space(3))) T*>(reinterpret_cast<lds_char*>(0) + base + imm) = v;
}

struct Ctx {
    __amdgpu_buffer_rsrc_t wrsrc;
    unsigned wave_goff, lane16;
    unsigned b_wread[2];            // weight buffer p + lane*16
    unsigned s_wdst[2];             // this wave's DMA piece in weight buffer p (wave-uniform)
    unsigned b_bias;                // (lane>>4)*16
    unsigned b_posx;
    int wave, lane;
};

struct WFrag {
    ex8 a[4];
    f32x4 bias0;
};

struct State {
    ex8 X[NCB][8], Y[NCB][8];        // [column block][k-step of 32]
    f32x4 pend[NCB][2];               // [column block][tile of the pending pair]
    float sigma[NCB];
    bool bad;                         // range guard: a non-finite accumulator was seen
    WFrag* wf;                        // the coming chunk's first weight fragments (outlive a tile)
};

template <bool RELU>
__device__ __forceinline__ unsigned pack2(float a, float b) {
    const f32x2 v = {a, b};
    const ex2 r = __builtin_convertvector(v, ex2);
    if constexpr (RELU) {
        const s16x2 z = {0, 0};
        return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, r), z));
    } else {
        return __builtin_bit_cast(unsigned, r);
    }
}

template <int CC>
struct Stage {
    static constexpr int NEXT = (CC + 1) % NUM_CHUNKS;
    static constexpr int PIECES = (chunk_kib(NEXT) + WAVES - 1) / WAVES;
    static constexpr int SRC_OFF = chunk_off_kib(NEXT) * 1024;
    static __device__ __forceinline__ void issue_piece(const Ctx& c, int p) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            c.wrsrc, reinterpret_cast<lds_void*>(reinterpret_cast<lds_char*>(0) + c.s_wdst[NEXT & 1] + p * (WAVES * 1024)), 16,
            c.lane16, c.wave_goff + (SRC_OFF + p * WAVES * 1024), 0, 0);
    }
    static __device__ __forceinline__ void issue(const Ctx& c) {
#pragma unroll
        for (int p = 0; p < PIECES; ++p) issue_piece(c, p);
    }
};

// One of the 8 pieces of the epilogue of row-tile pair Q of layer L (mlp_bf16_16.hip epilogue_piece without the
// training-forward stores): piece i -> column block i>>2, word i&3 of the next layer's fragment Q.  (L8, Q = 8) is the
// lone sigma tile.
template <int L, int Q>
__device__ __forceinline__ void epilogue_piece(int i, const f32x4 (&acc)[NCB][2], ex8 (&dst)[NCB][8], State& st) {
    constexpr LayerDesc D = layer_desc(L);
    const int cb = i >> 2, j2 = i & 3;
    if constexpr (Q == 0 && L >= 1 && L <= 7) {
        // range guard, as in mlp_bf16_16.hip: an inf input feature makes every row of the layer non-finite
        if (j2 == 0) st.bad |= __builtin_amdgcn_classf(acc[cb][0][0], 0x207);      // sNaN | qNaN | -inf | +inf
    }
    if constexpr (L == SIGMA_LAYER) {
        static_assert(Q == SIGMA_TILE / 2, "only the sigma tile of L8 runs here");
        if (j2 == 0) st.sigma[cb] = acc[cb][0][0];
    } else {
        u32x4 w = __builtin_bit_cast(u32x4, dst[cb][Q]);
        w[j2] = pack2<D.relu != 0>(acc[cb][j2 >> 1][2 * (j2 & 1)], acc[cb][j2 >> 1][2 * (j2 & 1) + 1]);
        dst[cb][Q] = __builtin_bit_cast(ex8, w);
    }
}

template <int L, int P0, int N, int J = 0>
__device__ __forceinline__ void in_chunk_epilogue(int j, int i, const f32x4 (&acc)[NCB][2], ex8 (&dst)[NCB][8], State& st) {
    if constexpr (J < N) {
        if (j == J) epilogue_piece<L, P0 + J>(i, acc, dst, st);
        else in_chunk_epilogue<L, P0, N, J + 1>(j, i, acc, dst, st);
    }
}

// ---- one chunk: NT 16-row tiles of layer L starting at tile chunk_rt0(L, C) (mlp_bf16_16.hip chunk_step, inference form)
// PL/PQ: layer / pair of the pending accumulators handed over by the previous chunk.
template <int L, int C, int PL, int PQ>
__device__ __forceinline__ void chunk_step(const Ctx& c, State& st, ex8 (&in)[NCB][8], ex8 (&out)[NCB][8]) {
    constexpr LayerDesc D = layer_desc(L);
    constexpr int KS_CHAIN = D.chain_k / 32;
    constexpr int KS_EXTRA = D.extra_slots / 32;
    constexpr int KS = KS_CHAIN + KS_EXTRA;
    constexpr int CC = chunk_first(L) + C;
    constexpr int NT = chunk_tiles(CC);
    constexpr int RT0 = chunk_rt0(L, C);
    constexpr int F = NT * KS;
    constexpr int AHEAD = 4;
    constexpr int BIAS_OFF = LDS_BIAS + (b16_bias_off(L) + 16 * RT0) * 4;
    constexpr int MT = NCB * KS;
    constexpr int PEND_M0 = NT * MT >= 4 * NCB + 4 ? 2 : 0;
    constexpr int PAIR0 = RT0 / 2;
    constexpr int NPAIR_IN = NT >= 4 ? NT / 2 - 1 : 0;
    constexpr int PAIR_M0 = 2 * MT + (MT >= 4 * NCB + 2 ? 2 : 0);
    static_assert(NT < 4 || NT % 2 == 0, "whole pairs per chunk");
    static_assert(D.extra_kind != 2, "no direction features in the sigma network");
    static_assert(PL < 0 || PL == L || NCB * PQ >= PEND_M0 + 4 * NCB, "pending pair finished too late");
    const unsigned wb = c.b_wread[CC & 1];
    const unsigned xb = c.b_posx;
    constexpr int NCC = (CC + 1) % NUM_CHUNKS;
    constexpr int NL = chunk_layer(NCC);
    constexpr int NF = chunk_tiles(NCC) * (layer_desc(NL).chain_k / 32 + layer_desc(NL).extra_slots / 32);
    constexpr int NBIAS_OFF = LDS_BIAS + (b16_bias_off(NL) + 16 * chunk_rt0(NL, NCC - chunk_first(NL))) * 4;
    const unsigned nwb = c.b_wread[NCC & 1];
    constexpr int TAIL = 3;
    constexpr int FB = F <= TAIL ? F : F - TAIL;
    WFrag& wf = *st.wf;
    auto barrier_and_prefetch = [&]() {
        // every fragment read of this chunk was issued two fragment slots ago: lgkmcnt(0) is free; vmcnt(0): this wave's
        // DMA pieces of the next chunk have landed (the only vector-memory instructions in flight are those pieces and,
        // in the first chunk of a tile, the previous tile's sigma stores and this tile's point loads)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        chunk_barrier<0>();
#pragma unroll
        for (int f = 0; f < AHEAD && f < NF; ++f) wf.a[f] = lds_load<ex8>(nwb, f * 1024);
        wf.bias0 = lds_load<f32x4>(c.b_bias, NBIAS_OFF);
        __builtin_amdgcn_sched_barrier(0);
    };

    // the next chunk's DMA pieces go out one per SPREAD MFMAs, the last one well before the barrier
    constexpr int SPREAD = 4;
    constexpr bool DMA_SPREAD = 1 + SPREAD * (Stage<CC>::PIECES - 1) + 8 <= FB * NCB;
    if constexpr (!DMA_SPREAD) Stage<CC>::issue(c);
    __builtin_amdgcn_sched_barrier(0);

    ex8 a[AHEAD];
#pragma unroll
    for (int f = 0; f < AHEAD && f < F; ++f) a[f] = wf.a[f];
    ex8 bx[NCB][KS_EXTRA > 0 ? KS_EXTRA : 1];
    if constexpr (KS_EXTRA > 0) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int e = 0; e < KS_EXTRA; ++e) bx[cb][e] = lds_load<ex8>(xb, cb * 2048 + e * 1024);
    }
    f32x4 acc[NCB][NT];
    acc[0][0] = wf.bias0;
    for (int cb = 1; cb < NCB; ++cb) acc[cb][0] = acc[0][0];
    __builtin_amdgcn_sched_barrier(0);

    // register lifetimes against the MFMA write-after-read hazards: see mlp_bf16_16.hip chunk_step
    ex8 as_prev = a[0];
    f32x4 c_prev = acc[0][0];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int f = t * KS + ks;
            if (f == FB) barrier_and_prefetch();
            const ex8 as = a[f % AHEAD];
            if (f + AHEAD < F) a[f % AHEAD] = lds_load<ex8>(wb, (f + AHEAD) * 1024);
            if (t + 1 < NT && ks == KS / 2) {
                acc[0][t + 1 < NT ? t + 1 : 0] = lds_load<f32x4>(c.b_bias, BIAS_OFF + 64 * (t + 1));
                for (int cb = 1; cb < NCB; ++cb) acc[cb][t + 1 < NT ? t + 1 : 0] = acc[0][t + 1 < NT ? t + 1 : 0];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const int m = f * NCB + cb;
                ex8 bs;
                if (ks < KS_CHAIN) bs = in[cb][ks < KS_CHAIN ? ks : 0];
                else bs = bx[cb][KS_EXTRA > 0 ? (ks - KS_CHAIN < KS_EXTRA ? ks - KS_CHAIN : 0) : 0];
                const f32x4 c_old = acc[cb][t];
                acc[cb][t] = NERF_MFMA(as, bs, c_old, 0, 0, 0);
                asm volatile("" ::"v"(c_prev));
                c_prev = c_old;
                if constexpr (DMA_SPREAD) {
                    if (m % SPREAD == 1 && m / SPREAD < Stage<CC>::PIECES) Stage<CC>::issue_piece(c, m / SPREAD);
                }
                if constexpr (PL >= 0) {
                    if (m >= PEND_M0 && m < PEND_M0 + 4 * NCB) {
                        if constexpr (PL == L) epilogue_piece<PL, PQ>(m - PEND_M0, st.pend, out, st);
                        else epilogue_piece<PL, PQ>(m - PEND_M0, st.pend, in, st);
                    }
                }
                if constexpr (NPAIR_IN > 0) {
                    const int j = (m - PAIR_M0) / (2 * MT), pm = (m - PAIR_M0) - j * (2 * MT);
                    if (m >= PAIR_M0 && j < NPAIR_IN && pm < 4 * NCB) {
                        f32x4 pr[NCB][2];
                        for (int q_ = 0; q_ < NCB; ++q_) { pr[q_][0] = acc[q_][2 * j]; pr[q_][1] = acc[q_][2 * j + 1]; }
                        in_chunk_epilogue<L, PAIR0, NPAIR_IN>(j, pm, pr, out, st);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            asm volatile("" ::"v"(as_prev));
            as_prev = as;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    asm volatile("" ::"v"(as_prev));
    asm volatile("" ::"v"(c_prev));
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        st.pend[cb][0] = acc[cb][NT >= 2 ? NT - 2 : 0];
        st.pend[cb][1] = acc[cb][NT - 1];
    }
    if constexpr (FB == F) barrier_and_prefetch();
}

__host__ __device__ constexpr int prev_layer(int L, int C) { return C > 0 ? L : L - 1; }
__host__ __device__ constexpr int prev_pair(int L, int C) {
    // pending pair when chunk (L, C) starts: the last pair of the previous chunk (L0 of a tile starts with none)
    return C > 0 ? (chunk_rt0(L, C) / 2 - 1) : (L > 0 ? b16_mt(L - 1) / 2 - 1 : 0);
}

template <int L, int... Cs>
__device__ __forceinline__ void run_layer_seq(const Ctx& c, State& st, ex8 (&in)[NCB][8], ex8 (&out)[NCB][8],
                                              std::integer_sequence<int, Cs...>) {
    (chunk_step<L, Cs, prev_layer(L, Cs), prev_pair(L, Cs)>(c, st, in, out), ...);
}
template <int L>
__device__ __forceinline__ void run_layer(const Ctx& c, State& st, ex8 (&in)[NCB][8], ex8 (&out)[NCB][8]) {
    run_layer_seq<L>(c, st, in, out, std::make_integer_sequence<int, layer_chunks(L)>{});
}

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
    epilogue_piece<SIGMA_LAYER, SIGMA_TILE / 2>(0, st.pend, st.X, st);     // the sigma tile is still pending
    for (int cb_ = 1; cb_ < NCB; ++cb_) epilogue_piece<SIGMA_LAYER, SIGMA_TILE / 2>(4 * cb_, st.pend, st.X, st);
}

template <bool GRID>
__global__ __launch_bounds__(WAVES * 64, WAVES / 4) void DENSITY_KERNEL(DensityArgs a, long long ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    (void)smem;
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
    {
        const float* bsrc = reinterpret_cast<const float*>(img + (long long)B16_WEIGHT_KIB * 1024);
        for (int i = threadIdx.x; i < B16_BIAS_FLOATS; i += WAVES * 64) lds_store<float>(i * 4, LDS_BIAS, bsrc[i]);
        Stage<NUM_CHUNKS - 1>::issue(c);         // chunk 0
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    WFrag wf;
    {
        constexpr int F0 = chunk_tiles(0) * (layer_desc(0).chain_k / 32 + layer_desc(0).extra_slots / 32);
#pragma unroll
        for (int f = 0; f < 4 && f < F0; ++f) wf.a[f] = lds_load<ex8>(c.b_wread[0], f * 1024);
        wf.bias0 = lds_load<f32x4>(c.b_bias, LDS_BIAS + b16_bias_off(0) * 4);
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
        // sticky range flag (nerf_layout.h B16_STATUS_OFF), the plain vector buffer store of mlp_bf16_16.hip flag_nonfinite
        if (bad) __builtin_amdgcn_raw_buffer_store_b32(1u, c.wrsrc, (int)(B16_STATUS_OFF + 4 * NERF_STATUS_WORD_NONFINITE), 0, 0);
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
