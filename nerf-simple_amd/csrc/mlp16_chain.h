// mlp16_chain.h -- the 16x16x32 MFMA chain of the 16-bit MLP kernels: the chunk sequence of a 256-point tile, its
// hand-scheduled inner routine (chunk_step) and what goes with it.  One definition for every kernel that runs the chain:
// mlp_bf16_16.hip (inference, fused render, training forward; bf16 and fp16) and density.hip (the sigma-only network).
// tools/isa_diff.py shows whether an edit here, or a move of code into here, changed any kernel's instructions.
//
// The including file defines, for its build, before the #include:
//   elem_t, NERF_MFMA     the operand type and the matching v_mfma_f32_16x16x32 builtin;
// and supplies two types of its own to the templates below:
//   a chunk plan P        which tiles are streamed, in which chunks:
//       static constexpr int LAYERS;                   layers of the sequence (0 .. LAYERS - 1 of nerf_layout::layer_desc)
//       static constexpr bool SAVE;                    the training-forward stores (SAVE != 0 below) may be instantiated
//       static constexpr int tpc(int L);               16-row tiles per chunk of layer L
//       static constexpr int mt(int L);                16-row tiles of layer L that are streamed (consecutive in the image)
//       static constexpr int layer_off_kib(int L);     where the first of them starts in the weight image
//       static constexpr int bias_off(int L);          and in the bias table (floats)
//     A layer 8 of ONE tile is the lone sigma tile (row 256, pair 8): the folded and the sigma-only plans.  The chunk
//     count must be even (the double buffer's parity is cyclic over tiles) and a chunk must fit LDS_WBUF;
//   a tile state St       `using Plan = P;` and the members chunk_step touches: pend, bad, wf, sigma, and only where the
//     plan reaches them rgb (layer 10), posd_off (direction features) and the SAVE fields (see mlp_bf16_16.hip State).
// What a kernel keeps to itself besides its inputs and outputs: the prologue (Ctx set-up, bias table and chunk 0 into
// LDS, chunk 0's first fragments) and the posx encoder block of its stage_inputs.  Both were tried as routines of this
// header, in several forms (one routine, halves, by value, by reference): each compiles to other machine code in every
// kernel, the fused render's MFMA stream included -- a routine is simplified on its own before it is inlined -- and
// the kernels' instructions are what every measurement in DESIGN.md stands on.  The two copies must stay equal: density's
// sigma is column 3 of the forward's output bit for bit (tests/test_gpu_mesh.py).
//
// Schedule (DESIGN.md sections 4-5 record every decision here with its A/B measurement):
//   * a wave owns 32 points = two 16-point column blocks; 64 lanes = 16 points x 4 lane groups;
//   * two stacked 16-row accumulator tiles (2q, 2q+1), bias-initialised, ReLU'd and converted pairwise, ARE the B
//     fragment of the next layer's k-step q (32 features): activations never leave the registers;
//   * weights stream L2 -> LDS by LDS-DMA in chunks, double buffered, one barrier per chunk; one weight fragment read
//     from LDS (16 rows x 32 k, 1 KiB) feeds two MFMAs (the two column blocks);
//   * the chunk barrier sits three fragments before the END of a chunk and the next chunk's first fragments are
//     requested right behind it, so no chunk starts with an LDS round trip; the next chunk's DMA pieces go out one per
//     four MFMAs;
//   * in the inference kernels a wave's issue priority falls in four steps over a chunk, so that the two waves of a SIMD
//     stay in step and neither runs the end of a chunk alone (chunk_prio below).
#pragma once
#include "nerf_device.h"
#include <utility>

typedef elem_t ex8 __attribute__((ext_vector_type(8)));
typedef elem_t ex2 __attribute__((ext_vector_type(2)));

namespace {

using namespace nerf_layout;

// NCB 16-point column blocks per wave: 8 waves (2 per SIMD) x 2 blocks.  (4 waves x 4 blocks with
// the accumulators in AGPRs halves the LDS weight reads but measured 4.5 % slower: DESIGN.md section 5.)
constexpr int NCB = 2;
constexpr int WAVES = 16 / NCB;
constexpr int TILE_PTS = WAVES * 16 * NCB;

// ---- chunk arithmetic of plan P ---------------------------------------------------------------
template <class P>
__host__ __device__ constexpr int layer_chunks(int L) { return (P::mt(L) + P::tpc(L) - 1) / P::tpc(L); }
template <class P>
__host__ __device__ constexpr int chunk_first(int L) {
    int c = 0;
    for (int i = 0; i < L; ++i) c += layer_chunks<P>(i);
    return c;
}
template <class P>
constexpr int NUM_CHUNKS = chunk_first<P>(P::LAYERS);
template <class P>
__host__ __device__ constexpr int chunk_layer(int cc) {
    int L = 0;
    while (cc >= layer_chunks<P>(L)) { cc -= layer_chunks<P>(L); ++L; }
    return L;
}
template <class P>
__host__ __device__ constexpr int chunk_tiles(int cc) {
    const int L = chunk_layer<P>(cc), C = cc - chunk_first<P>(L);
    const int left = P::mt(L) - C * P::tpc(L);
    return left < P::tpc(L) ? left : P::tpc(L);
}
template <class P>
__host__ __device__ constexpr int chunk_kib(int cc) { return chunk_tiles<P>(cc) * b16_ks(chunk_layer<P>(cc)); }
template <class P>
__host__ __device__ constexpr int chunk_off_kib(int cc) {
    const int L = chunk_layer<P>(cc), C = cc - chunk_first<P>(L);
    return P::layer_off_kib(L) + C * P::tpc(L) * b16_ks(L);
}
// MFMAs of a wave per tile
template <class P>
__host__ __device__ constexpr int tile_mfmas() {
    int m = 0;
    for (int cc = 0; cc < NUM_CHUNKS<P>; ++cc) m += chunk_kib<P>(cc) * NCB;
    return m;
}

// LDS: [bias table | weight buffer 0 | weight buffer 1 | the kernel's own (encoded inputs, sample ring) from LDS_CHAIN_END]
constexpr int LDS_WBUF = 40 * 1024;
constexpr int LDS_BIAS = 0;
constexpr int LDS_W0 = 10 * 1024;
constexpr int LDS_CHAIN_END = LDS_W0 + 2 * LDS_WBUF;
static_assert(B16_BIAS_FLOATS * 4 <= LDS_W0, "bias table");
// every chunk fits a weight buffer, and the double buffer's parity is cyclic over tiles
template <class P>
__host__ __device__ constexpr bool plan_fits() {
    for (int cc = 0; cc < NUM_CHUNKS<P>; ++cc)
        if (chunk_kib<P>(cc) * 1024 > LDS_WBUF) return false;
    return NUM_CHUNKS<P> % 2 == 0;
}

// ---- issue priority inside a chunk (inference; DESIGN.md section 5, "Keeping a SIMD's two waves in step") -----------
// The two waves of a SIMD share its matrix pipe, and issue between them goes by priority first, then age.  At equal
// priority the older wave takes every slot it can use, finishes its MFMAs of a chunk first and waits in the chunk
// barrier while its partner runs the rest alone -- and one in-order wave, with a weight read, a conversion and a ReLU
// between its MFMAs, does not fill the pipe.  So a wave's priority FALLS as it advances through the chunk: PRIO_LEVELS
// steps of equal length, top level at the first MFMA, level 0 from the last step on (the barrier, BARRIER_TAIL
// fragments before the end, lies in it: both waves leave it together and nothing needs favouring there).  The wave
// that is behind is in an earlier step and outranks its partner, whichever of the two is the older one: same code in
// every wave, no wave-id test, no branch.  A level changes only between weight fragments (both column-block MFMAs of a
// fragment issue at one level).  The cut-off, by the stamps of every chunk barrier (profiles/chunk_priority_stamp_chunks_*.txt):
// chunks under PRIO_MIN_MFMAS MFMAs hold level 0 -- the sigma tile (16), the rgb tile (8), the 32-MFMA halves of layer 0:
// a step of theirs would be a few MFMAs, shorter than the lag it is to bound -- and so does layer 0 as a whole (the
// sigma-only plan runs it as one 64-MFMA chunk): its lag is the prologue's, the leader waits longer there than the
// chunk's own MFMAs take.  Every chunk ends at level 0, so the prologue, the ring barrier and compositing run at
// level 0 in all waves.  Rules tried and their A/B: DESIGN.md section 5.
constexpr int BARRIER_TAIL = 3;       // the chunk barrier sits this many weight fragments before the end of a chunk
constexpr int PRIO_LEVELS = 4;
constexpr int PRIO_MIN_MFMAS = 64;
static_assert(PRIO_LEVELS >= 2 && PRIO_LEVELS <= 4, "s_setprio has levels 0..3");
__host__ __device__ constexpr bool chunk_stepped(int L, int mfmas) { return L >= 1 && mfmas >= PRIO_MIN_MFMAS; }
// level of chunk-linear MFMA m = fragment * NCB + column block, in a stepped chunk of `mfmas` MFMAs
__host__ __device__ constexpr int chunk_prio(int m, int mfmas, int levels) {
    const int step = mfmas / NCB / levels;            // weight fragments per level
    const int lv = levels - 1 - (m / NCB) / step;
    return lv > 0 ? lv : 0;
}
// what chunk_step relies on, for one chunk of F fragments whose barrier sits in front of fragment FB
__host__ __device__ constexpr bool chunk_prio_ok(int L, int F, int FB) {
    const int M = F * NCB;
    if (!chunk_stepped(L, M)) return true;            // held at level 0: constant by construction
    if (chunk_prio(0, M, PRIO_LEVELS) != PRIO_LEVELS - 1) return false;
    for (int m = 1; m < M; ++m) {
        if (chunk_prio(m, M, PRIO_LEVELS) > chunk_prio(m - 1, M, PRIO_LEVELS)) return false;       // never rises
        if (m >= FB * NCB && chunk_prio(m, M, PRIO_LEVELS) != 0) return false;                     // level 0 from the barrier on
        if (m % NCB != 0 && chunk_prio(m, M, PRIO_LEVELS) != chunk_prio(m - 1, M, PRIO_LEVELS)) return false;   // one level per fragment
    }
    return true;
}
template <class P>
__host__ __device__ constexpr bool plan_prio_ok() {
    for (int cc = 0; cc < NUM_CHUNKS<P>; ++cc) {
        const int F = chunk_kib<P>(cc);               // a weight fragment is 1 KiB
        if (!chunk_prio_ok(chunk_layer<P>(cc), F, F <= BARRIER_TAIL ? F : F - BARRIER_TAIL)) return false;
    }
    return true;
}
// s_setprio takes an immediate: the unrolled chunk loop folds this to the one instruction
__device__ __forceinline__ void set_prio(int level) {
    switch (level) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
    }
}

struct Ctx {
    __amdgpu_buffer_rsrc_t wrsrc;
    unsigned wave_goff, lane16;
    unsigned b_wread[2];            // weight buffer p + lane*16
    unsigned s_wdst[2];             // this wave's DMA piece in weight buffer p (wave-uniform)
    unsigned b_bias;                // (lane>>4)*16
    unsigned b_posx, b_posd;        // this lane's encoded inputs (the kernel's prologue; posd: kernels with direction features)
    int wave, lane;
};

// The first AHEAD weight fragments and the first bias vector of the chunk that runs next, requested
// right behind the barrier that publishes its buffer -- which the inference kernels place three
// fragments BEFORE the end of the previous chunk, so the LDS round trip of these reads is covered by
// that chunk's last six MFMAs instead of idling the matrix pipe at every chunk start.
struct WFrag {
    ex8 a[4];
    f32x4 bias0;
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

// LDS-DMA of the chunk behind chunk CC (cyclic: the last chunk of a tile fetches the first one of the next tile)
template <class P, int CC>
using Stage = ChunkDma<Ctx, (CC + 1) % NUM_CHUNKS<P>, chunk_kib<P>((CC + 1) % NUM_CHUNKS<P>), chunk_off_kib<P>((CC + 1) % NUM_CHUNKS<P>), WAVES>;

// One of the 8 pieces of the epilogue of row-tile pair Q of layer L (tiles
// 2Q, 2Q+1; both column blocks): piece i -> column block i>>2, word i&3 of the
// next layer's fragment Q.  Heads: (L8, Q=8) is the lone sigma tile, L10 the
// rgb tile.
template <int L, int Q, int SAVE = 0, class St>
__device__ __forceinline__ void epilogue_piece(int i, const f32x4 (&acc)[NCB][2], ex8 (&dst)[NCB][8], St& st) {
    static_assert(!SAVE || St::Plan::SAVE, "this plan has no training forward");
    constexpr LayerDesc D = layer_desc(L);
    const int cb = i >> 2, j2 = i & 3;   // i in [0, 4*NCB)
    if constexpr (Q == 0 && L >= 1 && L <= 9) {
        // Range guard.  If ANY input feature of this layer is inf (an fp16 activation beyond 65504) every one of its
        // rows sums w * inf: +-inf, or NaN with two of them -- so one accumulator element per point tells.  (The
        // outputs alone do not: the integer ReLU below turns a NaN with the sign bit set into 0, and a layer whose
        // rows are all NaN comes out as all zeros, finite from there on.)  One compare per column block and layer.
        // (A layer 8 that is the sigma tile alone has no pair 0; an inf in h8 shows in the colour layer, which reads
        // h8 itself, and in sigma, which the tile's finiteness check sees.)
        if (j2 == 0) st.bad |= __builtin_amdgcn_classf(acc[cb][0][0], 0x207);      // sNaN | qNaN | -inf | +inf
    }
    if constexpr (L == 10) {
        if (j2 == 0) { st.rgb[cb][0] = acc[cb][0][0]; st.rgb[cb][1] = acc[cb][0][1]; st.rgb[cb][2] = acc[cb][0][2]; }
    } else if constexpr (L == 8 && Q == 8) {
        if (j2 == 0) st.sigma[cb] = acc[cb][0][0];
    } else {
        u32x4 w = __builtin_bit_cast(u32x4, dst[cb][Q]);
        w[j2] = pack2<D.relu != 0>(acc[cb][j2 >> 1][2 * (j2 & 1)], acc[cb][j2 >> 1][2 * (j2 & 1) + 1]);
        dst[cb][Q] = __builtin_bit_cast(ex8, w);
        if constexpr (SAVE == 2) {
            // 8-bit storage form: magnitudes are collected word by word over a group of four fragments (128 features); when
            // the group's last fragment is complete in both column blocks the wave converts and writes all four under one
            // exponent (nerf_device.h store_group_f8).  The accumulator is picked by (layer, group) parity: the pending pair
            // of the previous layer and this layer's first pair can be in flight together.
            constexpr int GS = (L & 1) * 2 + ((Q >> 2) & 1);
            st.amax[GS] = f8_absmax<D.relu == 0>(((Q & 3) == 0 && i == 0) ? 0.f : st.amax[GS], acc[cb][j2 >> 1][2 * (j2 & 1)],
                                                 acc[cb][j2 >> 1][2 * (j2 & 1) + 1]);
            if constexpr ((Q & 3) == 3) {
                if (i == 4 * NCB - 1) {
                    static_assert(NCB == 2, "store_group_f8 takes the two column blocks of a wave");
                    constexpr int Q0 = Q - 3;
                    char* tb = st.acts + (f8_offset_bytes(L, st.P) + st.tile * F8_BLOCK_BYTES);
                    char* sp = st.acts + (f8_scale_offset_bytes(L, st.P) + st.tile * 64);
                    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(tb, 0, (int)F8_BLOCK_BYTES, 0x00020000);
                    const __amdgpu_buffer_rsrc_t rss = __builtin_amdgcn_make_buffer_rsrc(sp, 0, 64, 0x00020000);
                    const u32x4 g0[4] = {__builtin_bit_cast(u32x4, dst[0][Q0]), __builtin_bit_cast(u32x4, dst[0][Q0 + 1]),
                                         __builtin_bit_cast(u32x4, dst[0][Q0 + 2]), __builtin_bit_cast(u32x4, dst[0][Q0 + 3])};
                    const u32x4 g1[4] = {__builtin_bit_cast(u32x4, dst[1][Q0]), __builtin_bit_cast(u32x4, dst[1][Q0 + 1]),
                                         __builtin_bit_cast(u32x4, dst[1][Q0 + 2]), w};
                    store_group_f8<2>(rs, st.loff[0], Q0 * 8192, rss, (int)(threadIdx.x & 63), (int)(threadIdx.x >> 6) * 8 + Q0,
                                      g0, g1, st.amax[GS]);
                }
            }
        }
        if constexpr (SAVE) {
            // the fragment is complete: write this lane's 2 x 4 features of layer L's output
            // (features 32Q+4g.. and 32Q+16+4g.. of its point) for the backward pass
            if (SAVE == 1 && j2 == 3) {
                // Buffer stores into this (layer, tile)'s point-blocked block (nerf_layout.h),
                // unconditional so the vector-memory instruction count per chunk is a constant
                // (chunk_barrier); lanes past the last point carry an offset outside num_records.
                // The lane holds two 8-byte pieces (features 32Q+4g.. and 32Q+16+4g..):
                // v_permlane16_swap trades one with the neighbouring 16-lane row (g ^ 1) -- even g
                // ends up with [its first piece | g+1's first piece], odd g with [g-1's second piece |
                // its second piece], i.e. one whole 16-byte granule (chunk 4Q + swapped_chunk(g)).
                // The 16 lanes of a quarter-wave then write 256 contiguous bytes.
                char* tb = st.acts + (act_offset_bytes(L, st.P) + st.tile * ACT_BLOCK_BYTES);
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(tb, 0, (int)ACT_BLOCK_BYTES, 0x00020000);
                store_granule<2>(rs, st.loff[cb], Q * 16384, w);
            }
            if constexpr (D.relu != 0) {
                // ReLU mask for the backward pass: one bit per feature (post-ReLU bf16 != 0), collected
                // per group of 4 pairs and written as one coalesced dword per thread
                static_assert(NCB == 2, "mask layout: two column blocks per wave");
                // t = {low != 0, high != 0} as 0/1 halves: one packed unsigned min with {1, 1} (hipcc
                // lowers the generic form to two compares, two selects and a permute)
                const unsigned wj = w[j2];
                unsigned t;
                asm("v_pk_min_u16 %0, %1, %2" : "=v"(t) : "v"(wj), "s"(0x00010001u));
                const int pos = (Q & 3) * 4 + j2;
                st.mb[cb][Q >> 2] = pos == 0 ? t : ((t << pos) | st.mb[cb][Q >> 2]);
                if (pos == 15) {
                    // wave-uniform 64-bit base + this thread's 32-bit offset (scalar base, one offset VGPR)
                    char* mp = st.acts + (st.mask_tile + ((long long)L * mask_tiles(st.P) * 4 + (cb * 2 + (Q >> 2))) * 2048);
                    *reinterpret_cast<unsigned*>(mp + (unsigned)(threadIdx.x * 4)) = st.mb[cb][Q >> 2];
                }
            }
        }
    }
}

// vector-memory instructions epilogue_piece<L, Q, SAVE> issues over its 4*NCB pieces
template <int SAVE>
__host__ __device__ constexpr int pair_vmem_ops(int L, int Q) {
    if (!SAVE || L < 0 || L == 10 || (L == 8 && Q == 8)) return 0;
    const int masks = (layer_desc(L).relu != 0 && (Q & 3) == 3) ? NCB : 0;  // a mask dword per block behind every fourth pair
    // bf16 form: one activation store per block; 8-bit form: a group of four fragments at once (4 stores + 1 exponent dword)
    return (SAVE == 2 ? ((Q & 3) == 3 ? F8_GROUP + 1 : 0) : NCB) + masks;
}
template <int SAVE>
__host__ __device__ constexpr int pair_mask_ops(int L, int Q) {
    if (!SAVE || L < 0 || L == 10 || (L == 8 && Q == 8)) return 0;
    return (layer_desc(L).relu != 0 && (Q & 3) == 3) ? NCB : 0;
}
template <int SAVE>
__host__ __device__ constexpr int vmem_before_barrier(int L, int PL, int PQ, int pair0, int npair_in, int pend_m0, int pend_per,
                                                      int pair_m0, int mt, int m_limit) {
    int n = 0;
    // Column block cb's last piece (4 cb + 3) carries its mask dword and, in the bf16 form, its activation store; in the
    // 8-bit form the wave's column blocks are converted and written together -- a whole group of four fragments -- by
    // the last piece of the group's last pair.
    const int last = 4 * NCB - 1;
    if (PL >= 0) {
        const int masks = pair_mask_ops<SAVE>(PL, PQ), data = pair_vmem_ops<SAVE>(PL, PQ) - masks;
        for (int cb = 0; cb < NCB; ++cb) {
            const int own = 4 * cb + 3;
            if (pend_m0 + own / pend_per < m_limit) n += masks / NCB + (SAVE == 2 ? 0 : data / NCB);
        }
        if (SAVE == 2 && pend_m0 + last / pend_per < m_limit) n += data;
    }
    for (int j = 0; j < npair_in; ++j) {
        const int masks = pair_mask_ops<SAVE>(L, pair0 + j), data = pair_vmem_ops<SAVE>(L, pair0 + j) - masks;
        for (int cb = 0; cb < NCB; ++cb) {
            const int own = 4 * cb + 3;
            if (pair_m0 + j * 2 * mt + own < m_limit) n += masks / NCB + (SAVE == 2 ? 0 : data / NCB);
        }
        if (SAVE == 2 && pair_m0 + j * 2 * mt + last < m_limit) n += data;
    }
    return n;
}
// epilogue piece `i` of in-chunk pair j (a compile-time pair index is needed: dispatch over the few values)
template <int L, int P0, int N, int SAVE, int J = 0, class St>
__device__ __forceinline__ void in_chunk_epilogue(int j, int i, const f32x4 (&acc)[NCB][2], ex8 (&dst)[NCB][8], St& st) {
    if constexpr (J < N) {
        if (j == J) epilogue_piece<L, P0 + J, SAVE>(i, acc, dst, st);
        else in_chunk_epilogue<L, P0, N, SAVE, J + 1>(j, i, acc, dst, st);
    }
}

// ---- one chunk: NT 16-row tiles of layer L starting at tile C * tpc(L) of the streamed ones --------
// PL/PQ: layer / pair of the pending accumulators handed over by the previous chunk.
template <int L, int C, int PL, int PQ, int SAVE, class St>
__device__ __forceinline__ void chunk_step(const Ctx& c, St& st, ex8 (&in)[NCB][8], ex8 (&out)[NCB][8]) {
    using P = typename St::Plan;
    constexpr LayerDesc D = layer_desc(L);
    constexpr int KS_CHAIN = D.chain_k / 32;
    constexpr int KS_EXTRA = D.extra_slots / 32;
    constexpr int KS = KS_CHAIN + KS_EXTRA;
    constexpr int CC = chunk_first<P>(L) + C;
    constexpr int NT = chunk_tiles<P>(CC);
    constexpr int RT0 = C * P::tpc(L);
    constexpr int F = NT * KS;                      // weight fragments (each feeds 2 MFMAs)
    constexpr int AHEAD = 4;                         // weight fragments in flight ahead of their MFMAs (2..8 measure alike)
    constexpr int BIAS_OFF = LDS_BIAS + (P::bias_off(L) + 16 * RT0) * 4;
    // chunk-linear MFMA index m = (t*KS + ks)*2 + cb
    constexpr int MT = NCB * KS;                      // MFMAs per row tile
    constexpr int PEND_M0 = (L == 10) ? 0 : (NT * MT >= 4 * NCB + 4 ? 2 : 0);
    constexpr int PEND_PER = (L == 10) ? 2 : 1;     // pieces per MFMA for the pending pair
    // Row-tile pairs of this chunk: pair j (tiles 2j, 2j+1; layer pair PAIR0 + j) gets its epilogue in the shadow
    // of the MFMAs of pair j + 1, starting at MFMA PAIR_M0 + j * 2 MT; the last pair is handed to the next chunk
    constexpr int PAIR0 = RT0 / 2;
    constexpr int NPAIR_IN = NT >= 4 ? NT / 2 - 1 : 0;
    constexpr int PAIR_M0 = 2 * MT + (MT >= 4 * NCB + 2 ? 2 : 0);
    static_assert(NT < 4 || NT % 2 == 0, "whole pairs per chunk");
    // a pending pair of the PREVIOUS layer is this layer's k-step PQ, first read by MFMA 2*PQ
    static_assert(PL < 0 || PL == L || (PL == 8 && PQ == 8) || NCB * PQ >= PEND_M0 + 4 * NCB / PEND_PER,
                  "pending pair finished too late");
    const unsigned wb = c.b_wread[CC & 1];
    // the chunk that runs next (cyclic: the last chunk of a tile prefetches the first one of the next tile)
    constexpr int NCC = (CC + 1) % NUM_CHUNKS<P>;
    constexpr int NL = chunk_layer<P>(NCC);
    constexpr int NF = chunk_tiles<P>(NCC) * (layer_desc(NL).chain_k / 32 + layer_desc(NL).extra_slots / 32);
    constexpr int NBIAS_OFF = LDS_BIAS + (P::bias_off(NL) + 16 * (NCC - chunk_first<P>(NL)) * P::tpc(NL)) * 4;
    const unsigned nwb = c.b_wread[NCC & 1];
    // Where the chunk's barrier sits, as a fragment index: TAIL fragments before the end of the chunk.
    constexpr int TAIL = BARRIER_TAIL;
    constexpr int FB = F <= TAIL ? F : F - TAIL;
    // Falling issue priority over the chunk (chunk_prio above).  Not in the training forward, which is issue-bound in
    // another regime (counted vmcnt waits, stores in every epilogue piece) and keeps its machine code.
    constexpr bool STEPPED = !SAVE && chunk_stepped(L, F * NCB);
    static_assert(plan_prio_ok<P>(), "priority: top level at MFMA 0, never rising, one level per fragment, 0 from the barrier on");
    // The training forward's counted wait: vector-memory instructions this wave issues between its DMA pieces
    // (first in the chunk) and the barrier, i.e. the activation / mask stores of the epilogue pieces that sit in
    // front of MFMA FB * NCB (piece 4 cb + 3 of a pair carries column block cb's stores); the ones behind the
    // barrier are older than the next chunk's DMA and need no count.  (Inference: 0 -- the only vector-memory
    // instructions in flight are the DMA pieces and, in the first chunk of a tile, the previous tile's output stores
    // and this tile's input loads.)
    constexpr int VMEM_N = vmem_before_barrier<SAVE>(L, PL, PQ, PAIR0, NPAIR_IN, PEND_M0, PEND_PER, PAIR_M0, MT, FB * NCB);
    WFrag& wf = *st.wf;
    auto barrier_and_prefetch = [&]() {
        // Every fragment read of this chunk has been issued at least two fragment slots ago (AHEAD = 4,
        // TAIL = 3): lgkmcnt(0) is free, and it makes the buffer reusable -- no wave reads it after its
        // barrier.  vmcnt: this wave's LDS-DMA pieces of the next chunk (issued first in this chunk) have
        // landed; the training forward's stores behind them may fly on.
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        chunk_barrier<VMEM_N>();
#pragma unroll
        for (int f = 0; f < AHEAD && f < NF; ++f) wf.a[f] = lds_load<ex8>(nwb, f * 1024);
        wf.bias0 = lds_load<f32x4>(c.b_bias, NBIAS_OFF);
        __builtin_amdgcn_sched_barrier(0);
    };

    // DMA of the next chunk: the training forward issues all pieces first (its counted vmcnt assumes every
    // store of the chunk behind them); the inference kernels, whose first fragments are already in
    // registers, start their MFMAs at once and issue one piece every SPREAD MFMAs -- provided the last
    // piece still goes out well before the MFMA in front of which the barrier publishes that buffer
    // (a piece issued behind the barrier would be read by the prefetch before it has landed)
    constexpr int SPREAD = 4;
    constexpr bool DMA_SPREAD = !SAVE && 1 + SPREAD * (Stage<P, CC>::PIECES - 1) + 8 <= FB * NCB;
    if constexpr (!DMA_SPREAD) Stage<P, CC>::issue(c);
    __builtin_amdgcn_sched_barrier(0);   // every other vector-memory instruction of the chunk stays behind the DMA

    ex8 a[AHEAD];
#pragma unroll
    for (int f = 0; f < AHEAD && f < F; ++f) a[f] = wf.a[f];       // requested behind the previous barrier
    // the encoded inputs of the layer: posx (2 KiB per column block at b_posx) or the lane's direction fragment
    ex8 bx[NCB][KS_EXTRA > 0 ? KS_EXTRA : 1];
    if constexpr (KS_EXTRA > 0) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int e = 0; e < KS_EXTRA; ++e) {
                if constexpr (D.extra_kind == 1) bx[cb][e] = lds_load<ex8>(c.b_posx, cb * 2048 + e * 1024);
                else bx[cb][e] = lds_load<ex8>(st.posd_off[cb], e * 1024);
            }
    }
    f32x4 acc[NCB][NT];
    // register i of lane group g is row 16*rt + 4g + i: one 16-B bias read per tile
    acc[0][0] = wf.bias0;
    for (int cb = 1; cb < NCB; ++cb) acc[cb][0] = acc[0][0];
    __builtin_amdgcn_sched_barrier(0);

    // Register lifetimes against the MFMA write-after-read hazards.  The allocator hands the registers an
    // MFMA has just read for the last time (its weight fragment, and the old accumulator: D != C in the
    // VGPR form) to the very next definition -- the following ds_read or cvt_pk -- and the hazard
    // recognizer then puts 2-4 wait states between the two: 617 s_nop per tile, ~1700 cycles per wave,
    // in a stream whose issue time is what bounds the kernel.  Empty asm uses keep a fragment alive for one
    // more fragment slot and an accumulator for one more MFMA, so the registers that come free were last
    // read two instructions ago: 8 more live VGPRs, 190 s_nop per tile, -1.7 ... 2.1 % time.
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
            if constexpr (STEPPED) {
                // every chunk is entered at level 0 (the previous one ended there): emitted only where the level changes
                const int lv = chunk_prio(f * NCB, F * NCB, PRIO_LEVELS);
                if (lv != (f == 0 ? 0 : chunk_prio((f - 1) * NCB, F * NCB, PRIO_LEVELS))) set_prio(lv);
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
                asm volatile("" :: "v"(c_prev));
                c_prev = c_old;
                if constexpr (DMA_SPREAD) {
                    if (m % SPREAD == 1 && m / SPREAD < Stage<P, CC>::PIECES) Stage<P, CC>::issue_piece(c, m / SPREAD);
                }
                // ---- epilogue pieces in this MFMA's shadow
                if constexpr (PL >= 0) {
                    if (m >= PEND_M0 && m < PEND_M0 + 4 * NCB / PEND_PER) {
#pragma unroll
                        for (int k = 0; k < PEND_PER; ++k) {
                            const int i = (m - PEND_M0) * PEND_PER + k;
                            if constexpr (PL == L) epilogue_piece<PL, PQ, SAVE>(i, st.pend, out, st);
                            else epilogue_piece<PL, PQ, SAVE>(i, st.pend, in, st);
                        }
                    }
                }
                if constexpr (NPAIR_IN > 0) {
                    const int j = (m - PAIR_M0) / (2 * MT), pm = (m - PAIR_M0) - j * (2 * MT);
                    if (m >= PAIR_M0 && j < NPAIR_IN && pm < 4 * NCB) {
                        f32x4 pr[NCB][2];
                        for (int q_ = 0; q_ < NCB; ++q_) { pr[q_][0] = acc[q_][2 * j]; pr[q_][1] = acc[q_][2 * j + 1]; }
                        in_chunk_epilogue<L, PAIR0, NPAIR_IN, SAVE>(j, pm, pr, out, st);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            asm volatile("" :: "v"(as_prev));
            as_prev = as;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    asm volatile("" :: "v"(as_prev));
    asm volatile("" :: "v"(c_prev));
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        st.pend[cb][0] = acc[cb][NT >= 2 ? NT - 2 : 0];
        st.pend[cb][1] = acc[cb][NT - 1];
    }
    if constexpr (FB == F) barrier_and_prefetch();
}

__host__ __device__ constexpr int prev_layer(int L, int C) { return C > 0 ? L : L - 1; }
template <class P>
__host__ __device__ constexpr int prev_pair(int L, int C) {
    // pending pair when chunk (L, C) starts: same layer -> the last pair of chunk C-1; else the previous
    // layer's last pair (L8 ends with its lone sigma tile, marked as pair 8)
    return C > 0 ? C * P::tpc(L) / 2 - 1 : (L > 0 ? (L - 1 == 8 ? 8 : P::mt(L - 1) / 2 - 1) : 0);
}

template <int L, int SAVE, class St, int... Cs>
__device__ __forceinline__ void run_layer_seq(const Ctx& c, St& st, ex8 (&in)[NCB][8], ex8 (&out)[NCB][8],
                                              std::integer_sequence<int, Cs...>) {
    using P = typename St::Plan;
    (chunk_step<L, Cs, prev_layer(L, Cs), prev_pair<P>(L, Cs), SAVE>(c, st, in, out), ...);
}
// layer L of the tile: its chunks in order (the plan is the state's: St::Plan)
template <int L, int SAVE = 0, class St>
__device__ __forceinline__ void run_layer(const Ctx& c, St& st, ex8 (&in)[NCB][8], ex8 (&out)[NCB][8]) {
    run_layer_seq<L, SAVE>(c, st, in, out, std::make_integer_sequence<int, layer_chunks<typename St::Plan>(L)>{});
}

// Sticky range flag (nerf_layout.h B16_STATUS_OFF): a point with a non-finite accumulator in layers 1..9 (epilogue_piece)
// or a non-finite output sets status word 0 behind the packed image.  The host wrapper reads it
// (utils/nets.py): the reference is fp32 and has no range limit (utils/nets.py:16-32), so an overflowing fp16 render
// must not pass silently.  A plain store of the constant 1 through the weight image's own buffer descriptor (every
// writer writes the same value: no atomic, no extra pointer kept live across the tile loop).
__device__ __forceinline__ void flag_nonfinite(const Ctx& c, bool bad) {
    if (bad) __builtin_amdgcn_raw_buffer_store_b32(1u, c.wrsrc, (int)(B16_STATUS_OFF + 4 * NERF_STATUS_WORD_NONFINITE), 0, 0);
}

}  // namespace
