// dw_products.h -- what the two storage forms of the parameter-gradient launch (dw_gemm.hip: bf16, dw_gemm_f8.hip: e4m3)
// have in common: the table of the 14 products, the bucket rule, the split of the workgroups over the products, the layout of
// the e4m3 scratch and (for hipcc) the kernels' lookup of their product.  The host part is plain C++ like nerf_layout.h
// and is checked on the CPU against the tests' models (tests/test_dw_products_cpu.py).  A change to which operand goes with
// which, or to who gets how many workgroups, is made here and nowhere else.
#pragma once
#include "nerf_layout.h"

namespace nerf_layout {

// an operand by name: dY[layer] / X[layer] (point-blocked, act_width(layer) features), the encoder rows, the packed d_raw
enum class DwKind { DY, ACT, POSX, POSD, DSR };
struct DwOperand { DwKind kind; int layer; };
// C[r, c] = sum_p a[p, r0 + r] * b[p, c] for 0 <= r < Mv, 0 <= c < Nv at grads[coff + r * ldc + c];
// boff >= 0: the column sums of a (= db of the layer whose dY it is) at grads[boff]
struct DwProduct { DwOperand a, b; int coff, ldc, r0, Mv, Nv, boff; };
constexpr int DW_NUM_PRODUCTS = 14;
constexpr DwOperand dw_dy(int L) { return {DwKind::DY, L}; }
constexpr DwOperand dw_act(int L) { return {DwKind::ACT, L}; }
constexpr DwOperand DW_POSX{DwKind::POSX, 0}, DW_POSD{DwKind::POSD, 0}, DW_DSR{DwKind::DSR, 0};
// a 256 x 256 layer L at w_off, its bias behind the weight
constexpr DwProduct dw_dense(int L, int w_off) { return {dw_dy(L), dw_act(L - 1), w_off, 256, 0, 256, 256, w_off + 65536}; }
constexpr int DW_LW = 256 * 256 + 256;
constexpr DwProduct DW_PRODUCTS[DW_NUM_PRODUCTS] = {
    {dw_dy(0), DW_POSX, OFF_L0_W, 63, 0, 256, 63, OFF_L0_B},                  // layers_0.0
    dw_dense(1, OFF_L1_W), dw_dense(2, OFF_L1_W + DW_LW),                     // layers_0.{2,4,6,8}
    dw_dense(3, OFF_L1_W + 2 * DW_LW), dw_dense(4, OFF_L1_W + 3 * DW_LW),
    {dw_dy(5), dw_act(4), OFF_SKIP_W, 319, 0, 256, 256, OFF_SKIP_B},          // skip [h ; x]: h part
    {dw_dy(5), DW_POSX, OFF_SKIP_W + 256, 319, 0, 256, 63, -1},               //               x part
    dw_dense(6, OFF_L6_W), dw_dense(7, OFF_L6_W + DW_LW),                     // layers_1.{0,2}
    {DW_DSR, dw_act(7), OFF_SIG_W, 256, 3, 1, 256, -1},                       // sigma_fc.0 (row 3 of dsr)
    {dw_dy(8), dw_act(7), OFF_L2_W, 256, 0, 256, 256, OFF_L2_B},              // layers_2
    {dw_dy(9), dw_act(8), OFF_C0_W, 283, 0, 128, 256, OFF_C0_B},              // color_fc.0 [h ; d]: h part
    {dw_dy(9), DW_POSD, OFF_C0_W + 256, 283, 0, 128, 27, -1},                 //                      d part
    {DW_DSR, dw_act(9), OFF_C1_W, 128, 0, 3, 128, -1},                        // color_fc.2 (rows 0..2)
};

// what differs between the storage forms and bears on the plan
struct DwForm { int slab, bytes_per_feature, dsr_width; };     // points per slab; operand bytes per feature; packed d_raw
constexpr DwForm DW_BF16{32, 2, 32}, DW_E4M3{64, 1, 16};
// features of an operand as a kernel reads it
constexpr int dw_operand_width(DwOperand o, DwForm f) {
    return o.kind == DwKind::POSX ? 64 : o.kind == DwKind::POSD ? 32 : o.kind == DwKind::DSR ? f.dsr_width : act_width(o.layer);
}

// products of a launch (indices into DW_PRODUCTS), product i on workgroups [wg0[i], wg0[i] + wgs[i]) of `workgroups`
struct DwPlan { int n; int product[16]; int wg0[16]; int wgs[16]; int workgroups; };
// bucket 0: all 14 products.  Buckets 1 and 2 split them at GRAD_BUCKET_SPLIT, the boundary of the flat gradient vector that
// data-parallel training reduces in two pieces: bucket 2 = the products whose destination lies below it (layers_0.*).
static inline DwPlan dw_plan(DwForm f, long long P, int bucket, int cus) {      // (static: the library exports its C ABI only)
    DwPlan plan{};
    int width[16];
    for (int i = 0; i < DW_NUM_PRODUCTS; ++i) {
        const bool head = DW_PRODUCTS[i].coff < GRAD_BUCKET_SPLIT;
        if (bucket != 0 && head != (bucket == 2)) continue;
        width[plan.n] = dw_operand_width(DW_PRODUCTS[i].a, f) + dw_operand_width(DW_PRODUCTS[i].b, f);
        plan.product[plan.n++] = i;
    }
    const int n = plan.n;
    // workgroups per product, one per CU in total.  A slab costs a workgroup the bytes it streams,
    // (M + N) * bytes_per_feature per point, plus a fixed part (barrier, DMA issue, fragment reads) that measures
    // larger than the byte part: profiles/r01e_dw_sweep.jsonl -- weights (M + N) + c with c = 0 /
    // 256 / 1024 / 8192 give 0.79 / 0.63 / 0.62 / 0.61 ms at 262144 points.  (Sizing by flops
    // left the thin products -- 32 x 256 reads as much of X as 256 x 256 -- as a 2 ms tail.)
    constexpr double slab_cost = 1024.0;
    double total = 0;
    for (int i = 0; i < n; ++i) total += (double)width[i] + slab_cost;
    const long long nslab = (P + f.slab - 1) / f.slab;
    // exactly `cus` workgroups in total when the slices allow it (the LDS ring leaves one
    // workgroup per CU, so a 257th would run as a second wave and double the kernel's time):
    // floor of each share, then the largest remainders get the leftover workgroups
    const long long need = (P * 256 * f.bytes_per_feature >> 30) + 1;      // a slice's operand stays below 1 GiB (32-bit buffer range)
    long long w[16];
    double rem[16];
    long long used = 0;
    for (int i = 0; i < n; ++i) {
        const double share = ((double)width[i] + slab_cost) / total * cus;
        w[i] = (long long)share;
        rem[i] = share - (double)w[i];
        if (w[i] < need) { w[i] = need; rem[i] = 0; }
        if (w[i] >= nslab) { w[i] = nslab; rem[i] = -1; }
        used += w[i];
    }
    while (used < cus) {
        int best = -1;
        for (int i = 0; i < n; ++i)
            if (rem[i] >= 0 && w[i] < nslab && (best < 0 || rem[i] > rem[best])) best = i;
        if (best < 0) break;
        ++w[best]; rem[best] = 0; ++used;      // a second round goes by product order
    }
    for (int i = 0; i < n; ++i) {
        plan.wg0[i] = plan.workgroups;
        plan.wgs[i] = (int)w[i];
        plan.workgroups += (int)w[i];
    }
    return plan;
}

// scratch_f8: the narrow operands in the 8-bit form (nerf_layout.h f8_narrow_*), each on a 256-byte boundary: posx | posd | dsr
struct F8Scratch { long long px, pd, ds, total; };
constexpr F8Scratch f8_scratch(long long P) {
    const long long pd = align256(f8_narrow_bytes(dw_operand_width(DW_POSX, DW_E4M3), P));
    const long long ds = pd + align256(f8_narrow_bytes(dw_operand_width(DW_POSD, DW_E4M3), P));
    return {0, pd, ds, ds + align256(f8_narrow_bytes(dw_operand_width(DW_DSR, DW_E4M3), P))};
}

#if defined(__HIPCC__)
// The device side of DwPlan::wg0: the product (entry of the kernel's own table) that workgroup blockIdx.x works on.  The only
// piece of the two kernels' framing that lives here; the others cannot move without moving instructions (DESIGN.md section
// 30), and this one only with its result in a variable of the kernel's (returned by value, the loop compiles differently).
template <class Table>
__device__ __forceinline__ void dw_product_of_workgroup(const Table& tab, int& di) {
    di = 0;
    while (di + 1 < tab.n && (int)blockIdx.x >= tab.d[di + 1].wg0) ++di;
}
#endif

}  // namespace nerf_layout
