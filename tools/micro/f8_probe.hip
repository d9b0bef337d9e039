// What exactly do the gfx950 8-bit instructions do that the fp8 storage form of the training step is built on?  The guides
// name them but not their lane maps.  Three probes, each printed against a host model:
//   1. ds_read_b64_tr_b8: which LDS byte lands in (lane, byte k) for two address patterns;
//   2. v_cvt_scalef32_pk_fp8_bf16 / v_cvt_scalef32_pk_f32_fp8: is the scale a divisor on the way down and a factor on the
//      way up, which half does op_sel pick, how does it round and saturate;
//   3. v_mfma_scale_f32_32x32x64_f8f6f4 with e4m3 operands: where do a lane's 32 bytes sit in K and whose scale byte
//      multiplies them?  (Measured, profiles/r04_f8_probe.txt: the same byte position of the A lane of row m and of the B
//      lane of column n pair up; K block 0 = bytes 0..15 of lanes r and r + 32, scaled by the byte op_sel picks from the
//      scale register of lane r; K block 1 = bytes 16..31 of both lanes, scale from lane r + 32 -- NOT "a lane's 32 bytes
//      are one block", which is the model the first check prints as failing.)
//   4. how exact is the sum inside one instruction (products 2^-14 below the largest of their group of eight are dropped;
//      on random signed data the mean error is 5e-9 of the sum of |products|: nothing beside 8-bit operands), and how
//      the instruction's sum is added into the accumulator C = 2^k (profiles/f8_probe_accumulator.txt);
//   5. what the exponent byte 0xFF (e8m0's NaN) does to a K block whose data bytes are zero, and to one whose are not.
//   hipcc --offload-arch=gfx950 -O2 -o f8_probe f8_probe.hip && ./f8_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v2i __attribute__((ext_vector_type(2)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef short v2s __attribute__((ext_vector_type(2)));
typedef __bf16 v2bf __attribute__((ext_vector_type(2)));
typedef float v2f __attribute__((ext_vector_type(2)));

__global__ void tr_kernel(const unsigned char* fill, int nfill, const int* addr, v2i* out) {
    extern __shared__ char sm[];
    for (int i = threadIdx.x; i < nfill; i += 64) sm[i] = fill[i];
    __syncthreads();
    out[threadIdx.x] = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) v2i*)(sm + addr[threadIdx.x]));
}

__global__ void cvt_kernel(const v2bf* x, const float* sc, int n, unsigned* down_lo, unsigned* down_hi, v2f* up_lo, v2f* up_hi) {
    const int i = threadIdx.x;
    if (i >= n) return;
    const v2s old = {(short)0x1111, (short)0x2222};
    down_lo[i] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(old, x[i], sc[i], false));
    down_hi[i] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(old, x[i], sc[i], true));
    up_lo[i] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(down_lo[i], sc[i], false);
    up_hi[i] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(down_hi[i], sc[i], true);
}

template <int OA, int OB>
__global__ void mfma_kernel(const v8i* a, const v8i* b, const int* sa, const int* sb, v16f* d) {
    const int l = threadIdx.x;
    v16f c;
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    d[l] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[l], b[l], c, 0, 0, OA, sa[l], OB, sb[l]);
}

template <int OA, int OB>
__global__ void mfma_c_kernel(const v8i* a, const v8i* b, const int* sa, const int* sb, float c0, v16f* d) {
    const int l = threadIdx.x;
    v16f c;
    for (int r = 0; r < 16; ++r) c[r] = c0;
    d[l] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[l], b[l], c, 0, 0, OA, sa[l], OB, sb[l]);
}

static float e4m3(unsigned char v) {
    const int s = v >> 7, e = (v >> 3) & 15, m = v & 7;
    if (e == 15 && m == 7) return NAN;
    const float x = e == 0 ? ldexpf((float)m / 8.f, -6) : ldexpf(1.f + (float)m / 8.f, e - 7);
    return s ? -x : x;
}
static unsigned short bf16_bits(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    return (unsigned short)((u + 0x7fff + ((u >> 16) & 1)) >> 16);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

int main() {
    // ---- 1. transposing read
    {
        const int NF = 4096;
        unsigned char h_fill[2][NF];
        for (int i = 0; i < NF; ++i) { h_fill[0][i] = i & 0xff; h_fill[1][i] = i >> 8; }
        int h_addr[2][64];
        for (int l = 0; l < 64; ++l) {
            h_addr[0][l] = l * 8;
            h_addr[1][l] = (l >> 4) * 1024 + ((l & 15) >> 1) * 64 + (l & 1) * 8;      // rows of 64 B, two lanes per row
        }
        unsigned char* d_fill; int* d_addr; v2i* d_out;
        CK(hipMalloc(&d_fill, NF)); CK(hipMalloc(&d_addr, 256)); CK(hipMalloc(&d_out, 512));
        for (int pat = 0; pat < 2; ++pat) {
            unsigned char got[2][512];
            for (int f = 0; f < 2; ++f) {
                CK(hipMemcpy(d_fill, h_fill[f], NF, hipMemcpyHostToDevice));
                CK(hipMemcpy(d_addr, h_addr[pat], 256, hipMemcpyHostToDevice));
                hipLaunchKernelGGL(tr_kernel, dim3(1), dim3(64), NF, 0, d_fill, NF, d_addr, d_out);
                CK(hipMemcpy(got[f], d_out, 512, hipMemcpyDeviceToHost));
            }
            printf("tr_b8 pattern %d (lane: its address | LDS byte address delivered to byte 0..7)\n", pat);
            int model_ok = 1;
            for (int l = 0; l < 64; ++l) {
                if (l < 18 || l == 32 || l == 47 || l == 63) printf("  lane %2d: %4d |", l, h_addr[pat][l]);
                for (int k = 0; k < 8; ++k) {
                    const int src = got[0][l * 8 + k] | (got[1][l * 8 + k] << 8);
                    if (l < 18 || l == 32 || l == 47 || l == 63) printf(" %4d", src);
                    // model: within the 16-lane group, byte k of lane j comes from the address of lane 2k + (j >> 3), byte j & 7
                    const int grp = l & ~15, j = l & 15;
                    const int want = h_addr[pat][grp + 2 * k + (j >> 3)] + (j & 7);
                    if (src != want) model_ok = 0;
                }
                if (l < 18 || l == 32 || l == 47 || l == 63) printf("\n");
            }
            printf("  model 'byte k of lane j <- address of lane 2k + (j>>3) of the group, byte j&7': %s\n", model_ok ? "HOLDS" : "does NOT hold");
        }
    }
    // ---- 2. conversions
    {
        const float xs[][2] = {{1.f, 3.f}, {0.3f, -100.f}, {500.f, 1e-3f}, {448.f, 464.f}, {0.0175f, -0.0019f}, {1.0625f, 1.1875f},
                               {17.f, 19.f}, {240.f, 256.f}};
        const float scs[] = {1.f, 2.f, 0.25f, 16.f, 3.f};
        const int NX = sizeof(xs) / sizeof(xs[0]), NS = sizeof(scs) / sizeof(scs[0]), n = NX * NS;
        unsigned short hx[64][2]; float hs[64];
        for (int i = 0; i < n; ++i) { hx[i][0] = bf16_bits(xs[i % NX][0]); hx[i][1] = bf16_bits(xs[i % NX][1]); hs[i] = scs[i / NX]; }
        v2bf* dx; float* ds; unsigned *dl, *dh; v2f *ul, *uh;
        CK(hipMalloc(&dx, 256)); CK(hipMalloc(&ds, 256)); CK(hipMalloc(&dl, 256)); CK(hipMalloc(&dh, 256)); CK(hipMalloc(&ul, 512)); CK(hipMalloc(&uh, 512));
        CK(hipMemcpy(dx, hx, n * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(ds, hs, n * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(cvt_kernel, dim3(1), dim3(64), 0, 0, dx, ds, n, dl, dh, ul, uh);
        unsigned hl[64], hh[64]; float hul[64][2], huh[64][2];
        CK(hipMemcpy(hl, dl, n * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(hh, dh, n * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(hul, ul, n * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(huh, uh, n * 8, hipMemcpyDeviceToHost));
        printf("cvt_scalef32_pk_fp8_bf16 (old = 0x22221111): x0 x1 scale | word(lo sel) word(hi sel) | decoded e4m3 of the new bytes | back up (lo) (hi)\n");
        for (int i = 0; i < n; ++i) {
            const unsigned b0 = hh[i] >> 16 & 0xff, b1 = hh[i] >> 24;
            printf("  %9.4g %9.4g %5.2f | %08x %08x | %9.4g %9.4g | %9.4g %9.4g  %9.4g %9.4g\n", xs[i % NX][0], xs[i % NX][1], hs[i], hl[i], hh[i],
                   e4m3(b0), e4m3(b1), hul[i][0], hul[i][1], huh[i][0], huh[i][1]);
        }
    }
    // ---- 3. scaled MFMA
    {
        unsigned char ha[64][32], hb[64][32];
        int hsa[64], hsb[64];
        srand(7);
        for (int l = 0; l < 64; ++l) {
            for (int j = 0; j < 32; ++j) {
                do ha[l][j] = rand() & 0xff; while ((ha[l][j] & 0x7f) == 0x7f);
                do hb[l][j] = rand() & 0xff; while ((hb[l][j] & 0x7f) == 0x7f);
            }
            // scale bytes in byte 1 (A) and byte 2 (B) of the scale dword; the other bytes hold decoys
            hsa[l] = (0x55 << 24) | (0x99 << 16) | ((120 + rand() % 12) << 8) | 0x33;
            hsb[l] = (0x44 << 24) | ((122 + rand() % 12) << 16) | (0x88 << 8) | 0x22;
        }
        v8i *da, *db; int *dsa, *dsb; v16f* dd;
        CK(hipMalloc(&da, 2048)); CK(hipMalloc(&db, 2048)); CK(hipMalloc(&dsa, 256)); CK(hipMalloc(&dsb, 256)); CK(hipMalloc(&dd, 4096));
        CK(hipMemcpy(da, ha, 2048, hipMemcpyHostToDevice)); CK(hipMemcpy(db, hb, 2048, hipMemcpyHostToDevice));
        CK(hipMemcpy(dsa, hsa, 256, hipMemcpyHostToDevice)); CK(hipMemcpy(dsb, hsb, 256, hipMemcpyHostToDevice));
        hipLaunchKernelGGL((mfma_kernel<1, 2>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dd);
        float hd[64][16];
        CK(hipMemcpy(hd, dd, 4096, hipMemcpyDeviceToHost));
        // C/D layout of the 32x32 forms: lane l, register r -> row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
        double worst = 0, worst_noscale = 0, big = 0;
        for (int l = 0; l < 64; ++l)
            for (int r = 0; r < 16; ++r) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), n = l & 31;
                double want = 0, plain = 0;
                for (int b = 0; b < 2; ++b) {
                    const int la = m + 32 * b, lb = n + 32 * b;
                    double s = 0;
                    for (int j = 0; j < 32; ++j) s += (double)e4m3(ha[la][j]) * (double)e4m3(hb[lb][j]);
                    plain += s;
                    want += s * ldexp(1.0, ((hsa[la] >> 8) & 0xff) - 127) * ldexp(1.0, ((hsb[lb] >> 16) & 0xff) - 127);
                }
                worst = fmax(worst, fabs(hd[l][r] - want));
                worst_noscale = fmax(worst_noscale, fabs(hd[l][r] - plain));
                big = fmax(big, fabs(want));
            }
        // diagnostics: (a) all scale bytes 127: pairing alone; (b) one lane's scale byte doubled: which partial sum moves
        {
            int one[64];
            for (int l = 0; l < 64; ++l) one[l] = 0x7f7f7f7f;
            CK(hipMemcpy(dsa, one, 256, hipMemcpyHostToDevice)); CK(hipMemcpy(dsb, one, 256, hipMemcpyHostToDevice));
            hipLaunchKernelGGL((mfma_kernel<1, 2>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dd);
            float h0[64][16];
            CK(hipMemcpy(h0, dd, 4096, hipMemcpyDeviceToHost));
            double w = 0, bg = 0;
            for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 16; ++r) {
                    const int m = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), n = l & 31;
                    double plain = 0;
                    for (int b = 0; b < 2; ++b)
                        for (int j = 0; j < 32; ++j) plain += (double)e4m3(ha[m + 32 * b][j]) * (double)e4m3(hb[n + 32 * b][j]);
                    w = fmax(w, fabs(h0[l][r] - plain)); bg = fmax(bg, fabs(plain));
                }
            printf("  (a) all scales 2^0: max |D - plain sum| = %.4g of %.4g\n", w, bg);
            const int Ls[] = {0, 5, 37, 63};
            for (int which = 0; which < 2; ++which)          // 0: A's scale, 1: B's scale
                for (int li = 0; li < 4; ++li)
                    for (int byte = 0; byte < 4; ++byte) {
                        const int L = Ls[li];
                        int sc[64];
                        for (int l = 0; l < 64; ++l) sc[l] = 0x7f7f7f7f;
                        sc[L] = (sc[L] & ~(0xff << (8 * byte))) | (0x80 << (8 * byte));
                        CK(hipMemcpy(which ? dsb : dsa, sc, 256, hipMemcpyHostToDevice));
                        CK(hipMemcpy(which ? dsa : dsb, one, 256, hipMemcpyHostToDevice));
                        hipLaunchKernelGGL((mfma_kernel<1, 2>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dd);
                        float h1[64][16];
                        CK(hipMemcpy(h1, dd, 4096, hipMemcpyDeviceToHost));
                        // which outputs moved, and for the first moved one: which quarters (lane half b, 8-byte group q) explain it
                        int moved = 0, fm = -1, fn = -1; double fdiff = 0;
                        int rows[32] = {0}, cols[32] = {0};
                        for (int l = 0; l < 64; ++l)
                            for (int r = 0; r < 16; ++r) {
                                const int m = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), n = l & 31;
                                const double df = (double)h1[l][r] - (double)h0[l][r];
                                if (fabs(df) > 1e-3) { ++moved; rows[m] = 1; cols[n] = 1; if (fm < 0) { fm = m; fn = n; fdiff = df; } }
                            }
                        int nr = 0, nc = 0, r0 = -1, c0 = -1;
                        for (int i = 0; i < 32; ++i) { if (rows[i]) { ++nr; if (r0 < 0) r0 = i; } if (cols[i]) { ++nc; if (c0 < 0) c0 = i; } }
                        printf("  (b) %c scale of lane %2d, byte %d doubled: %4d outputs moved (%d rows from %d, %d cols from %d)", which ? 'B' : 'A', L, byte, moved, nr, r0, nc, c0);
                        if (fm >= 0) {
                            double part[8];
                            for (int b = 0; b < 2; ++b)
                                for (int q = 0; q < 4; ++q) {
                                    double s2 = 0;
                                    for (int j = 8 * q; j < 8 * q + 8; ++j) s2 += (double)e4m3(ha[fm + 32 * b][j]) * (double)e4m3(hb[fn + 32 * b][j]);
                                    part[b * 4 + q] = s2;
                                }
                            int best = -1; double be = 1e300;
                            for (int mask = 1; mask < 256; ++mask) {
                                double s2 = 0;
                                for (int k = 0; k < 8; ++k) if (mask >> k & 1) s2 += part[k];
                                if (fabs(s2 - fdiff) < be) { be = fabs(s2 - fdiff); best = mask; }
                            }
                            printf("; D[%d][%d] moved by the quarters mask 0x%02x (bit = 4 b + q; residual %.3g)", fm, fn, best, be);
                        }
                        printf("\n");
                    }
        }
        printf("mfma_scale 32x32x64 e4m3: max |D - model| = %.4g (largest |D| %.4g); against the unscaled sum %.4g\n", worst, big, worst_noscale);
        printf("  model 'a lane's 32 bytes = one block, its own scale byte (op_sel), same byte position pairs': %s\n",
               worst <= 1e-5 * big ? "HOLDS" : "does NOT hold");
    }
    // ---- 4. how exact is the sum inside one scaled MFMA?  Row m of A = one large element 2^8 and 63 small ones 2^-t
    // (scale bytes lift the pair apart further); B = ones; C = 0 or a large accumulator.
    {
        v8i *da, *db; int *dsa, *dsb; v16f* dd;
        CK(hipMalloc(&da, 2048)); CK(hipMalloc(&db, 2048)); CK(hipMalloc(&dsa, 256)); CK(hipMalloc(&dsb, 256)); CK(hipMalloc(&dd, 4096));
        unsigned char ha[64][32], hb[64][32];
        int one[64];
        for (int l = 0; l < 64; ++l) one[l] = 0x7f7f7f7f;
        memset(hb, 0x38, sizeof(hb));                      // 1.0
        printf("sum inside one MFMA: row = {2^8, 63 x 2^-t}: D - 2^8 (exact: 63 x 2^-t)\n");
        for (int t = -6; t <= 9; ++t) {
            // small = 2^-t as e4m3: normal for t <= 6 (exp field 7 - t), subnormal 2^-7..2^-9 (mantissa 4, 2, 1)
            const unsigned char small = t <= 6 ? (unsigned char)((7 - t) << 3) : (unsigned char)(1 << (9 - t));
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 32; ++j) ha[l][j] = small;
            for (int m = 0; m < 32; ++m) ha[m][0] = (15 << 3);                  // 2^8
            CK(hipMemcpy(da, ha, 2048, hipMemcpyHostToDevice)); CK(hipMemcpy(db, hb, 2048, hipMemcpyHostToDevice));
            CK(hipMemcpy(dsa, one, 256, hipMemcpyHostToDevice)); CK(hipMemcpy(dsb, one, 256, hipMemcpyHostToDevice));
            hipLaunchKernelGGL((mfma_kernel<1, 2>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dd);
            float hd[64][16];
            CK(hipMemcpy(hd, dd, 4096, hipMemcpyDeviceToHost));
            printf("  t = %2d: D - 256 = %.9g   exact %.9g   (relative to 2^8: small = 2^%d)\n", t, (double)hd[0][0] - 256.0, 63.0 * ldexp(1.0, -t), -t - 8);
        }
        // signed random data: mean error against the exact sum
        srand(11);
        double se = 0, sa2 = 0, sabs = 0; int cnt = 0;
        for (int rep = 0; rep < 8; ++rep) {
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 32; ++j) {
                    // magnitudes log-uniform over 2^-3 .. 2^8, A positive (activations), B signed (gradients)
                    ha[l][j] = (unsigned char)(((4 + rand() % 12) << 3) | (rand() & 7));
                    hb[l][j] = (unsigned char)(((rand() & 1) << 7) | ((4 + rand() % 12) << 3) | (rand() & 7));
                    if ((ha[l][j] & 0x7f) == 0x7f) ha[l][j] = 0x7e;
                    if ((hb[l][j] & 0x7f) == 0x7f) hb[l][j] = (hb[l][j] & 0x80) | 0x7e;
                }
            CK(hipMemcpy(da, ha, 2048, hipMemcpyHostToDevice)); CK(hipMemcpy(db, hb, 2048, hipMemcpyHostToDevice));
            hipLaunchKernelGGL((mfma_kernel<1, 2>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, dd);
            float hd[64][16];
            CK(hipMemcpy(hd, dd, 4096, hipMemcpyDeviceToHost));
            for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 16; ++r) {
                    const int m = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), n = l & 31;
                    double ex = 0, ab = 0;
                    for (int b = 0; b < 2; ++b)
                        for (int j = 0; j < 32; ++j) {
                            const double pr = (double)e4m3(ha[m + 32 * b][j]) * (double)e4m3(hb[n + 32 * b][j]);
                            ex += pr; ab += fabs(pr);
                        }
                    se += hd[l][r] - ex; sa2 += (hd[l][r] - ex) * (hd[l][r] - ex); sabs += ab; ++cnt;
                }
        }
        printf("random blocks (A > 0, B signed, magnitudes 2^-3..2^8): mean error %.4g, rms error %.4g, mean sum of |products| %.4g\n",
               se / cnt, sqrt(sa2 / cnt), sabs / cnt);
        // the accumulator: C = 2^k, row = one product of 1.0 (63 zeros beside it), then 64 products of 1.0.  A true fp32
        // add gives D - C = 1 up to k = 23 and 0 (a tie, to even) at k = 24; 64 is exact at every k here.
        printf("sum into the accumulator: C = 2^k; D - C for a row of one product of 1.0 | of 64 products of 1.0\n");
        memset(hb, 0x38, sizeof(hb));
        CK(hipMemcpy(db, hb, 2048, hipMemcpyHostToDevice));
        CK(hipMemcpy(dsa, one, 256, hipMemcpyHostToDevice)); CK(hipMemcpy(dsb, one, 256, hipMemcpyHostToDevice));
        for (int k = 8; k <= 24; ++k) {
            const float c0 = ldexpf(1.f, k);
            double diff[2][2];
            for (int many = 0; many < 2; ++many) {
                memset(ha, many ? 0x38 : 0x00, sizeof(ha));
                for (int m = 0; m < 32; ++m) ha[m][0] = 0x38;
                CK(hipMemcpy(da, ha, 2048, hipMemcpyHostToDevice));
                hipLaunchKernelGGL((mfma_c_kernel<1, 2>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, c0, dd);
                float hd[64][16];
                CK(hipMemcpy(hd, dd, 4096, hipMemcpyDeviceToHost));
                diff[many][0] = (double)hd[0][0] - (double)c0;                  // D[0][0]
                diff[many][1] = (double)hd[63][15] - (double)c0;                // D[31][31]
            }
            printf("  k = %2d: D - C = %.9g (D[31][31]: %.9g) | %.9g (D[31][31]: %.9g)\n", k, diff[0][0], diff[0][1], diff[1][0], diff[1][1]);
        }
    }
    // ---- 5. the exponent byte 0xFF (the NaN of e8m0) on a K block: lanes 32..63 of A (K block 1) carry it, block 0 is a
    // row of 32 products of 1.0.  Does the block turn the output into NaN when its data bytes are all zero?  When they are not?
    {
        v8i *da, *db; int *dsa, *dsb; v16f* dd;
        CK(hipMalloc(&da, 2048)); CK(hipMalloc(&db, 2048)); CK(hipMalloc(&dsa, 256)); CK(hipMalloc(&dsb, 256)); CK(hipMalloc(&dd, 4096));
        unsigned char ha[64][32], hb[64][32];
        int one[64], sa[64];
        for (int l = 0; l < 64; ++l) { one[l] = 0x7f7f7f7f; sa[l] = l < 32 ? 0x7f7f7f7f : 0x7f7fff7f; }
        memset(hb, 0x38, sizeof(hb));
        CK(hipMemcpy(db, hb, 2048, hipMemcpyHostToDevice)); CK(hipMemcpy(dsb, one, 256, hipMemcpyHostToDevice));
        printf("exponent byte 0xFF on K block 1 of A (block 0: 32 products of 1.0, exponent 127):\n");
        for (int kind = 0; kind < 3; ++kind) {
            // 0: block 1 zero data under 0xFF; 1: block 1 ones under 0xFF; 2: block 1 zero data under byte 0 (2^-127)
            memset(ha, 0x38, sizeof(ha));
            for (int l = 0; l < 64; ++l)
                for (int j = 16; j < 32; ++j) ha[l][j] = kind == 1 ? 0x38 : 0x00;
            if (kind == 2) for (int l = 32; l < 64; ++l) sa[l] = 0x7f7f007f;
            CK(hipMemcpy(da, ha, 2048, hipMemcpyHostToDevice)); CK(hipMemcpy(dsa, sa, 256, hipMemcpyHostToDevice));
            hipLaunchKernelGGL((mfma_c_kernel<1, 2>), dim3(1), dim3(64), 0, 0, da, db, dsa, dsb, 0.f, dd);
            float hd[64][16];
            CK(hipMemcpy(hd, dd, 4096, hipMemcpyDeviceToHost));
            int nans = 0;
            for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 16; ++r) nans += std::isnan(hd[l][r]) ? 1 : 0;
            printf("  block 1 %s: D[0][0] = %.9g, %d of 1024 outputs NaN\n",
                   kind == 0 ? "zero data, exponent 0xFF" : kind == 1 ? "ones, exponent 0xFF     " : "zero data, exponent 0x00", (double)hd[0][0], nans);
        }
    }
    return 0;
}
