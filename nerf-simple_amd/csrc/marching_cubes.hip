// marching_cubes.hip -- surface extraction from an fp32 scalar volume (a density grid, density.hip).  Not in the reference.
//
// Volume sigma[Rx, Ry, Rz], C order (z fastest); grid point (i, j, k) has linear index v = (i Ry + j) Rz + k and
// coordinates x_a(i) = fl(lo_a + fl(i s_a)).  Semantics (include/nerf_amd.h; tests/mesh_model.py restates them in numpy):
//   * a corner is inside iff sigma > level; an edge crosses iff exactly one endpoint is inside and both are finite;
//   * one vertex per crossing edge, numbered by (v of its lower endpoint, axis x < y < z); on edge a -> b (a lower),
//     t = fl(fl(level - sa) / fl(sb - sa)) and the coordinate on the edge's axis is fl(xa + fl(t fl(xb - xa)));
//   * the normal is -grad sigma (central differences, one-sided on the grid's faces) interpolated with t and normalised;
//   * a cell with all corners finite emits its case's triangles (csrc/mc_tables.h); faces are numbered by (cell linear
//     index, table order); a cell with a non-finite corner emits nothing.
// Every item is grid point v: it owns the edges v -> v + e_a and, if it is a cell's origin, that cell.  Both orders
// above are then orders over v, so the vertex and face numbers are exclusive scans over v:
//   count: mc_count_kernel  -- per block of ITEMS grid points, the number of vertices and of faces;
//          mc_scan_kernel   -- one workgroup: exclusive scan of the block counts, totals -> counts[2];
//   emit:  mc_vertex_kernel -- per grid point its first vertex number and edge mask (workspace), vertices and normals;
//          mc_face_kernel   -- triangles, whose corners look their vertex numbers up in the workspace.
// Hand-written scans, fixed block partition, no atomics: the output is the same bytes on every run.
#include "nerf_device.h"
#include "launchers.h"
#include "mc_tables.h"

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_PER_THREAD = 8;
constexpr long long MC_ITEMS = (long long)MC_THREADS * MC_PER_THREAD;        // grid points per block
constexpr int MC_SCAN_THREADS = 1024;

struct Grid {
    long long nx, ny, nz, n;         // n = nx ny nz
    float lo[3], step[3];
    float level;
};

__device__ __forceinline__ float coord(const Grid& g, int a, long long i) { return add_rn(g.lo[a], mul_rn((float)i, g.step[a])); }
__device__ __forceinline__ bool inside_of(float s, float level) { return s > level; }
__device__ __forceinline__ bool finite_of(float s) { return __builtin_fabsf(s) < __builtin_inff(); }

// What grid point (i, j, k) contributes: a 3-bit mask of its crossing edges (bit a: edge v -> v + e_a) and, if it is the
// origin of a cell whose corners are all finite, that cell's case (else -1).
struct Item {
    unsigned mask;
    int cas;
};
__device__ __forceinline__ Item classify(const float* __restrict__ sigma, const Grid& g, long long v, long long i, long long j,
                                         long long k) {
    const long long sx = g.ny * g.nz, sy = g.nz;
    const bool ex = i + 1 < g.nx, ey = j + 1 < g.ny, ez = k + 1 < g.nz;
    float c[8];
    c[0] = sigma[v];
    c[1] = ex ? sigma[v + sx] : 0.f;
    c[2] = ey ? sigma[v + sy] : 0.f;
    c[4] = ez ? sigma[v + 1] : 0.f;
    Item it{0u, -1};
    const bool f0 = finite_of(c[0]), in0 = inside_of(c[0], g.level);
    if (ex && f0 && finite_of(c[1]) && inside_of(c[1], g.level) != in0) it.mask |= 1u;
    if (ey && f0 && finite_of(c[2]) && inside_of(c[2], g.level) != in0) it.mask |= 2u;
    if (ez && f0 && finite_of(c[4]) && inside_of(c[4], g.level) != in0) it.mask |= 4u;
    if (ex && ey && ez) {
        c[3] = sigma[v + sx + sy];
        c[5] = sigma[v + sx + 1];
        c[6] = sigma[v + sy + 1];
        c[7] = sigma[v + sx + sy + 1];
        bool fin = true;
        int cas = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            fin &= finite_of(c[q]);
            cas |= (inside_of(c[q], g.level) ? 1 : 0) << q;
        }
        if (fin) it.cas = cas;
    }
    return it;
}

// (i, j, k) of the first of this thread's MC_PER_THREAD consecutive grid points; step() walks to the next one
struct Walker {
    long long v, i, j, k;
    __device__ __forceinline__ void init(const Grid& g, long long v0) {
        v = v0;
        k = v0 % g.nz;
        const long long r = v0 / g.nz;
        j = r % g.ny;
        i = r / g.ny;
    }
    __device__ __forceinline__ void step(const Grid& g) {
        ++v;
        if (++k == g.nz) {
            k = 0;
            if (++j == g.ny) { j = 0; ++i; }
        }
    }
};

// exclusive scan of one value per thread over the workgroup (MC_THREADS), in thread order; also the block total
__device__ __forceinline__ long long block_exclusive_scan(long long x, long long& total, long long* lds_waves) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
    }
    if (lane == 63) lds_waves[wave] = incl;
    __syncthreads();
    long long before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < MC_THREADS / 64; ++w) {
        const long long t = lds_waves[w];
        if (w < wave) before += t;
        total += t;
    }
    __syncthreads();                        // lds_waves may be reused by the caller's next scan
    return before + incl - x;
}

__global__ __launch_bounds__(MC_THREADS) void mc_count_kernel(const float* __restrict__ sigma, Grid g, int* __restrict__ blk) {
    __shared__ long long lds_waves[MC_THREADS / 64];
    const long long base = (long long)blockIdx.x * MC_ITEMS + (long long)threadIdx.x * MC_PER_THREAD;
    int nv = 0, nt = 0;
    if (base < g.n) {
        Walker w;
        w.init(g, base);
        for (int r = 0; r < MC_PER_THREAD && w.v < g.n; ++r, w.step(g)) {
            const Item it = classify(sigma, g, w.v, w.i, w.j, w.k);
            nv += __builtin_popcount(it.mask);
            if (it.cas >= 0) nt += mc_tables::tri_count[it.cas];
        }
    }
    long long tv, tf;
    (void)block_exclusive_scan(nv, tv, lds_waves);
    (void)block_exclusive_scan(nt, tf, lds_waves);
    if (threadIdx.x == 0) {
        blk[2 * blockIdx.x] = (int)tv;
        blk[2 * blockIdx.x + 1] = (int)tf;
    }
}

// one workgroup: exclusive scan of the per-block counts -> 64-bit block offsets, and the totals
__global__ __launch_bounds__(MC_SCAN_THREADS) void mc_scan_kernel(const int* __restrict__ blk, long long nblk,
                                                                  long long* __restrict__ off, long long* __restrict__ counts) {
    __shared__ long long lds[2][MC_SCAN_THREADS];
    // thread t scans a contiguous run of blocks; runs are combined by a scan over the threads
    const long long per = (nblk + MC_SCAN_THREADS - 1) / MC_SCAN_THREADS;
    const long long b0 = (long long)threadIdx.x * per;
    const long long b1 = b0 + per < nblk ? b0 + per : nblk;
    long long sv = 0, sf = 0;
    for (long long b = b0; b < b1; ++b) { sv += blk[2 * b]; sf += blk[2 * b + 1]; }
    lds[0][threadIdx.x] = sv;
    lds[1][threadIdx.x] = sf;
    __syncthreads();
    // Hillis-Steele inclusive scan over the 1024 run sums (double-buffered through registers)
    for (int d = 1; d < MC_SCAN_THREADS; d <<= 1) {
        const long long av = threadIdx.x >= (unsigned)d ? lds[0][threadIdx.x - d] : 0;
        const long long af = threadIdx.x >= (unsigned)d ? lds[1][threadIdx.x - d] : 0;
        __syncthreads();
        lds[0][threadIdx.x] += av;
        lds[1][threadIdx.x] += af;
        __syncthreads();
    }
    long long pv = lds[0][threadIdx.x] - sv, pf = lds[1][threadIdx.x] - sf;
    for (long long b = b0; b < b1; ++b) {
        off[2 * b] = pv;
        off[2 * b + 1] = pf;
        pv += blk[2 * b];
        pf += blk[2 * b + 1];
    }
    if (threadIdx.x == MC_SCAN_THREADS - 1) {
        counts[0] = lds[0][threadIdx.x];
        counts[1] = lds[1][threadIdx.x];
    }
}

// d sigma / d axis a at grid point (i, j, k) (p = its linear index, idx = its coordinate on axis a, n = extent, st = stride)
__device__ __forceinline__ float grad_at(const float* __restrict__ sigma, const Grid& g, int a, long long p, long long idx,
                                         long long n, long long st) {
    const long long hi = idx + 1 < n ? idx + 1 : idx, lo = idx > 0 ? idx - 1 : idx;
    const float num = sub_rn(sigma[p + (hi - idx) * st], sigma[p - (idx - lo) * st]);
    const float den = sub_rn(coord(g, a, hi), coord(g, a, lo));
    return __fdiv_rn(num, den);
}

__global__ __launch_bounds__(MC_THREADS) void mc_vertex_kernel(const float* __restrict__ sigma, Grid g,
                                                               const long long* __restrict__ off, int* __restrict__ first,
                                                               unsigned char* __restrict__ emask, float* __restrict__ verts,
                                                               float* __restrict__ normals, long long max_verts) {
    __shared__ long long lds_waves[MC_THREADS / 64];
    const long long base = (long long)blockIdx.x * MC_ITEMS + (long long)threadIdx.x * MC_PER_THREAD;
    unsigned masks[MC_PER_THREAD];
    int nv = 0;
    Walker w0;
    if (base < g.n) {
        w0.init(g, base);
        Walker w = w0;
        for (int r = 0; r < MC_PER_THREAD; ++r, w.step(g)) {
            masks[r] = w.v < g.n ? classify(sigma, g, w.v, w.i, w.j, w.k).mask : 0u;
            nv += __builtin_popcount(masks[r]);
        }
    }
    long long tot;
    long long id = off[2 * blockIdx.x] + block_exclusive_scan(nv, tot, lds_waves);
    if (base >= g.n) return;
    const long long sx = g.ny * g.nz, sy = g.nz;
    const long long ext[3] = {g.nx, g.ny, g.nz}, str[3] = {sx, sy, 1};
    Walker w = w0;
    for (int r = 0; r < MC_PER_THREAD && w.v < g.n; ++r, w.step(g)) {
        first[w.v] = (int)id;
        emask[w.v] = (unsigned char)masks[r];
        const long long ijk[3] = {w.i, w.j, w.k};
        for (int a = 0; a < 3; ++a) {
            if (!(masks[r] >> a & 1u)) continue;
            if (id < max_verts) {
                const float sa = sigma[w.v], sb = sigma[w.v + str[a]];
                const float t = __fdiv_rn(sub_rn(g.level, sa), sub_rn(sb, sa));
                float p[3];
                for (int b = 0; b < 3; ++b) p[b] = coord(g, b, ijk[b]);
                const float xa = p[a], xb = coord(g, a, ijk[a] + 1);
                p[a] = add_rn(xa, mul_rn(t, sub_rn(xb, xa)));
                verts[3 * id] = p[0];
                verts[3 * id + 1] = p[1];
                verts[3 * id + 2] = p[2];
                if (normals) {
                    const float one_t = sub_rn(1.f, t);
                    float n[3];
                    for (int b = 0; b < 3; ++b) {
                        const long long ib = ijk[b] + (b == a ? 1 : 0);
                        const float ga = grad_at(sigma, g, b, w.v, ijk[b], ext[b], str[b]);
                        const float gb = grad_at(sigma, g, b, w.v + str[a], ib, ext[b], str[b]);
                        n[b] = -add_rn(mul_rn(one_t, ga), mul_rn(t, gb));
                    }
                    const float ln = sqrt_rn(add_rn(add_rn(mul_rn(n[0], n[0]), mul_rn(n[1], n[1])), mul_rn(n[2], n[2])));
                    const bool ok = ln > 0.f && ln < __builtin_inff();
                    for (int b = 0; b < 3; ++b) normals[3 * id + b] = ok ? __fdiv_rn(n[b], ln) : 0.f;
                }
            }
            ++id;
        }
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_face_kernel(const float* __restrict__ sigma, Grid g,
                                                             const long long* __restrict__ off, const int* __restrict__ first,
                                                             const unsigned char* __restrict__ emask, int* __restrict__ faces,
                                                             long long max_faces) {
    __shared__ long long lds_waves[MC_THREADS / 64];
    const long long base = (long long)blockIdx.x * MC_ITEMS + (long long)threadIdx.x * MC_PER_THREAD;
    int cases[MC_PER_THREAD];
    int nt = 0;
    Walker w0;
    if (base < g.n) {
        w0.init(g, base);
        Walker w = w0;
        for (int r = 0; r < MC_PER_THREAD; ++r, w.step(g)) {
            cases[r] = w.v < g.n ? classify(sigma, g, w.v, w.i, w.j, w.k).cas : -1;
            if (cases[r] >= 0) nt += mc_tables::tri_count[cases[r]];
        }
    }
    long long tot;
    long long f = off[2 * blockIdx.x + 1] + block_exclusive_scan(nt, tot, lds_waves);
    if (base >= g.n) return;
    const long long sx = g.ny * g.nz, sy = g.nz;
    Walker w = w0;
    for (int r = 0; r < MC_PER_THREAD && w.v < g.n; ++r, w.step(g)) {
        if (cases[r] < 0) continue;
        const int n = mc_tables::tri_count[cases[r]];
        for (int q = 0; q < n; ++q, ++f) {
            if (f >= max_faces) continue;
            int vid[3];
            for (int e3 = 0; e3 < 3; ++e3) {
                const int e = mc_tables::tri_edges[cases[r]][3 * q + e3];
                const int lc = mc_tables::edge_lower[e], a = e >> 2;
                const long long u = w.v + (lc & 1) * sx + ((lc >> 1) & 1) * sy + ((lc >> 2) & 1);
                vid[e3] = first[u] + __builtin_popcount((unsigned)emask[u] & ((1u << a) - 1u));
            }
            faces[3 * f] = vid[0];
            faces[3 * f + 1] = vid[1];
            faces[3 * f + 2] = vid[2];
        }
    }
}

// workspace: [block counts int32 x 2 | block offsets int64 x 2 | first vertex int32 per grid point | edge mask byte per point]
struct McWs {
    long long nblk, off_blk, off_off, off_first, off_mask, bytes;
};
McWs mc_ws(long long n) {
    constexpr auto up = nerf_layout::align256;
    McWs w;
    w.nblk = (n + MC_ITEMS - 1) / MC_ITEMS;
    w.off_blk = 0;
    w.off_off = up(w.nblk * 8);
    w.off_first = w.off_off + up(w.nblk * 16);
    w.off_mask = w.off_first + up(n * 4);
    w.bytes = w.off_mask + up(n);
    return w;
}

Grid make_grid(long long nx, long long ny, long long nz, float level, const float* lo, const float* step) {
    Grid g;
    g.nx = nx; g.ny = ny; g.nz = nz; g.n = nx * ny * nz;
    for (int a = 0; a < 3; ++a) { g.lo[a] = lo ? lo[a] : 0.f; g.step[a] = step ? step[a] : 1.f; }
    g.level = level;
    return g;
}

}  // namespace

extern "C" long long nerf_amd_mc_workspace_bytes(long long n) { return mc_ws(n).bytes; }

extern "C" int nerf_amd_launch_mc_count(const float* sigma, long long nx, long long ny, long long nz, float level, void* ws,
                                        long long* counts, hipStream_t stream) {
    (void)hipGetLastError();
    const Grid g = make_grid(nx, ny, nz, level, nullptr, nullptr);
    const McWs w = mc_ws(g.n);
    char* b = reinterpret_cast<char*>(ws);
    hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)w.nblk), dim3(MC_THREADS), 0, stream, sigma, g,
                       reinterpret_cast<int*>(b + w.off_blk));
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(MC_SCAN_THREADS), 0, stream, reinterpret_cast<const int*>(b + w.off_blk),
                       w.nblk, reinterpret_cast<long long*>(b + w.off_off), counts);
    return (int)hipGetLastError();
}

extern "C" int nerf_amd_launch_mc_emit(const float* sigma, long long nx, long long ny, long long nz, float level,
                                       const float* h_lo, const float* h_step, void* ws, float* verts, float* normals, int* faces,
                                       long long max_verts, long long max_faces, hipStream_t stream) {
    (void)hipGetLastError();
    const Grid g = make_grid(nx, ny, nz, level, h_lo, h_step);
    const McWs w = mc_ws(g.n);
    char* b = reinterpret_cast<char*>(ws);
    const long long* off = reinterpret_cast<const long long*>(b + w.off_off);
    int* first = reinterpret_cast<int*>(b + w.off_first);
    unsigned char* emask = reinterpret_cast<unsigned char*>(b + w.off_mask);
    hipLaunchKernelGGL(mc_vertex_kernel, dim3((unsigned)w.nblk), dim3(MC_THREADS), 0, stream, sigma, g, off, first, emask, verts,
                       normals, max_verts);
    hipLaunchKernelGGL(mc_face_kernel, dim3((unsigned)w.nblk), dim3(MC_THREADS), 0, stream, sigma, g, off,
                       (const int*)first, (const unsigned char*)emask, faces, max_faces);
    return (int)hipGetLastError();
}
