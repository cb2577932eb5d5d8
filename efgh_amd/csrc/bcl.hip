// BCL splat (K3) and the adjoints of the BCL's two index operations, as GATHERS - no floating-point atomics on the path.
// Replaces SparseSum / the ones-splat of nets/bilateralNN.py:6-40,179-211 and the autograd of the neighbour gather :240-242.
//   splat[h][c] = ( sum_{(p,r): off[p][r]==h} bary[p][r]*x[p][c] ) / ( sum bary[p][r] + 1e-5 )
// with x[p] = [el_minus_gr[p] (4 channels, written by the lattice build) | feat[p] (Cf channels)]: the level's input row of
// enet.py:113,119,... is never concatenated, the two parts are read where they lie (feature rows stay 128-B multiples).
//
// The inverse of `off` (vertex -> sorted list of its flat positions f = 4p + r) is a by-product of the lattice build
// (lattice.hip: list, vseg), so the splat is one kernel: a wave per vertex, the whole list (<= 64 entries per trip) and its
// weights fetched by one load each, then lanes = (entry, 16-byte chunk) pairs so that every row of the list is in flight at
// once; partial sums are folded across the entry slots with shuffles and the normalised row is written once.
#include "common.h"
#include <algorithm>

namespace {
constexpr int TPB = 256;

// blocks of consecutive vertices / points are dealt to the XCDs as contiguous bands (blocks b and b+8 share an XCD under
// round-robin dispatch): vertices are numbered sample-major, so an XCD's L2 sees the rows of one or two samples only.
// Speed only - any placement gives the same result.
__device__ __forceinline__ int64_t xcd_band_block(int64_t b, int64_t nblocks) {
    const int64_t per = (nblocks + 7) / 8;
    const int64_t x = b & 7, j = b >> 3;
    const int64_t r = x * per + j;
    return (j < per && r < nblocks) ? r : -1;
}

__device__ __forceinline__ void fma4(float4 &a, float b, const float4 &v) {
    a.x += b * v.x; a.y += b * v.y; a.z += b * v.z; a.w += b * v.w;
}

// LPV lanes per vertex (64: one vertex per wave; 32: two - short lists leave a whole wave mostly idle and the kernel is bound
// by the number of vertices in flight x the three dependent round trips vseg -> list/bary -> rows).  Four trips of row loads
// are issued before the first FMA.
template <int LPV>
__global__ void __launch_bounds__(TPB)
k_splat_gather(const float4 *__restrict__ emg, const float4 *__restrict__ feat, int64_t ldf4, int cf4,
               const float *__restrict__ bary, const int *__restrict__ list, const int2 *__restrict__ vseg, int H,
               float4 *__restrict__ splat, int64_t lds4, float *__restrict__ wsum, int normalize) {
    constexpr int VPB = TPB / LPV;                             // vertices per block
    const int64_t nblocks = ((int64_t)H + VPB - 1) / VPB;
    const int64_t blk = xcd_band_block(blockIdx.x, nblocks);
    if (blk < 0) return;
    const int lane = threadIdx.x & 63, lv = lane & (LPV - 1), gb = lane - lv;
    const int64_t hh = blk * VPB + threadIdx.x / LPV;
    const bool have = hh < H;
    const int h = have ? (int)hh : 0;
    const int he = emg ? 1 : 0;
    const int CH = he + cf4;                                   // 16-byte chunks per entry row
    const int EPT = CH >= LPV ? 1 : LPV / CH;                  // entries in flight per trip
    const int e = lv / CH, c = lv - e * CH;                    // this lane: entry slot e, chunk c (and c + 64 when CH > 64)
    const bool active = e < EPT;
    const int cc = active ? c : 0;
    int2 seg = have ? vseg[h] : make_int2(0, 0);
    int lmax = seg.y;
    if (LPV <= 32) lmax = max(lmax, __shfl_xor(lmax, 32));     // every group of the wave runs the same shuffle rounds
    if (LPV <= 16) lmax = max(lmax, __shfl_xor(lmax, 16));
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
    float w = 0.f;
    for (int base = 0; base < lmax; base += LPV) {
        const int m = min(LPV, max(seg.y - base, 0));
        const int mm = min(LPV, lmax - base);
        const int f_l = lv < m ? list[seg.x + base + lv] : 0;
        const float b_l = lv < m ? bary[f_l] : 0.f;
        for (int t = 0; t < mm; t += 4 * EPT) {
            float4 v[4];
            float bq[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bq[u] = 0.f;
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (t + u * EPT >= mm) continue;                          // (wave-uniform: no trip without an entry)
                const int j = t + u * EPT + e;
                const int f = __shfl(f_l, gb + (j & (LPV - 1)));          // (all lanes take part in both shuffles)
                const float b = __shfl(b_l, gb + (j & (LPV - 1)));
                const bool ok = active && j < m;
                // no branch around the load: lanes without an entry read row 0 with weight 0, so the four loads of a macro
                // trip are independent and all in flight before the first FMA
                const int p = ok ? f >> 2 : 0;
                bq[u] = ok ? b : 0.f;
                const float4 *src = (he && cc == 0) ? emg + p : feat + ((int64_t)p * ldf4 + (cc - he));
                v[u] = *src;
                if (LPV == 64 && c + 64 < CH && ok) fma4(a1, b, feat[(int64_t)p * ldf4 + (c + 64 - he)]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) { fma4(a0, bq[u], v[u]); w += bq[u]; }
        }
    }
    // fold the entry slots: lane c (< CH, slot 0) adds lanes c + k*CH of its group
    for (int k = 1; k < EPT; ++k) {
        const int src = gb + ((lv + k * CH) & (LPV - 1));
        const float4 o = make_float4(__shfl(a0.x, src), __shfl(a0.y, src), __shfl(a0.z, src), __shfl(a0.w, src));
        const float ow = __shfl(w, src);
        if (e == 0) { a0.x += o.x; a0.y += o.y; a0.z += o.z; a0.w += o.w; w += ow; }
    }
    if (e != 0 || !have) return;
    // w of slot 0 was accumulated by every lane of the slot identically
    const float nrm = normalize ? 1.0f / (w + 1e-5f) : 1.0f;          // (use_norm = False, bilateralNN.py:196: the plain sparse sum)
    float4 *dst = splat + (int64_t)h * lds4;                           // (lds4 = CH for the splat; the slice's backward has its own row stride)
    dst[c] = make_float4(a0.x * nrm, a0.y * nrm, a0.z * nrm, a0.w * nrm);
    if (LPV == 64 && c + 64 < CH) dst[c + 64] = make_float4(a1.x * nrm, a1.y * nrm, a1.z * nrm, a1.w * nrm);
    if (wsum && c == 0) wsum[h] = w;
}

// backward of the splat w.r.t. the feature part of the rows (el_minus_gr carries no gradient, generate_data.py:119):
//   gfeat[p][c] = sum_r bary[p][r] / (wsum[off[p][r]] + 1e-5) * gsplat[off[p][r]][coff + c]
__global__ void __launch_bounds__(TPB)
k_splat_bwd(const float4 *__restrict__ gsplat, int c4, int coff4, const float *__restrict__ wsum, int cf4,
            const float4 *__restrict__ bary, const int4 *__restrict__ off, int n, float4 *__restrict__ gfeat, int64_t ldg4, int normalize) {
    const int64_t total = (int64_t)n * cf4;
    const int64_t nblocks = (total + TPB - 1) / TPB;
    const int64_t blk = xcd_band_block(blockIdx.x, nblocks);
    if (blk < 0) return;
    const int64_t i = blk * TPB + threadIdx.x;
    if (i >= total) return;
    const int p = (int)(i / cf4), c = (int)(i - (int64_t)p * cf4);
    const int4 o = off[p];
    const float4 b = bary[p];
    const int oo[4] = {o.x, o.y, o.z, o.w};
    const float bb[4] = {b.x, b.y, b.z, b.w};
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float w = normalize ? bb[r] * (1.0f / (wsum[oo[r]] + 1e-5f)) : bb[r];
        fma4(a, w, gsplat[(int64_t)oo[r] * c4 + coff4 + c]);
    }
    gfeat[(int64_t)p * ldg4 + c] = a;
}

// ---- adjoint of the neighbour gather (bilateralNN.py:240-242): dst[h][c] = sum over (m, t) with table[m][t] == h of
// src[m][t*C + c].  The exact part of the neighbour relation is symmetric - table[m][t] == h  <=>  table[h][inv(t)] == m,
// inv(t) = index of the negated offset (generate_data.py:44-52: t <-> 15 - t for t >= 1) - so the adjoint is a gather through
// the SAME table; the aliased hits of key2int (lattice.hip k_neighbors: marked in column 15, listed in alist) are excluded
// here and added by k_table_alias_add.
template <int G>
__global__ void __launch_bounds__(TPB)
k_table_gather_t(const float *__restrict__ src, int C, const int *__restrict__ table, int H, float *__restrict__ dst) {
    constexpr int S = 64 / G;
    const int c4n = C >> 2;
    const int lane = threadIdx.x & 63, g = lane % G, sl = lane / G;
    const int64_t nblocks = ((int64_t)H + TPB / 64 - 1) / (TPB / 64);
    const int64_t blk = xcd_band_block(blockIdx.x, nblocks);
    if (blk < 0) return;
    const int h = (int)(blk * (TPB / 64) + (threadIdx.x >> 6));
    if (h >= H) return;
    const int tv = lane < 16 ? table[(int64_t)h * 16 + lane] : -1;
    const int amask = __shfl(tv, 15);
    const int64_t ld = 15LL * C;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
    for (int t0 = 0; t0 < 15; t0 += S) {             // (uniform trip count: every lane takes part in the shuffle)
        const int t = t0 + sl;
        const int m = __shfl(tv, t & 15);
        if (t >= 15 || m < 0 || (amask >> t & 1)) continue;
        const int ti = t == 0 ? 0 : 15 - t;
        const float4 *row = reinterpret_cast<const float4 *>(src + (int64_t)m * ld + (int64_t)ti * C);
        if (g < c4n) { float4 f = row[g]; a0.x += f.x; a0.y += f.y; a0.z += f.z; a0.w += f.w; }
        if (g + G < c4n) { float4 f = row[g + G]; a1.x += f.x; a1.y += f.y; a1.z += f.z; a1.w += f.w; }
    }
#pragma unroll
    for (int o = G; o < 64; o <<= 1) {
        a0.x += __shfl_xor(a0.x, o); a0.y += __shfl_xor(a0.y, o); a0.z += __shfl_xor(a0.z, o); a0.w += __shfl_xor(a0.w, o);
        a1.x += __shfl_xor(a1.x, o); a1.y += __shfl_xor(a1.y, o); a1.z += __shfl_xor(a1.z, o); a1.w += __shfl_xor(a1.w, o);
    }
    if (sl != 0) return;
    float4 *d = reinterpret_cast<float4 *>(dst + (int64_t)h * C);
    if (g < c4n) d[g] = a0;
    if (g + G < c4n) d[g + G] = a1;
}

// ---- the aliased neighbour hits (a handful per level; k_neighbors / k_lat_nbr list them in arrival order, which varies from run
// to run).  Both kernels below apply them in a FIXED order without atomics: every block loads the records, ranks them by their
// (entry, target) key in LDS, and owns the targets with target % gridDim.x == blockIdx.x - it walks the sorted records and adds the
// ones that land on its own targets, one after the other.
constexpr int ALIAS_LDS = 4096;

__device__ __forceinline__ int load_sorted_alias(const int2 *__restrict__ alist, const int *__restrict__ n_alias, int alias_cap,
                                                 int2 *sorted) {
    const int na = min(min(*n_alias, alias_cap), ALIAS_LDS);
    for (int i = threadIdx.x; i < na; i += TPB) {
        const int2 a = alist[i];
        int r = 0;
        for (int j = 0; j < na; ++j) {              // (records are distinct: an entry is listed once)
            const int2 o = alist[j];
            r += (o.x < a.x || (o.x == a.x && o.y < a.y)) ? 1 : 0;
        }
        sorted[r] = a;
    }
    __syncthreads();
    return na;
}

// dst[target][c] += src[m][t*C + c]   (adjoint of the neighbour gather on an explicit [H][15 C] intermediate)
__global__ void __launch_bounds__(TPB)
k_table_alias_add(const float *__restrict__ src, int C, const int2 *__restrict__ alist, const int *__restrict__ n_alias,
                  int alias_cap, float *__restrict__ dst) {
    __shared__ int2 sorted[ALIAS_LDS];
    const int na = load_sorted_alias(alist, n_alias, alias_cap, sorted);
    for (int k = 0; k < na; ++k) {
        const int2 a = sorted[k];
        if (a.y % (int)gridDim.x != (int)blockIdx.x) continue;
        const int m = a.x >> 4, t = a.x & 15;
        for (int c = threadIdx.x; c < C; c += TPB) dst[(int64_t)a.y * C + c] += src[((int64_t)m * 15 + t) * C + c];
        __syncthreads();                            // (the next record may hit the same target)
    }
}

// dx[target][c] += sum_n dy[m][n] * w[(n*C + c)*15 + t]   (the same adjoint when the gather and the convolution are one GEMM)
__global__ void __launch_bounds__(TPB)
k_blur_dgrad_alias(const float *__restrict__ dy, int64_t ldy, int N, const float *__restrict__ w, int C,
                   const int2 *__restrict__ alist, const int *__restrict__ n_alias, int alias_cap, float *__restrict__ dx,
                   int64_t ldx) {
    __shared__ int2 sorted[ALIAS_LDS];
    const int na = load_sorted_alias(alist, n_alias, alias_cap, sorted);
    for (int k = 0; k < na; ++k) {
        const int2 a = sorted[k];
        if (a.y % (int)gridDim.x != (int)blockIdx.x) continue;
        const int m = a.x >> 4, t = a.x & 15;
        const float *row = dy + (int64_t)m * ldy;
        for (int c = threadIdx.x; c < C; c += TPB) {
            float acc = 0.f;
            for (int n = 0; n < N; ++n) acc += row[n] * w[((int64_t)n * C + c) * 15 + t];
            dx[(int64_t)a.y * ldx + c] += acc;
        }
        __syncthreads();
    }
}


// ---- BCL slice (bilateralNN.py:251-263): lattice rows back onto points.  One thread per (point, 16-byte chunk): four C-wide rows
// gathered, weighted in the order r = 0..3, then the bias.  An offset outside [0, H) contributes nothing (the reference would wrap
// a -1 to the last vertex; efgh_offsets_invert counts such entries - here they are only kept from reading out of bounds).
__global__ void __launch_bounds__(TPB)
k_slice(const float4 *__restrict__ feat, int64_t ldf4, int H, const float4 *__restrict__ bary, const int4 *__restrict__ off, int n,
        int c4, const float4 *__restrict__ bias, float4 *__restrict__ out, int64_t ldo4, int ooff4) {
    const int64_t total = (int64_t)n * c4;
    const int64_t nblocks = (total + TPB - 1) / TPB;
    const int64_t blk = xcd_band_block(blockIdx.x, nblocks);
    if (blk < 0) return;
    const int64_t i = blk * TPB + threadIdx.x;
    if (i >= total) return;
    const int p = (int)(i / c4), c = (int)(i - (int64_t)p * c4);
    const int4 o = off[p];
    const float4 b = bary[p];
    const int oo[4] = {o.x, o.y, o.z, o.w};
    const float bb[4] = {b.x, b.y, b.z, b.w};
    float4 v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {                          // (the four row loads are independent: all in flight before the first FMA)
        const bool ok = (unsigned)oo[r] < (unsigned)H;
        v[r] = ok ? feat[(int64_t)oo[r] * ldf4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int r = 0; r < 4; ++r) fma4(a, bb[r], v[r]);
    if (bias) { const float4 bi = bias[c]; a.x += bi.x; a.y += bi.y; a.z += bi.z; a.w += bi.w; }
    out[(int64_t)p * ldo4 + ooff4 + c] = a;
}

// ---- the inverse of an `off` array that did not come out of the lattice build (out points of the slice): vertex -> ascending list
// of its flat positions f = 4p + r, in the build's own format.  Histogram (integer atomics), exclusive scan, scatter in arrival
// order into a scratch list, then every entry is RANKED among the entries of its vertex (they are distinct) and stored at its
// rank: the result does not depend on the arrival order.  Work of the last pass: sum over the vertices of (list length)^2
// comparisons, spread over all entries (no long tail on one wave).
constexpr int SCAN_ITEMS = 4, SCAN_TILE = TPB * SCAN_ITEMS;

__global__ void __launch_bounds__(TPB)
k_inv_hist(const int *__restrict__ off, int64_t nf, int H, int *__restrict__ count, int *__restrict__ err) {
    const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (f >= nf) return;
    const int h = off[f];
    if ((unsigned)h < (unsigned)H) atomicAdd(count + h, 1);
    else atomicAdd(err, 1);
}

// exclusive scan of v over the block's TPB threads (wave shuffles, the four wave totals through LDS) -> (prefix, block total)
__device__ __forceinline__ int block_excl_scan(int v, int *wtot, int &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                // (wtot may still be read from a previous call)
    if (lane == 63) wtot[wv] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < TPB / 64; ++k) { if (k < wv) base += wtot[k]; total += wtot[k]; }
    return base + inc - v;
}

// tile-local exclusive scan of the counts -> vseg (start within the tile, length); the tile's total -> tsum
__global__ void __launch_bounds__(TPB)
k_inv_scan_tiles(const int *__restrict__ count, int H, int2 *__restrict__ vseg, int *__restrict__ tsum) {
    __shared__ int wtot[TPB / 64];
    const int64_t h0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    int cnt[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) { cnt[k] = h0 + k < H ? count[h0 + k] : 0; s += cnt[k]; }
    int total;
    int pre = block_excl_scan(s, wtot, total);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (h0 + k < H) vseg[h0 + k] = make_int2(pre, cnt[k]);
        pre += cnt[k];
    }
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// one block: exclusive scan of the tile totals in place
__global__ void __launch_bounds__(TPB)
k_inv_scan_totals(int *__restrict__ tsum, int ntiles) {
    __shared__ int wtot[TPB / 64];
    int carry = 0;
    for (int base = 0; base < ntiles; base += TPB) {
        const int i = base + threadIdx.x;
        const int v = i < ntiles ? tsum[i] : 0;
        int total;
        const int pre = block_excl_scan(v, wtot, total);
        if (i < ntiles) tsum[i] = carry + pre;
        carry += total;
    }
}

// vseg starts made global; the counts become the scatter's cursors (zero again)
__global__ void __launch_bounds__(TPB)
k_inv_scan_apply(int2 *__restrict__ vseg, int H, const int *__restrict__ tsum, int *__restrict__ count) {
    const int64_t h = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (h >= H) return;
    vseg[h].x += tsum[h / SCAN_TILE];
    count[h] = 0;
}

__global__ void __launch_bounds__(TPB)
k_inv_scatter(const int *__restrict__ off, int64_t nf, int H, const int2 *__restrict__ vseg, int *__restrict__ cursor,
              int *__restrict__ tmp) {
    const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (f >= nf) return;
    const int h = off[f];
    if ((unsigned)h >= (unsigned)H) return;
    tmp[vseg[h].x + atomicAdd(cursor + h, 1)] = (int)f;          // (slot < length: the histogram counted the same entries)
}

__global__ void __launch_bounds__(TPB)
k_inv_rank(const int *__restrict__ off, int64_t nf, int H, const int2 *__restrict__ vseg, const int *__restrict__ tmp,
           int *__restrict__ list) {
    const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (f >= nf) return;
    const int h = off[f];
    if ((unsigned)h >= (unsigned)H) return;
    const int2 seg = vseg[h];
    int r = 0;
    for (int j = 0; j < seg.y; ++j) r += tmp[seg.x + j] < (int)f ? 1 : 0;
    list[seg.x + r] = (int)f;
}

// ---- bias gradient of the slice: column sums of gout's channel slice, a two-stage fold with a fixed tree (no atomics; a running
// sum of a few thousand like-signed values drifts by far more than a tree's log2 n roundings).  Stage 1: block b sums the rows
// [b*rows_per, (b+1)*rows_per): thread (row slot, chunk) takes every (TPB / c4)-th row of them in ascending order, the row slots are
// folded pairwise in LDS.  Stage 2: one block per chunk folds the <= 4 TPB block partials: every TPB-th one per thread, then pairwise.
__device__ __forceinline__ void add4(float4 &a, const float4 &v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }

__global__ void __launch_bounds__(TPB)
k_colsum_part(const float4 *__restrict__ g, int64_t ld4, int off4, int n, int c4, int rows_per, float4 *__restrict__ part) {
    __shared__ float4 sm[TPB];
    const int slots = TPB / c4, sl = threadIdx.x / c4, c = threadIdx.x - sl * c4;
    const int r0 = blockIdx.x * rows_per, r1 = min(n, r0 + rows_per);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (sl < slots)
        for (int p = r0 + sl; p < r1; p += slots) add4(a, g[(int64_t)p * ld4 + off4 + c]);
    sm[threadIdx.x] = a;
    int half = 1;
    while (half * 2 < slots) half *= 2;                 // (the largest power of two below the slot count; 0 rounds at slots == 1)
    for (int s = half; s > 0 && slots > 1; s >>= 1) {
        __syncthreads();
        if (sl < s && sl + s < slots) { add4(a, sm[(sl + s) * c4 + c]); sm[threadIdx.x] = a; }
    }
    if (sl == 0) part[(int64_t)blockIdx.x * c4 + c] = a;
}

__global__ void __launch_bounds__(TPB)
k_colsum_fold(const float4 *__restrict__ part, int nparts, int c4, float4 *__restrict__ dst) {
    __shared__ float4 sm[TPB];
    const int c = blockIdx.x, t = threadIdx.x;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = t; i < nparts; i += TPB) add4(a, part[(int64_t)i * c4 + c]);      // (<= COLSUM_PARTS / TPB terms)
    sm[t] = a;
    for (int s = TPB / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) { add4(a, sm[t + s]); sm[t] = a; }
    }
    if (t == 0) dst[c] = a;
}

constexpr int COLSUM_PARTS = 4 * TPB;            // most stage-1 blocks of the bias gradient (efgh_slice_bwd_workspace)

}  // namespace

extern "C" int efgh_splat_gather(const float *emg, const float *feat, int64_t ldf, int32_t Cf, const float *bary,
                                 const int32_t *list, const int32_t *vseg, int32_t H, int32_t avg_len,
                                 int32_t lanes_per_vertex, int32_t normalize, float *splat, float *wsum, void *stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EFGH_CHECK_ARG(feat && bary && list && vseg && splat && wsum && H > 0 && Cf > 0 && Cf % 4 == 0 && Cf <= 508 && ldf % 4 == 0);
    const int CH = (emg ? 1 : 0) + Cf / 4;
    // two vertices per wave when a row fits half a wave and the lists are short (avg_len = 4n/H entries per vertex)
    // two vertices per wave when two rows fit a wave's lanes and the lists are short: the kernel is bound by the vertices in
    // flight x the dependent round trips, not by the lanes (measured, level 1 of the bench scene: 46 vs 60 us)
    int lpv = lanes_per_vertex;
    if (lpv == 0) lpv = (CH <= 32 && avg_len <= 32) ? 32 : 64;
    EFGH_CHECK_ARG(lpv == 64 || (lpv == 32 && CH <= 32) || (lpv == 16 && CH <= 16));
    const int vpb = TPB / lpv;
    const int64_t nblocks = ((int64_t)H + vpb - 1) / vpb;
    const int64_t grid = (nblocks + 7) / 8 * 8;
    if (lpv == 16)
        k_splat_gather<16><<<(unsigned)grid, TPB, 0, st>>>((const float4 *)emg, (const float4 *)feat, ldf / 4, Cf / 4, bary, list,
                                                           (const int2 *)vseg, H, (float4 *)splat, CH, wsum, normalize);
    else if (lpv == 32)
        k_splat_gather<32><<<(unsigned)grid, TPB, 0, st>>>((const float4 *)emg, (const float4 *)feat, ldf / 4, Cf / 4, bary, list,
                                                           (const int2 *)vseg, H, (float4 *)splat, CH, wsum, normalize);
    else
        k_splat_gather<64><<<(unsigned)grid, TPB, 0, st>>>((const float4 *)emg, (const float4 *)feat, ldf / 4, Cf / 4, bary, list,
                                                           (const int2 *)vseg, H, (float4 *)splat, CH, wsum, normalize);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_splat_bwd(const float *gsplat, int32_t C, int32_t coff, const float *wsum, int32_t Cf, const float *bary,
                              const int32_t *off, int32_t n, float *gfeat, int64_t ldg, int32_t normalize, void *stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EFGH_CHECK_ARG(gsplat && wsum && bary && off && gfeat && n > 0 && C % 4 == 0 && coff % 4 == 0 && Cf % 4 == 0 && Cf > 0 &&
                   coff + Cf <= C && ldg % 4 == 0);
    const int64_t nblocks = ((int64_t)n * (Cf / 4) + TPB - 1) / TPB;
    const int64_t grid = (nblocks + 7) / 8 * 8;
    k_splat_bwd<<<(unsigned)grid, TPB, 0, st>>>((const float4 *)gsplat, C / 4, coff / 4, wsum, Cf / 4, (const float4 *)bary,
                                                (const int4 *)off, n, (float4 *)gfeat, ldg / 4, normalize);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_table_gather_transposed(const float *src, const int32_t *table, int32_t H, int32_t C, const int32_t *alist,
                                            const int32_t *n_alias, int32_t alias_cap, float *dst, void *stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EFGH_CHECK_ARG(src && table && dst && alist && n_alias && H > 0 && C > 0 && C % 4 == 0 && C <= 512 && alias_cap > 0 && alias_cap <= ALIAS_LDS);
    const int64_t nblocks = ((int64_t)H + TPB / 64 - 1) / (TPB / 64);
    const unsigned grid = (unsigned)((nblocks + 7) / 8 * 8);
    const int c4n = C / 4;
    if (c4n <= 16) k_table_gather_t<16><<<grid, TPB, 0, st>>>(src, C, table, H, dst);
    else if (c4n <= 32) k_table_gather_t<32><<<grid, TPB, 0, st>>>(src, C, table, H, dst);
    else k_table_gather_t<64><<<grid, TPB, 0, st>>>(src, C, table, H, dst);
    k_table_alias_add<<<64, TPB, 0, st>>>(src, C, (const int2 *)alist, n_alias, alias_cap, dst);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_blur_dgrad_alias(const float *dy, int64_t ldy, int32_t N, const float *w, int32_t C, const int32_t *alist,
                                     const int32_t *n_alias, int32_t alias_cap, float *dx, int64_t ldx, void *stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EFGH_CHECK_ARG(dy && w && alist && n_alias && dx && N > 0 && C > 0 && alias_cap > 0 && alias_cap <= ALIAS_LDS);
    k_blur_dgrad_alias<<<64, TPB, 0, st>>>(dy, ldy, N, w, C, (const int2 *)alist, n_alias, alias_cap, dx, ldx);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

// ---- slice step of the BCL (bilateralNN.py:248-263): out[p][ooff + c] = sum_r bary[p][r] * feat[off[p][r]][c] (+ bias[c])
extern "C" int efgh_slice(const float *feat, int64_t ldf, int32_t H, const float *bary, const int32_t *off, int32_t n_out, int32_t C,
                          const float *bias, float *out, int64_t ldo, int32_t ooff, void *stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EFGH_CHECK_ARG(feat && bary && off && out && H > 0 && n_out > 0 && C > 0 && C % 4 == 0 && ldf % 4 == 0 && ldf >= C &&
                   ldo % 4 == 0 && ooff >= 0 && ooff % 4 == 0 && (int64_t)ooff + C <= ldo);
    const int64_t nblocks = ((int64_t)n_out * (C / 4) + TPB - 1) / TPB;
    const int64_t grid = (nblocks + 7) / 8 * 8;
    EFGH_CHECK_ARG(grid < (1ll << 31));
    k_slice<<<(unsigned)grid, TPB, 0, st>>>((const float4 *)feat, ldf / 4, H, (const float4 *)bary, (const int4 *)off, n_out, C / 4,
                                            (const float4 *)bias, (float4 *)out, ldo / 4, ooff / 4);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

static inline int64_t inv_align(int64_t b) { return (b + 255) / 256 * 256; }
static inline int64_t inv_tiles(int64_t H) { return (H + SCAN_TILE - 1) / SCAN_TILE; }

extern "C" int64_t efgh_offsets_invert_workspace(int32_t n_out, int32_t H) {
    if (n_out <= 0 || H <= 0) return 0;
    // counts / cursors [H], tile totals, the arrival-order list [4 n_out]
    return inv_align(4ll * H) + inv_align(4ll * inv_tiles(H)) + inv_align(16ll * n_out);
}

// ---- inverse lists of an out-point set (the slice's backward walks them): what the lattice build leaves for its own points
// (lattice.hip: list, vseg), rebuilt from `off` alone
extern "C" int efgh_offsets_invert(const int32_t *off, int32_t n_out, int32_t H, int32_t *vseg, int32_t *list, int32_t *err,
                                   void *workspace, void *stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EFGH_CHECK_ARG(off && vseg && list && err && workspace && n_out > 0 && H > 0 && n_out <= (1 << 29) &&
                   ((uintptr_t)workspace & 255) == 0);
    const int64_t nf = 4ll * n_out;
    const int ntiles = (int)inv_tiles(H);
    char *ws = (char *)workspace;
    int *count = (int *)ws;
    int *tsum = (int *)(ws + inv_align(4ll * H));
    int *tmp = (int *)(ws + inv_align(4ll * H) + inv_align(4ll * ntiles));
    if (hipMemsetAsync(count, 0, 4ll * H, st) != hipSuccess || hipMemsetAsync(err, 0, 4, st) != hipSuccess) {
        efgh_set_error("%s:%d: hipMemsetAsync failed", __FILE__, __LINE__);
        return EFGH_E_LAUNCH;
    }
    const unsigned gf = (unsigned)((nf + TPB - 1) / TPB), gh = (unsigned)(((int64_t)H + TPB - 1) / TPB);
    k_inv_hist<<<gf, TPB, 0, st>>>(off, nf, H, count, err);
    k_inv_scan_tiles<<<(unsigned)ntiles, TPB, 0, st>>>(count, H, (int2 *)vseg, tsum);
    k_inv_scan_totals<<<1, TPB, 0, st>>>(tsum, ntiles);
    k_inv_scan_apply<<<gh, TPB, 0, st>>>((int2 *)vseg, H, tsum, count);
    k_inv_scatter<<<gf, TPB, 0, st>>>(off, nf, H, (const int2 *)vseg, count, tmp);
    k_inv_rank<<<gf, TPB, 0, st>>>(off, nf, H, (const int2 *)vseg, tmp, list);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int64_t efgh_slice_bwd_workspace(int32_t C) { return C > 0 ? 4ll * COLSUM_PARTS * C : 0; }

// ---- backward of the slice w.r.t. the lattice rows (autograd of bilateralNN.py:251-257) as a gather over the vertex lists of the
// out points, and w.r.t. the bias (:260-261): k_splat_gather without el_minus_gr and without the density factor
extern "C" int efgh_slice_bwd(const float *gout, int64_t ldo, int32_t ooff, int32_t C, const float *bary, const int32_t *list,
                              const int32_t *vseg, int32_t H, int32_t n_out, int32_t lanes_per_vertex, float *gfeat, int64_t ldg,
                              float *gbias, void *workspace, void *stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EFGH_CHECK_ARG(gout && bary && list && vseg && gfeat && H > 0 && n_out > 0 && C > 0 && C % 4 == 0 && C <= 508 && ldo % 4 == 0 &&
                   ooff >= 0 && ooff % 4 == 0 && (int64_t)ooff + C <= ldo && ldg % 4 == 0 && ldg >= C && (!gbias || workspace));
    const int CH = C / 4;
    const int avg_len = (int)std::max<int64_t>(1, 4ll * n_out / H);
    int lpv = lanes_per_vertex;
    if (lpv == 0) lpv = (CH <= 32 && avg_len <= 32) ? 32 : 64;          // (the splat's rule, efgh_splat_gather)
    EFGH_CHECK_ARG(lpv == 64 || (lpv == 32 && CH <= 32) || (lpv == 16 && CH <= 16));
    const int vpb = TPB / lpv;
    const int64_t nblocks = ((int64_t)H + vpb - 1) / vpb;
    const int64_t grid = (nblocks + 7) / 8 * 8;
    EFGH_CHECK_ARG(grid < (1ll << 31));
    const float4 *rows = (const float4 *)(gout + ooff);
    if (lpv == 16)
        k_splat_gather<16><<<(unsigned)grid, TPB, 0, st>>>(nullptr, rows, ldo / 4, CH, bary, list, (const int2 *)vseg, H,
                                                           (float4 *)gfeat, ldg / 4, nullptr, 0);
    else if (lpv == 32)
        k_splat_gather<32><<<(unsigned)grid, TPB, 0, st>>>(nullptr, rows, ldo / 4, CH, bary, list, (const int2 *)vseg, H,
                                                           (float4 *)gfeat, ldg / 4, nullptr, 0);
    else
        k_splat_gather<64><<<(unsigned)grid, TPB, 0, st>>>(nullptr, rows, ldo / 4, CH, bary, list, (const int2 *)vseg, H,
                                                           (float4 *)gfeat, ldg / 4, nullptr, 0);
    if (gbias) {
        const int rows_per = (n_out + COLSUM_PARTS - 1) / COLSUM_PARTS;
        const int nparts = (n_out + rows_per - 1) / rows_per;
        k_colsum_part<<<(unsigned)nparts, TPB, 0, st>>>((const float4 *)gout, ldo / 4, ooff / 4, n_out, CH, rows_per, (float4 *)workspace);
        k_colsum_fold<<<(unsigned)CH, TPB, 0, st>>>((const float4 *)workspace, nparts, CH, (float4 *)gbias);
    }
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}
