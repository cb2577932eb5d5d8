// 3x3 convolutions with FOUR input channels per tap and 32..128 outputs on fp32 MFMA (gfx950): the RGB / range / depth
// input layers (nets/vgg.py:77 first layer, nets/gnet.py:21,80) and the data gradient of G's 1- and 2-channel transposed
// heads (a stride-2 3x3 convolution over the 4-channel-padded output gradient).  K = 36 only, so the layer is bound by
// writing (forward) or reading (weight gradient) the wide side; the generic implicit-GEMM kernel spends its time on the
// per-quad gather arithmetic instead (12-26 TFLOP/s, 1.9 TB/s).  Here one WAVE owns 32 consecutive output pixels of
// an image row (no workgroup barrier anywhere in the loop): the three input rows go to its LDS slice once (two planes of channel pairs, so that the 32 pixels of an MFMA operand
// are 256 contiguous bytes), the 36 x N weights live in registers for the whole (persistent) workgroup, and each wave
// runs 18 v_mfma_f32_32x32x2_f32 per 32 pixels x 32 outputs: MFMA step (tap t, e) contracts channels {e, 2 + e}.
// Epilogue = that of k_gather_gemm (bias, BN statistics of the pre-activation value, scale/shift, residual, activation).
//
// Weight gradient: dW[n][t][c] = sum_p G[p][n] * X[p + tap t][c] on v_mfma_f32_16x16x4_f32 (k = 4 output pixels per
// instruction; 36 columns = 2.25 -> 3 column tiles), G read once straight from global memory, per-workgroup partial sums
// combined with fp32 atomics.
#include "common.h"


namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TP = 32;                  // output pixels per unit: one wave, no workgroup barrier in the loop
constexpr int LWMAX = (TP - 1) * 2 + 3; // staged input pixels per row at stride 2
constexpr int WAVES = 4;

struct C4Args {
    const float *A; long long lda;
    int B, Hin, Win, Ho, Wo, s;
    const float *W; int N;
    const float *bias, *scale, *shift, *residual; long long ldr;
    int act; float slope;
    float *out; long long ldo;
    float *stats;
    long long units; int jblocks;
    const float *G; long long ldg; float *dW;       // wgrad
    // train-mode pooled layer (k_c4_conv_pool<.., true>, k_c4_pool_bwd_draw): BatchNorm's per-channel vectors, the pooled gradient
    const float *mean, *invstd, *coef; const double *m1, *m2;
    const float *dyp; float *raw_win, *draw;
};

__device__ __forceinline__ void unit_coords(const C4Args &p, long long unit, long long &row, int &i, long long &b, int &j0) {
    const int jb = (int)(unit % p.jblocks);
    row = unit / p.jblocks;                          // b * Ho + i
    i = (int)(row % p.Ho); b = row / p.Ho;
    j0 = jb * TP;
}

// the (up to) four staged pixels of this lane for one unit: flat index idx = lane + 64 q over [3][LW]
__device__ __forceinline__ float4 load_px(const C4Args &p, int idx, int LW, int i, long long b, int j0) {
    const int kh = idx / LW, x = idx - kh * LW;
    const int yin = p.s * i - 1 + kh, xin = p.s * j0 - 1 + x;
    if (kh < 3 && (unsigned)yin < (unsigned)p.Hin && (unsigned)xin < (unsigned)p.Win)
        return *reinterpret_cast<const float4 *>(p.A + ((b * p.Hin + yin) * p.Win + xin) * p.lda);
    return make_float4(0.f, 0.f, 0.f, 0.f);
}

// LDS traffic of ONE wave: the hardware keeps a wave's LDS instructions in order, the fences keep the compiler from moving them
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// STORE = false: the statistics-only pass of a train-mode pooled layer (efgh_c4_conv3x3_stats).  Same units, same MFMA order, same
// order of the column sums - the statistics rows have the bits of the storing launch; the transpose tile and the output stores are
// compiled out.
template <int NT, bool RES, bool STORE = true>
__global__ void __launch_bounds__(64 * WAVES, 2) k_c4_conv(const C4Args p) {
    static_assert(STORE || !RES, "the statistics-only pass has no residual");
    __shared__ float2 Pw[WAVES][3][2][LWMAX + 1];
    __shared__ float red[2][WAVES][NT * 32];
    constexpr int TPITCH = 40;                       // floats per row of the transpose tile (h = 0 / 1 rows land on disjoint banks)
    __shared__ __attribute__((aligned(16))) float Tw[WAVES][STORE ? 32 * TPITCH : 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int LW = (TP - 1) * p.s + 3;
    float2 (*P)[2][LWMAX + 1] = Pw[wave];
    float *T = Tw[wave];

    float2 bw[9][NT];
    float bi[NT], sc[NT], sf[NT], s1[NT], s2[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = 32 * j + r;
#pragma unroll
        for (int t = 0; t < 9; ++t) bw[t][j] = *reinterpret_cast<const float2 *>(p.W + ((long long)n * 9 + t) * 4 + 2 * h);
        bi[j] = p.bias ? p.bias[n] : 0.f;
        sc[j] = p.scale ? p.scale[n] : 1.f;
        sf[j] = p.shift ? p.shift[n] : 0.f;
        s1[j] = 0.f; s2[j] = 0.f;
    }
    const float neg = p.act == 1 ? 0.f : (p.act == 2 ? p.slope : 1.f);

    // the weight loads are complete before the loop (an empty asm that reads them): otherwise the loop body inherits their
    // outstanding-load state and waits on the NEXT unit's prefetch in the middle of the MFMAs
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t) asm volatile("" ::"v"(bw[t][j].x), "v"(bw[t][j].y));

    const long long nwaves = (long long)gridDim.x * WAVES;
    long long unit = (long long)blockIdx.x * WAVES + wave;
    long long row = 0, b = 0; int i = 0, j0 = 0;     // coordinates of the unit whose pixels are in pf0..3
    long long crow = 0; int cj0 = 0;                 // ... of the unit staged in LDS
    float4 pf0, pf1, pf2, pf3;                       // (named registers: no scratch)
#define EFGH_FETCH(u)                                                                    \
    {                                                                                   \
        unit_coords(p, u, row, i, b, j0);                                               \
        pf0 = load_px(p, lane, LW, i, b, j0); pf1 = load_px(p, lane + 64, LW, i, b, j0); \
        pf2 = load_px(p, lane + 128, LW, i, b, j0); pf3 = load_px(p, lane + 192, LW, i, b, j0); \
    }
#define EFGH_PUT(q, v)                                                                   \
    {                                                                                   \
        const int idx = lane + 64 * q;                                                  \
        if (idx < 3 * LW) {                                                             \
            const int kh = idx / LW, x = idx - kh * LW;                                 \
            P[kh][0][x] = make_float2(v.x, v.y); P[kh][1][x] = make_float2(v.z, v.w);   \
        }                                                                               \
    }
#define EFGH_STAGE()                                                                     \
    {                                                                                   \
        crow = row; cj0 = j0;                                                           \
        EFGH_PUT(0, pf0) EFGH_PUT(1, pf1) EFGH_PUT(2, pf2) EFGH_PUT(3, pf3)             \
    }
    if (unit < p.units) {
        EFGH_FETCH(unit)
        EFGH_STAGE()
        if (unit + nwaves < p.units) EFGH_FETCH(unit + nwaves)
    }
    // per unit: operand reads + MFMAs, THEN the LDS refill with the next unit (its loads are one MFMA phase old, and so are
    // the previous unit's stores: the vmcnt(0) in front of the refill costs nothing), the loads of the unit after that, and
    // only then this unit's stores
    for (; unit < p.units; unit += nwaves) {
        const long long orow0 = crow; const int oj0 = cj0;
        wave_lds_sync();
        f32x16 acc[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
        const int px = r * p.s;
        float2 af[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) af[t] = P[t / 3][h][px + t % 3];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[t].x, bw[t][j].x, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[t].y, bw[t][j].y, acc[j], 0, 0, 0);
            }
        }
        wave_lds_sync();
        if (unit + nwaves < p.units) {
            EFGH_STAGE()
            if (unit + 2 * nwaves < p.units) EFGH_FETCH(unit + 2 * nwaves)
        }
        // branch-free epilogue: act(v) = max(v, 0) + neg * min(v, 0) with neg = 0 (ReLU) / slope (leaky) / 1 (none).  The accumulator
        // layout has one output channel per lane (4-byte stores); every 32 x 32 block goes through a wave-private LDS tile
        // [pixel][channel] and leaves as 16-byte stores, eight lanes per pixel row (128 contiguous bytes)
        const bool full = oj0 + TP <= p.Wo;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            // the residual is read in the STORE layout (16 bytes per lane, issued before the tile is even written, so the loads
            // overlap the LDS round trip): the first version read it in the accumulator layout - sixteen dependent 4-byte loads
            // per lane and block in a wave that has nobody to hide their latency behind (3.6 ms instead of 0.6 on G's depth head)
            float4 rr[4];
            if (RES) {
#pragma unroll
                for (int pass = 0; pass < 4; ++pass) {
                    const int pl = 8 * pass + (lane >> 3), c4 = (lane & 7) * 4;
                    rr[pass] = (full || oj0 + pl < p.Wo)
                                   ? *reinterpret_cast<const float4 *>(p.residual + (orow0 * p.Wo + oj0 + pl) * p.ldr + 32 * j + c4)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            if (STORE) wave_lds_sync();              // the tile's previous readers are done
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int pl = (q & 3) + 8 * (q >> 2) + 4 * h;
                const bool ok = full || oj0 + pl < p.Wo;
                float v = acc[j][q] + bi[j];
                if (ok) { s1[j] += v; s2[j] = fmaf(v, v, s2[j]); }
                if (!STORE) continue;
                v = fmaf(v, sc[j], sf[j]);
                T[pl * TPITCH + r] = RES ? v : act_neg(v, neg);
            }
            if (!STORE) continue;
            wave_lds_sync();
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int pl = 8 * pass + (lane >> 3), c4 = (lane & 7) * 4;
                float4 v = *reinterpret_cast<const float4 *>(&T[pl * TPITCH + c4]);
                if (RES) {
                    v.x += rr[pass].x; v.y += rr[pass].y; v.z += rr[pass].z; v.w += rr[pass].w;
                    v.x = act_neg(v.x, neg); v.y = act_neg(v.y, neg);
                    v.z = act_neg(v.z, neg); v.w = act_neg(v.w, neg);
                }
                if (full || oj0 + pl < p.Wo)
                    *reinterpret_cast<float4 *>(p.out + (orow0 * p.Wo + oj0 + pl) * p.ldo + 32 * j + c4) = v;
            }
        }
    }
#undef EFGH_FETCH
#undef EFGH_PUT
#undef EFGH_STAGE
    if (p.stats) {                                   // one statistics row per workgroup
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            s1[j] += __shfl_xor(s1[j], 32); s2[j] += __shfl_xor(s2[j], 32);
            if (h == 0) { red[0][wave][32 * j + r] = s1[j]; red[1][wave][32 * j + r] = s2[j]; }
        }
        __syncthreads();
        for (int n = tid; n < NT * 32; n += 64 * WAVES) {
            float a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) { a1 += red[0][w][n]; a2 += red[1][w][n]; }
            p.stats[((long long)blockIdx.x * 2 + 0) * p.N + n] = a1;
            p.stats[((long long)blockIdx.x * 2 + 1) * p.N + n] = a2;
        }
    }
}

// ---- the same layer followed by MaxPool2d(2,2) (inference path of the VGG trunks, nets/vgg.py:69-83) ----------------------------
// unit = 32 output pixels of a ROW PAIR (2 ip, 2 ip + 1): four input rows in the wave's LDS slice, both rows' accumulators in
// registers (2 x NT x 16), the window maximum of act((v + bias) * scale + shift) taken vertically in the accumulator layout and
// horizontally on the way out of the transpose tile - 16 pooled pixels x 32 channels leave per tile, the full-resolution map
// (4 GB at 15.7 M pixels x 64 channels) is neither written nor read back by a pooling pass.  Stride 1 only; same MFMA order as
// k_c4_conv, so the result is bit-identical to k_c4_conv followed by efgh_maxpool2.
constexpr int LW1 = TP + 2;
__device__ __forceinline__ float4 load_px4(const C4Args &p, int idx, int ip, long long b, int j0) {
    const int kh = idx / LW1, x = idx - kh * LW1;
    const int yin = 2 * ip - 1 + kh, xin = j0 - 1 + x;
    if (kh < 4 && (unsigned)yin < (unsigned)p.Hin && (unsigned)xin < (unsigned)p.Win)
        return *reinterpret_cast<const float4 *>(p.A + ((b * p.Hin + yin) * p.Win + xin) * p.lda);
    return make_float4(0.f, 0.f, 0.f, 0.f);
}

// ReLU as the training path's pooling pass writes it (k_maxpool2_affine's act_f), and the first maximum in scan order of a window's
// four activated values under a strict `>` (pool_cell_dpre, k_pool_bn_bwd_reduce_y)
__device__ __forceinline__ float relu_sel(float t) { return t > 0.f ? t : 0.f; }
__device__ __forceinline__ int first_max4(const float e[4]) {
    int best = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) if (e[k] > e[best]) best = k;
    return best;
}

// TRAIN = true: the forward of a train-mode BatchNorm + ReLU layer (efgh_c4_conv3x3_pooled_train), after the statistics-only pass
// has given scale / shift.  The pooled value is that of k_c4_conv followed by k_maxpool2_affine, bit for bit: the affine map is ONE
// fused multiply-add there (the library is built with the compiler's default contraction, and k_maxpool2_affine's `v*scale + shift`
// compiles to v_fma_f32), so it is written as fmaf here, and the ReLU is act_f's select.  For the channels whose BatchNorm backward
// takes xhat from raw (pooled_xhat_from_raw) the raw value of the window's first maximum goes to raw_win [B][Ho/2][Wo/2][N]; the
// other channels store nothing there.
template <int NT, bool TRAIN = false>
__global__ void __launch_bounds__(64 * WAVES, 2) k_c4_conv_pool(const C4Args p) {
    __shared__ float2 Pw[WAVES][4][2][LW1 + 1];
    constexpr int TPITCH = 40;
    __shared__ __attribute__((aligned(16))) float Tw[WAVES][32 * TPITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    float2 (*P)[2][LW1 + 1] = Pw[wave];
    float *T = Tw[wave];
    const int Hp = p.Ho >> 1, Wp = p.Wo >> 1;

    float2 bw[9][NT];
    float bi[NT], sc[NT], sf[NT];
    bool win[NT];                                    // TRAIN: this lane's channel of tile j leaves raw_win
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = 32 * j + r;
#pragma unroll
        for (int t = 0; t < 9; ++t) bw[t][j] = *reinterpret_cast<const float2 *>(p.W + ((long long)n * 9 + t) * 4 + 2 * h);
        bi[j] = p.bias ? p.bias[n] : 0.f;
        sc[j] = p.scale ? p.scale[n] : 1.f;
        sf[j] = p.shift ? p.shift[n] : 0.f;
        win[j] = TRAIN && pooled_xhat_from_raw(p.mean[n], p.invstd[n], sc[j], sf[j]);
    }
    const float neg = p.act == 1 ? 0.f : (p.act == 2 ? p.slope : 1.f);
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t) asm volatile("" ::"v"(bw[t][j].x), "v"(bw[t][j].y));

    const long long nwaves = (long long)gridDim.x * WAVES;
    long long unit = (long long)blockIdx.x * WAVES + wave;
    long long rowp = 0, b = 0; int ip = 0, j0 = 0;   // coordinates of the unit whose pixels are in pf0..2 (rowp = b * Hp + ip)
    long long crow = 0; int cj0 = 0;                 // ... of the unit staged in LDS
    float4 pf0, pf1, pf2;                            // 4 x 34 staged pixels = 136 <= 192
#define EFGH_FETCH(u)                                                                    \
    {                                                                                   \
        const int jb = (int)((u) % p.jblocks);                                          \
        rowp = (u) / p.jblocks; ip = (int)(rowp % Hp); b = rowp / Hp; j0 = jb * TP;     \
        pf0 = load_px4(p, lane, ip, b, j0); pf1 = load_px4(p, lane + 64, ip, b, j0);    \
        pf2 = load_px4(p, lane + 128, ip, b, j0);                                       \
    }
#define EFGH_PUT(q, v)                                                                   \
    {                                                                                   \
        const int idx = lane + 64 * q;                                                  \
        if (idx < 4 * LW1) {                                                            \
            const int kh = idx / LW1, x = idx - kh * LW1;                               \
            P[kh][0][x] = make_float2(v.x, v.y); P[kh][1][x] = make_float2(v.z, v.w);   \
        }                                                                               \
    }
#define EFGH_STAGE()                                                                     \
    {                                                                                   \
        crow = rowp; cj0 = j0;                                                          \
        EFGH_PUT(0, pf0) EFGH_PUT(1, pf1) EFGH_PUT(2, pf2)                              \
    }
    if (unit < p.units) {
        EFGH_FETCH(unit)
        EFGH_STAGE()
        if (unit + nwaves < p.units) EFGH_FETCH(unit + nwaves)
    }
    for (; unit < p.units; unit += nwaves) {
        const long long orow0 = crow; const int oj0 = cj0;
        wave_lds_sync();
        f32x16 acc[2][NT];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[half][j][q] = 0.f;
            float2 af[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) af[t] = P[t / 3 + half][h][r + t % 3];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    acc[half][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[t].x, bw[t][j].x, acc[half][j], 0, 0, 0);
                    acc[half][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[t].y, bw[t][j].y, acc[half][j], 0, 0, 0);
                }
            }
        }
        wave_lds_sync();
        if (unit + nwaves < p.units) {
            EFGH_STAGE()
            if (unit + 2 * nwaves < p.units) EFGH_FETCH(unit + 2 * nwaves)
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            wave_lds_sync();                         // the tile's previous readers are done
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int pl = (q & 3) + 8 * (q >> 2) + 4 * h;
                const float t0 = fmaf(acc[0][j][q] + bi[j], sc[j], sf[j]), t1 = fmaf(acc[1][j][q] + bi[j], sc[j], sf[j]);
                const float v0 = TRAIN ? relu_sel(t0) : act_neg(t0, neg);
                const float v1 = TRAIN ? relu_sel(t1) : act_neg(t1, neg);
                T[pl * TPITCH + r] = fmaxf(v0, v1);
            }
            if (TRAIN && win[j]) {
                // a window's four values sit in ONE lane: accumulator elements q, q + 1 (q even) are the pixels pl, pl + 1 of both rows
#pragma unroll
                for (int q = 0; q < 16; q += 2) {
                    const int pp = ((q & 3) >> 1) + 4 * (q >> 2) + 2 * h;
                    const float rw[4] = {acc[0][j][q] + bi[j], acc[0][j][q + 1] + bi[j], acc[1][j][q] + bi[j], acc[1][j][q + 1] + bi[j]};
                    float e[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) e[k] = relu_sel(fmaf(rw[k], sc[j], sf[j]));
                    const int best = first_max4(e);
                    if ((oj0 >> 1) + pp < Wp)
                        p.raw_win[(orow0 * Wp + (oj0 >> 1) + pp) * (long long)p.N + 32 * j + r] =
                            best == 0 ? rw[0] : (best == 1 ? rw[1] : (best == 2 ? rw[2] : rw[3]));
                }
            }
            wave_lds_sync();
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const int item = 64 * pass + lane, pp = item >> 3, c4 = (item & 7) * 4;
                const float4 a = *reinterpret_cast<const float4 *>(&T[(2 * pp) * TPITCH + c4]);
                const float4 c = *reinterpret_cast<const float4 *>(&T[(2 * pp + 1) * TPITCH + c4]);
                float4 v;
                v.x = fmaxf(a.x, c.x); v.y = fmaxf(a.y, c.y); v.z = fmaxf(a.z, c.z); v.w = fmaxf(a.w, c.w);
                if ((oj0 >> 1) + pp < Wp)
                    *reinterpret_cast<float4 *>(p.out + (orow0 * Wp + (oj0 >> 1) + pp) * p.ldo + 32 * j + c4) = v;
            }
        }
    }
#undef EFGH_FETCH
#undef EFGH_PUT
#undef EFGH_STAGE
}

// ---- BatchNorm backward "apply" of the train-mode pooled layer, raw RECOMPUTED (efgh_c4_pool_bwd_draw) ---------------------------
// What k_pool_bn_bwd_apply (backward.hip) makes of the stored raw map, from the layer's input instead: the row-pair unit of
// k_c4_conv_pool (a last pair of an odd map has one row), raw = acc + bias in the same MFMA order, and then per 2x2 cell - whose four
// values sit in one lane, see k_c4_conv_pool - pool_cell_dpre's rule for a ReLU: the pooled gradient times act' goes to the first
// maximum of relu(raw*pscale + pshift), every other element and every cell of an odd last row / column has dpre = 0; draw =
// bn_draw_f64.  The full-resolution draw leaves through the transpose tile as 16-byte stores, one image row at a time.  No atomics.
template <int NT, bool NTS>
__global__ void __launch_bounds__(64 * WAVES, 2) k_c4_pool_bwd_draw(const C4Args p) {
    __shared__ float2 Pw[WAVES][4][2][LW1 + 1];
    constexpr int TPITCH = 40;
    __shared__ __attribute__((aligned(16))) float Tw[WAVES][32 * TPITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    float2 (*P)[2][LW1 + 1] = Pw[wave];
    float *T = Tw[wave];
    const int Hp = p.Ho >> 1, Wp = p.Wo >> 1, Hc = (p.Ho + 1) >> 1;

    float2 bw[9][NT];
    float bi[NT], sc[NT], sf[NT];
    double mu[NT], is[NT], cf[NT], m1[NT], m2[NT], zm1[NT];      // (zm1: dpre - m1 of an element that is no winner)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = 32 * j + r;
#pragma unroll
        for (int t = 0; t < 9; ++t) bw[t][j] = *reinterpret_cast<const float2 *>(p.W + ((long long)n * 9 + t) * 4 + 2 * h);
        bi[j] = p.bias ? p.bias[n] : 0.f;
        sc[j] = p.scale[n]; sf[j] = p.shift[n];
        mu[j] = (double)p.mean[n]; is[j] = (double)p.invstd[n]; cf[j] = (double)p.coef[n];
        m1[j] = p.m1[n]; m2[j] = p.m2[n];
        zm1[j] = bn_draw_dpre_m1(0.f, m1[j]);
    }
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t) asm volatile("" ::"v"(bw[t][j].x), "v"(bw[t][j].y));

    const long long nwaves = (long long)gridDim.x * WAVES;
    long long unit = (long long)blockIdx.x * WAVES + wave;
    long long rowc = 0, b = 0; int ip = 0, j0 = 0;   // coordinates of the unit whose pixels are in pf0..2 (rowc = b * Hc + ip)
    long long crow = 0; int cj0 = 0;                 // ... of the unit staged in LDS
    float4 pf0, pf1, pf2;
#define EFGH_FETCH(u)                                                                    \
    {                                                                                   \
        const int jb = (int)((u) % p.jblocks);                                          \
        rowc = (u) / p.jblocks; ip = (int)(rowc % Hc); b = rowc / Hc; j0 = jb * TP;     \
        pf0 = load_px4(p, lane, ip, b, j0); pf1 = load_px4(p, lane + 64, ip, b, j0);    \
        pf2 = load_px4(p, lane + 128, ip, b, j0);                                       \
    }
#define EFGH_PUT(q, v)                                                                   \
    {                                                                                   \
        const int idx = lane + 64 * q;                                                  \
        if (idx < 4 * LW1) {                                                            \
            const int kh = idx / LW1, x = idx - kh * LW1;                               \
            P[kh][0][x] = make_float2(v.x, v.y); P[kh][1][x] = make_float2(v.z, v.w);   \
        }                                                                               \
    }
#define EFGH_STAGE()                                                                     \
    {                                                                                   \
        crow = rowc; cj0 = j0;                                                          \
        EFGH_PUT(0, pf0) EFGH_PUT(1, pf1) EFGH_PUT(2, pf2)                              \
    }
    if (unit < p.units) {
        EFGH_FETCH(unit)
        EFGH_STAGE()
        if (unit + nwaves < p.units) EFGH_FETCH(unit + nwaves)
    }
    for (; unit < p.units; unit += nwaves) {
        const int oj0 = cj0, oip = (int)(crow % Hc);
        const long long ob = crow / Hc;
        const bool row1 = 2 * oip + 1 < p.Ho;        // (wave-uniform) the pair's second row exists
        // the pooled gradient of this lane's eight cells, per channel tile: in flight during the MFMAs
        float g[NT][8];
#pragma unroll
        for (int q = 0; q < 16; q += 2) {
            const int pc = (oj0 >> 1) + ((q & 3) >> 1) + 4 * (q >> 2) + 2 * h;
            const bool pooled = oip < Hp && pc < Wp;
#pragma unroll
            for (int j = 0; j < NT; ++j)
                g[j][q >> 1] = pooled ? p.dyp[((ob * Hp + oip) * Wp + pc) * (long long)p.N + 32 * j + r] : 0.f;
        }
        wave_lds_sync();
        f32x16 acc[2][NT];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[half][j][q] = 0.f;
            float2 af[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) af[t] = P[t / 3 + half][h][r + t % 3];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    acc[half][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[t].x, bw[t][j].x, acc[half][j], 0, 0, 0);
                    acc[half][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[t].y, bw[t][j].y, acc[half][j], 0, 0, 0);
                }
            }
        }
        wave_lds_sync();
        if (unit + nwaves < p.units) {
            EFGH_STAGE()
            if (unit + 2 * nwaves < p.units) EFGH_FETCH(unit + 2 * nwaves)
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            // acc[half][j][q] <- draw of (row 2 oip + half, pixel pl(q)), cell by cell
#pragma unroll
            for (int q = 0; q < 16; q += 2) {
                const int pc = (oj0 >> 1) + ((q & 3) >> 1) + 4 * (q >> 2) + 2 * h;
                const bool pooled = oip < Hp && pc < Wp;
                const float rw[4] = {acc[0][j][q] + bi[j], acc[0][j][q + 1] + bi[j], acc[1][j][q] + bi[j], acc[1][j][q + 1] + bi[j]};
                float e[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) e[k] = relu_sel(fmaf(rw[k], sc[j], sf[j]));
                const int best = first_max4(e);
                // ReLU: act' at the winner is 1 where its activated value - the window's maximum - is positive, else 0
                const float emax = fmaxf(fmaxf(e[0], e[1]), fmaxf(e[2], e[3]));
                const float dwin = pooled ? g[j][q >> 1] * (emax > 0.f ? 1.f : 0.f) : 0.f;
                const double twin = bn_draw_dpre_m1(dwin, m1[j]);
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = bn_draw_f64(rw[k], k == best ? twin : zm1[j], mu[j], is[j], cf[j], m2[j]);
                acc[0][j][q] = o[0]; acc[0][j][q + 1] = o[1]; acc[1][j][q] = o[2]; acc[1][j][q + 1] = o[3];
            }
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                if (half == 1 && !row1) break;
                wave_lds_sync();                     // the tile's previous readers are done
#pragma unroll
                for (int q = 0; q < 16; ++q) T[((q & 3) + 8 * (q >> 2) + 4 * h) * TPITCH + r] = acc[half][j][q];
                wave_lds_sync();
                float *drow = p.draw + (((ob * p.Ho + 2 * oip + half) * p.Wo) + oj0) * (long long)p.N + 32 * j;
#pragma unroll
                for (int pass = 0; pass < 4; ++pass) {
                    const int pl = 8 * pass + (lane >> 3), c4 = (lane & 7) * 4;
                    const float4 v = *reinterpret_cast<const float4 *>(&T[pl * TPITCH + c4]);
                    if (oj0 + pl < p.Wo) st_stream<NTS>(drow + (long long)pl * p.N + c4, v);
                }
            }
        }
    }
#undef EFGH_FETCH
#undef EFGH_PUT
#undef EFGH_STAGE
}

// ---- weight gradient ---------------------------------------------------------------------------------------------
// unit = 32 output (= gradient) pixels of one image row, taken by one wave in 8 groups of 4 (the k of
// v_mfma_f32_16x16x4_f32).  A operand: G[pixel k][n] (16 outputs of an n-tile), B operand: X[pixel k + tap][c] for column
// (t, c) = 16 qt + lane&15 (columns >= 36 are zero).
template <int NT16>
__global__ void __launch_bounds__(64 * WAVES) k_c4_wgrad(const C4Args p) {
    __shared__ float4 Xw[WAVES][3][LWMAX + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q16 = lane & 15, k4 = lane >> 4;
    const int LW = (TP - 1) * p.s + 3;
    float4 (*X)[LWMAX + 1] = Xw[wave];
    f32x4 acc[NT16][3];
#pragma unroll
    for (int a = 0; a < NT16; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[a][c][e] = 0.f;
    // LDS float offset of this lane's column in each column tile, relative to the group's first pixel
    int coff[3]; bool cok[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int col = 16 * c + q16, t = col >> 2, ch = col & 3;
        cok[c] = col < 36;
        coff[c] = cok[c] ? ((t / 3) * (LWMAX + 1) + t % 3) * 4 + ch : 0;
    }
    const float *Xf = reinterpret_cast<const float *>(&X[0][0]);

    const long long nwaves = (long long)gridDim.x * WAVES;
    long long unit = (long long)blockIdx.x * WAVES + wave;
    long long row = 0, b = 0; int i = 0, j0 = 0;
    float4 pf0, pf1, pf2, pf3;
    float ga[8][NT16], gn[8][NT16];                  // G of the current / next unit (all 8 groups in flight at once)
#define EFGH_FETCH(u)                                                                    \
    {                                                                                   \
        unit_coords(p, u, row, i, b, j0);                                               \
        pf0 = load_px(p, lane, LW, i, b, j0); pf1 = load_px(p, lane + 64, LW, i, b, j0); \
        pf2 = load_px(p, lane + 128, LW, i, b, j0); pf3 = load_px(p, lane + 192, LW, i, b, j0); \
        const float *grow = p.G + (row * p.Wo + j0) * p.ldg + q16;                       \
        _Pragma("unroll") for (int g = 0; g < 8; ++g) {                                 \
            const int pl = 4 * g + k4;                                                  \
            const bool ok = j0 + pl < p.Wo;                                             \
            _Pragma("unroll") for (int a = 0; a < NT16; ++a) gn[g][a] = ok ? grow[(long long)pl * p.ldg + 16 * a] : 0.f; \
        }                                                                               \
    }
#define EFGH_PUT(q, v)                                                                   \
    {                                                                                   \
        const int idx = lane + 64 * q;                                                  \
        if (idx < 3 * LW) X[idx / LW][idx % LW] = v;                                     \
    }
    if (unit < p.units) EFGH_FETCH(unit)
    for (; unit < p.units; unit += nwaves) {
        wave_lds_sync();                             // the previous unit's operand reads are done
        EFGH_PUT(0, pf0) EFGH_PUT(1, pf1) EFGH_PUT(2, pf2) EFGH_PUT(3, pf3)
#pragma unroll
        for (int g = 0; g < 8; ++g)
#pragma unroll
            for (int a = 0; a < NT16; ++a) ga[g][a] = gn[g][a];
        wave_lds_sync();
        if (unit + nwaves < p.units) EFGH_FETCH(unit + nwaves)        // in flight during the MFMAs below
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const int pl = 4 * g + k4;                               // this lane's pixel of the group
            float xb[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) xb[c] = cok[c] ? Xf[coff[c] + pl * p.s * 4] : 0.f;
#pragma unroll
            for (int a = 0; a < NT16; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[g][a], xb[c], acc[a][c], 0, 0, 0);
        }
    }
#undef EFGH_FETCH
#undef EFGH_PUT
    // acc[a][c][e]: n = 16a + 4*(lane>>4) + e, column = 16c + (lane&15).  Every wave leaves its own partial [N][36] plane (a
    // wave without units leaves zeros); efgh_c4_wgrad folds the planes in wave order: no atomics, bit-reproducible run to run
    float *plane = p.dW + ((long long)blockIdx.x * WAVES + wave) * (16 * NT16 * 36);
#pragma unroll
    for (int a = 0; a < NT16; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (!cok[c]) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                plane[(16 * a + 4 * k4 + e) * 36 + 16 * c + q16] = acc[a][c][e];
        }
}

bool c4_geometry_ok(const efgh_gemm_desc *d) {
    if (!d || d->mode != 1 || d->C != 4 || d->T != 9 || d->M_dev || d->nbatch > 1) return false;
    if (d->sh != d->sw || (d->sh != 1 && d->sh != 2) || d->osh != 1 || d->osw != 1 || d->oh0 || d->ow0) return false;
    if (d->Hv != d->Ho || d->Wv != d->Wo || d->B <= 0 || d->M != (int64_t)d->B * d->Ho * d->Wo) return false;
    for (int t = 0; t < 9; ++t) if (d->dh[t] != t / 3 - 1 || d->dw[t] != t % 3 - 1) return false;
    // every input pixel a valid output touches must exist or be padding: s*(Ho-1) - 1 + 2 <= Hin is NOT required (out-of-image
    // taps read zeros), but the LDS row must cover them: guaranteed by LW = (TP-1)*s + 3
    if (d->residual && (d->ldr % 4 != 0 || (((uintptr_t)d->residual) & 15) != 0)) return false;      // 16-byte residual reads
    return d->lda % 4 == 0 && (((uintptr_t)d->A) & 15) == 0;
}

void fill(C4Args &a, const efgh_gemm_desc *d) {
    a.A = d->A; a.lda = d->lda; a.B = d->B; a.Hin = d->Hin; a.Win = d->Win; a.Ho = d->Ho; a.Wo = d->Wo; a.s = d->sh;
    a.W = d->W; a.N = d->N; a.bias = d->bias; a.scale = d->scale; a.shift = d->shift; a.residual = d->residual; a.ldr = d->ldr; a.act = d->act; a.slope = d->slope;
    a.out = d->out; a.ldo = d->ldo; a.stats = d->stats;
    a.jblocks = (d->Wo + TP - 1) / TP;
    a.units = (long long)d->B * d->Ho * a.jblocks;
    a.G = nullptr; a.ldg = 0; a.dW = nullptr;
    a.mean = a.invstd = a.coef = a.dyp = nullptr; a.m1 = a.m2 = nullptr; a.raw_win = a.draw = nullptr;
}

int grid_of(long long units) {                     // persistent: 3 workgroups of 4 waves per CU
    const long long g = (units + WAVES - 1) / WAVES;
    return (int)(g < 768 ? g : 768);
}

}  // namespace

extern "C" int efgh_c4_supported(const efgh_gemm_desc *d) {
    return (c4_geometry_ok(d) && (d->N == 32 || d->N == 64 || d->N == 128)) ? 1 : 0;
}

extern "C" int32_t efgh_c4_stats_rows(int32_t B, int32_t Ho, int32_t Wo) {
    return grid_of((long long)B * Ho * ((Wo + TP - 1) / TP));
}

extern "C" int efgh_c4_conv3x3(const efgh_gemm_desc *d, void *stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EFGH_CHECK_ARG(efgh_c4_supported(d) && d->W && d->out && (((uintptr_t)d->W) & 7) == 0);
    EFGH_CHECK_ARG(d->ldo % 4 == 0 && (((uintptr_t)d->out) & 15) == 0);           // 16-byte output stores
    C4Args a;
    fill(a, d);
    const int grid = grid_of(a.units);
    const bool res = d->residual != nullptr;
#define EFGH_GO(NT)                                                                  \
    {                                                                               \
        if (res) k_c4_conv<NT, true><<<grid, 64 * WAVES, 0, st>>>(a);               \
        else k_c4_conv<NT, false><<<grid, 64 * WAVES, 0, st>>>(a);                  \
    }
    if (d->N == 32) EFGH_GO(1) else if (d->N == 64) EFGH_GO(2) else EFGH_GO(4)
#undef EFGH_GO
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_c4_pooled_supported(const efgh_gemm_desc *d) {
    return (efgh_c4_supported(d) && d->sh == 1 && !d->residual && !d->stats && d->Ho >= 2 && d->Wo >= 2) ? 1 : 0;
}

extern "C" int efgh_c4_conv3x3_pooled(const efgh_gemm_desc *d, void *stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EFGH_CHECK_ARG(efgh_c4_pooled_supported(d) && d->W && d->out && (((uintptr_t)d->W) & 7) == 0);
    EFGH_CHECK_ARG(d->ldo % 4 == 0 && (((uintptr_t)d->out) & 15) == 0);
    C4Args a;
    fill(a, d);
    a.units = (long long)d->B * (d->Ho / 2) * a.jblocks;          // row pairs x 32-pixel blocks
    const int grid = grid_of(a.units);
    if (d->N == 32) k_c4_conv_pool<1><<<grid, 64 * WAVES, 0, st>>>(a);
    else if (d->N == 64) k_c4_conv_pool<2><<<grid, 64 * WAVES, 0, st>>>(a);
    else k_c4_conv_pool<4><<<grid, 64 * WAVES, 0, st>>>(a);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

// ---- the train-mode pooled layer without its full-resolution map: statistics pass, pooled forward, recomputing apply ----
extern "C" int efgh_c4_conv3x3_stats(const efgh_gemm_desc *d, void *stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EFGH_CHECK_ARG(efgh_c4_supported(d) && d->W && d->stats && !d->residual && (((uintptr_t)d->W) & 7) == 0);
    C4Args a;
    fill(a, d);
    a.out = nullptr;
    const int grid = grid_of(a.units);               // the grid of efgh_c4_conv3x3: one statistics row per workgroup
    if (d->N == 32) k_c4_conv<1, false, false><<<grid, 64 * WAVES, 0, st>>>(a);
    else if (d->N == 64) k_c4_conv<2, false, false><<<grid, 64 * WAVES, 0, st>>>(a);
    else k_c4_conv<4, false, false><<<grid, 64 * WAVES, 0, st>>>(a);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_c4_conv3x3_pooled_train(const efgh_gemm_desc *d, const float *mean, const float *invstd, float *raw_win,
                                            void *stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EFGH_CHECK_ARG(efgh_c4_pooled_supported(d) && d->W && d->out && (((uintptr_t)d->W) & 7) == 0);
    EFGH_CHECK_ARG(d->ldo % 4 == 0 && (((uintptr_t)d->out) & 15) == 0);
    EFGH_CHECK_ARG(d->act == 1 && d->scale && d->shift && mean && invstd && raw_win);
    C4Args a;
    fill(a, d);
    a.units = (long long)d->B * (d->Ho / 2) * a.jblocks;
    a.mean = mean; a.invstd = invstd; a.raw_win = raw_win;
    const int grid = grid_of(a.units);
    if (d->N == 32) k_c4_conv_pool<1, true><<<grid, 64 * WAVES, 0, st>>>(a);
    else if (d->N == 64) k_c4_conv_pool<2, true><<<grid, 64 * WAVES, 0, st>>>(a);
    else k_c4_conv_pool<4, true><<<grid, 64 * WAVES, 0, st>>>(a);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_c4_pool_bwd_draw(const efgh_gemm_desc *d, const float *dy_pool, const float *mean, const float *invstd,
                                     const float *coef, const double *m1, const double *m2, float *draw, void *stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EFGH_CHECK_ARG(efgh_c4_pooled_supported(d) && d->W && (((uintptr_t)d->W) & 7) == 0 && d->scale && d->shift);
    EFGH_CHECK_ARG(d->act == 1 && dy_pool && mean && invstd && coef && m1 && m2 && draw && (((uintptr_t)draw) & 15) == 0);
    C4Args a;
    fill(a, d);
    a.out = nullptr;
    a.units = (long long)d->B * ((d->Ho + 1) / 2) * a.jblocks;     // row pairs (the last one of an odd map has one row) x 32-pixel blocks
    a.mean = mean; a.invstd = invstd; a.coef = coef; a.m1 = m1; a.m2 = m2; a.dyp = dy_pool; a.draw = draw;
    const int grid = grid_of(a.units);
    const bool nt = efgh_stream_nt((long long)d->M * d->N * 4);
#define EFGH_GO(NT)                                                                  \
    {                                                                               \
        if (nt) k_c4_pool_bwd_draw<NT, true><<<grid, 64 * WAVES, 0, st>>>(a);       \
        else k_c4_pool_bwd_draw<NT, false><<<grid, 64 * WAVES, 0, st>>>(a);         \
    }
    if (d->N == 32) EFGH_GO(1) else if (d->N == 64) EFGH_GO(2) else EFGH_GO(4)
#undef EFGH_GO
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_c4_wgrad_supported(const efgh_gemm_desc *d) {
    return (c4_geometry_ok(d) && d->N % 16 == 0 && d->N >= 32 && d->N <= 128) ? 1 : 0;
}

/* floats of scratch efgh_c4_wgrad needs: one partial [N][36] plane per wave of the launch */
extern "C" int64_t efgh_c4_wgrad_workspace(const efgh_gemm_desc *d) {
    if (!efgh_c4_wgrad_supported(d)) return 0;
    C4Args a;
    fill(a, d);
    return (int64_t)grid_of(a.units) * WAVES * d->N * 36;
}

extern "C" int efgh_c4_wgrad(const efgh_gemm_desc *d, const float *G, int64_t ldg, float *dWp, float *workspace,
                             const efgh_wgrad_out_desc *out, void *stream_) {
    hipStream_t st = (hipStream_t)stream_;
    EFGH_CHECK_ARG(efgh_c4_wgrad_supported(d) && G && dWp && ldg >= d->N);
    EFGH_CHECK_ARG(workspace && (((uintptr_t)workspace) & 15) == 0 && (((uintptr_t)dWp) & 15) == 0);
    C4Args a;
    fill(a, d);
    a.G = G; a.ldg = ldg; a.dW = workspace;
    const int grid = grid_of(a.units);
    switch (d->N / 16) {
    case 2: k_c4_wgrad<2><<<grid, 256, 0, st>>>(a); break;
    case 3: k_c4_wgrad<3><<<grid, 256, 0, st>>>(a); break;
    case 4: k_c4_wgrad<4><<<grid, 256, 0, st>>>(a); break;
    case 5: k_c4_wgrad<5><<<grid, 256, 0, st>>>(a); break;
    case 6: k_c4_wgrad<6><<<grid, 256, 0, st>>>(a); break;
    case 7: k_c4_wgrad<7><<<grid, 256, 0, st>>>(a); break;
    default: k_c4_wgrad<8><<<grid, 256, 0, st>>>(a); break;
    }
    const bool wrote = efgh_launch_fold_splits(workspace, grid * WAVES, (long long)d->N * 36, dWp, st, out);
    EFGH_CHECK_LAUNCH();
    return wrote ? EFGH_WROTE_OUT : EFGH_OK;
}
