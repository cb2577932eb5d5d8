// The differentiable form of score.hip's mutual information ("Refining a pose"): a Parzen-smoothed joint histogram whose MI
// has an analytic gradient with respect to the projection matrix (Mattes' formulation of Pandey et al.'s objective).  The grey level
// is sampled BILINEARLY at (u - 0.5, v - 0.5) and spread linearly over two neighbouring grey cells with integer weights of
// resolution FRAC = 256, so the histogram stays an integer one and goes through the UNCHANGED k_score_mi.  Four kernels:
//   k_soft_hist    grid (point chunk, k, b), k_score_hist's shape: LDS counters, integer flush; pooled, the samples share one histogram
//   k_soft_table   one workgroup per histogram: column sums in integers, Tt[x][y] = log h_xy - log h_y (0 where h_xy = 0), a flag per
//                  cell for h_xy > 0, and the histogram's total
//   k_soft_grad    grid (point chunk, k, b): per point a = s ok (Tt[x][j+1] - Tt[x][j]) (bins / 256) / n, and its twelve contributions
//                  to dMI/dP; twelve float64 accumulators a thread in index order, a fixed pairwise tree of plain LDS stores over the
//                  block, one partial per chunk with plain stores
//   k_soft_fold    one workgroup per (b, k): the chunks' partials through the same fixed tree
// Float64 throughout with every operation rounded on its own (-ffp-contract=off; tests/score_soft_contract.py restates it in numpy).
// No floating-point atomic: two runs give the same bits.  The gradient is that of the unquantised function at fixed membership: it
// ignores points that enter or leave the frame and is zero where the grey coordinate is clamped.  k_soft_hist and k_soft_grad have
// ONE body and two instances each: the MASKED one (efgh_score_soft_hist_masked, efgh_score_soft_grad_masked) also wants the point's bit
// in score_vis.hip's per-candidate visibility mask, so histogram and gradient share their membership by construction.
#include "score_common.h"

namespace {
constexpr int FRAC = 256;                                        // weight resolution: a point adds FRAC to the histogram
static_assert((long long)EFGH_SCORE_CHUNK * FRAC < (1LL << 32), "a chunk of points, FRAC each, fits the 32-bit LDS counter");
constexpr int MAX_FOLD = 2048;                                   // chunks of one (b, k), padded to a power of two, that k_soft_fold holds in LDS

struct Sample {
    int x, j, q, s;                                              // value bin, lower grey cell, weight of cell j + 1 in 1/FRAC, gate
    double gu, gv, u, v;                                         // the grey level's slope in u and v at the sample; the pixel coordinates
};

// one point under one candidate -> does it count, and where.  The counting rule and the value bin are k_score_hist's
__device__ __forceinline__ bool sample(const float *__restrict__ pcb, long long cs, int i, float val, const double *__restrict__ T,
                                       const uint8_t *__restrict__ imgb, int H, int W, int bins, float lo, float scale, double min_depth,
                                       Sample &o) {
    if (!(val == val)) return false;                             // a NaN value drops the point
    const Hit h = project(pcb, cs, i, T, H, W, min_depth);
    if (h.state != ST_OCCLUDED) return false;                    // in frame; nothing here asks whether it is hidden
    const float top = (float)(bins - 1);
    const float tv = (val - lo) * scale;                         // two float32 operations
    o.x = tv >= top ? bins - 1 : (tv > 0.f ? (int)tv : 0);
    // fuse.hip's bilinear convention on the integer L
    const double fx = h.u - 0.5, fy = h.v - 0.5;
    const double x0 = floor(fx), y0 = floor(fy);
    const double tx = fx - x0, ty = fy - y0;
    const int xi = (int)x0, yi = (int)y0;
    const int xa = min(max(xi, 0), W - 1), xb = min(max(xi + 1, 0), W - 1);
    const int ya = min(max(yi, 0), H - 1), yb = min(max(yi + 1, 0), H - 1);
    const double a = (double)luma(imgb + ((long long)ya * W + xa) * 3), b = (double)luma(imgb + ((long long)ya * W + xb) * 3);
    const double c = (double)luma(imgb + ((long long)yb * W + xa) * 3), d = (double)luma(imgb + ((long long)yb * W + xb) * 3);
    const double ba = b - a, dc = d - c;
    const double tp = a + ba * tx, bt = c + dc * tx;
    const double g = tp + (bt - tp) * ty;
    o.gu = ba + (dc - ba) * ty;
    o.gv = bt - tp;
    o.u = h.u; o.v = h.v;
    const double t = g * ((double)bins / 256.0) - 0.5;           // the factor is a power of two: the product is exact
    const double fl = floor(t);
    const int j = fl < 0.0 ? 0 : (fl > (double)(bins - 2) ? bins - 2 : (int)fl);      // (g lies in 0 .. 255: t is finite)
    const double r = t - (double)j;
    o.j = j;
    o.s = (r > 0.0 && r < 1.0) ? 1 : 0;
    const double fr = r < 0.0 ? 0.0 : (r > 1.0 ? 1.0 : r);
    o.q = (int)(fr * (double)FRAC + 0.5);
    return true;
}

template <bool MASKED>
__global__ void __launch_bounds__(TPB)
k_soft_hist(const float *__restrict__ pc, long long bs, long long cs, int N, const float *__restrict__ value, long long vbs,
            const double *__restrict__ P, int K, const uint8_t *__restrict__ img, int H, int W, int bins, float lo, float scale,
            double min_depth, int pool, const unsigned *__restrict__ mask, unsigned *__restrict__ hist) {
    __shared__ unsigned cnt[MAX_BINS * MAX_BINS];
    const int k = blockIdx.y, b = blockIdx.z, nb = bins * bins;
    for (int c = threadIdx.x; c < nb; c += TPB) cnt[c] = 0u;
    __syncthreads();
    const float *__restrict__ pcb = pc + b * bs;
    const float *__restrict__ vb = value + b * vbs;
    const double *__restrict__ T = P + 12 * ((long long)b * K + k);
    const uint8_t *__restrict__ imgb = img + (long long)b * H * W * 3;
    const unsigned *__restrict__ mk = MASKED ? mask + ((long long)b * K + k) * mask_words(N) : nullptr;
    const int first = blockIdx.x * EFGH_SCORE_CHUNK;        // (N < 2^23: no index here comes near 2^31)
    const int end = min(first + EFGH_SCORE_CHUNK, N);
    for (int i = first + threadIdx.x; i < end; i += TPB) {
        Sample s;
        if (MASKED && !mask_bit(mk, i)) continue;                // hidden under this candidate
        if (!sample(pcb, cs, i, vb[i], T, imgb, H, W, bins, lo, scale, min_depth, s)) continue;
        unsigned *row = cnt + s.x * bins + s.j;                  // j <= bins - 2: cell j + 1 is in the row
        if (s.q != FRAC) atomicAdd(row, (unsigned)(FRAC - s.q));
        if (s.q) atomicAdd(row + 1, (unsigned)s.q);
    }
    __syncthreads();
    unsigned *__restrict__ out = hist + (pool ? (long long)k : (long long)b * K + k) * nb;
    for (int c = threadIdx.x; c < nb; c += TPB) {
        const unsigned n = cnt[c];
        if (n) atomicAdd(out + c, n);
    }
}

__global__ void __launch_bounds__(TPB)
k_soft_table(const unsigned *__restrict__ hist, int bins, double *__restrict__ table, uint8_t *__restrict__ flag,
             unsigned *__restrict__ total) {
    __shared__ unsigned col[MAX_BINS];
    __shared__ double lcol[MAX_BINS];
    const int nb = bins * bins;
    const unsigned *__restrict__ h = hist + (long long)blockIdx.x * nb;
    if (threadIdx.x < MAX_BINS) col[threadIdx.x] = 0u;
    __syncthreads();
    for (int c = threadIdx.x; c < nb; c += TPB) {
        const unsigned n = h[c];
        if (n) atomicAdd(&col[c % bins], n);
    }
    __syncthreads();
    if (threadIdx.x < bins) lcol[threadIdx.x] = col[threadIdx.x] ? log((double)col[threadIdx.x]) : 0.0;
    if (threadIdx.x == TPB - 1) {                                // the total from the column sums (a wave that takes no logarithm)
        unsigned tot = 0u;
        for (int y = 0; y < bins; ++y) tot += col[y];
        total[blockIdx.x] = tot;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < nb; c += TPB) {
        const unsigned n = h[c];
        table[(long long)blockIdx.x * nb + c] = n ? log((double)n) - lcol[c % bins] : 0.0;       // (n > 0: its column sum is too)
        flag[(long long)blockIdx.x * nb + c] = n ? 1 : 0;
    }
}

// red[c][0 .. TPB) for c < 12 summed in place in tree_sum's shape, all twelve at once: pairs a distance 128, 64, .. 1 apart
__device__ __forceinline__ void tree12(double (*red)[TPB]) {
    for (int s = TPB >> 1; s > 0; s >>= 1) {
        __syncthreads();
        for (int e = threadIdx.x; e < 12 * s; e += TPB) {
            const int c = e / s, i = e - c * s;
            red[c][i] = red[c][i] + red[c][i + s];
        }
    }
    __syncthreads();
}

template <bool MASKED>
__global__ void __launch_bounds__(TPB)
k_soft_grad(const float *__restrict__ pc, long long bs, long long cs, int N, const float *__restrict__ value, long long vbs,
            const double *__restrict__ P, int K, const uint8_t *__restrict__ img, int H, int W, int bins, float lo, float scale,
            double min_depth, int pool, const double *__restrict__ table, const uint8_t *__restrict__ flag,
            const unsigned *__restrict__ total, const unsigned *__restrict__ mask, double *__restrict__ part) {
    __shared__ double red[12][TPB];
    const int k = blockIdx.y, b = blockIdx.z, nb = bins * bins;
    const float *__restrict__ pcb = pc + b * bs;
    const float *__restrict__ vb = value + b * vbs;
    const double *__restrict__ T = P + 12 * ((long long)b * K + k);
    const uint8_t *__restrict__ imgb = img + (long long)b * H * W * 3;
    const unsigned *__restrict__ mk = MASKED ? mask + ((long long)b * K + k) * mask_words(N) : nullptr;
    const long long hi = pool ? (long long)k : (long long)b * K + k;
    const double *__restrict__ Tt = table + hi * nb;
    const uint8_t *__restrict__ fl = flag + hi * nb;
    const double n = (double)(total[hi] / (unsigned)FRAC);       // the points that counted
    const double gain = (double)bins / 256.0;
    double acc[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) acc[c] = 0.0;
    const int first = blockIdx.x * EFGH_SCORE_CHUNK;
    const int end = min(first + EFGH_SCORE_CHUNK, N);
    for (int i = first + threadIdx.x; i < end; i += TPB) {      // a thread's points in index order
        Sample s;
        if (MASKED && !mask_bit(mk, i)) continue;                // hidden under this candidate
        if (!sample(pcb, cs, i, vb[i], T, imgb, H, W, bins, lo, scale, min_depth, s)) continue;
        const int c0 = s.x * bins + s.j;
        if (!(s.s && fl[c0] && fl[c0 + 1])) continue;            // gate shut, or a cell that is empty: no contribution
        const double a = ((Tt[c0 + 1] - Tt[c0]) * gain) / n;     // (a counted point: n >= 1)
        const double px = (double)pcb[i], py = (double)pcb[cs + i], pz = (double)pcb[2 * cs + i];
        const double w = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];      // project()'s w, the same bits
        const double r0 = (a * s.gu) / w, r1 = (a * s.gv) / w;
        const double r2 = -((a * (s.gu * s.u + s.gv * s.v)) / w);
        acc[0] += r0 * px; acc[1] += r0 * py; acc[2] += r0 * pz; acc[3] += r0;
        acc[4] += r1 * px; acc[5] += r1 * py; acc[6] += r1 * pz; acc[7] += r1;
        acc[8] += r2 * px; acc[9] += r2 * py; acc[10] += r2 * pz; acc[11] += r2;
    }
#pragma unroll
    for (int c = 0; c < 12; ++c) red[c][threadIdx.x] = acc[c];
    tree12(red);
    if (threadIdx.x < 12) part[(((long long)b * K + k) * gridDim.x + blockIdx.x) * 12 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ void __launch_bounds__(TPB)
k_soft_fold(const double *__restrict__ part, int nchunk, int npow, double *__restrict__ grad) {
    __shared__ double t[MAX_FOLD];
    const double *__restrict__ p = part + (long long)blockIdx.x * nchunk * 12;
    for (int c = 0; c < 12; ++c) {
        for (int i = threadIdx.x; i < npow; i += TPB) t[i] = i < nchunk ? p[(long long)i * 12 + c] : 0.0;
        const double r = tree_sum(t, npow);
        if (threadIdx.x == 0) grad[(long long)blockIdx.x * 12 + c] = r;
    }
}

// the checks the histogram and the gradient launch share; *scale = (float)bins / (hi - lo), formed once in float32 as score.hip does
int check_points(const char *who, int B, int N, int K, int H, int W, int bins, float lo, float hi, double min_depth, int pool, float *scale) {
    SCORE_ARG(bins_ok(bins), "%s: bins = %d, supported are 8, 16, 32 and 64 (the counters live in LDS)", who, bins);
    SCORE_ARG(K > 0 && K <= MAX_K, "%s: K = %d candidates, supported are 1 .. %d", who, K, MAX_K);
    SCORE_ARG(B > 0 && B <= 65535, "%s: B = %d, supported are 1 .. 65535", who, B);
    SCORE_ARG(pool == 0 || pool == 1, "%s: pool = %d must be 0 or 1", who, pool);
    SCORE_ARG(N > 0 && (int64_t)N < (1LL << 23), "%s: N = %d must be positive and below 2^23 (a point adds 256 to a 32-bit histogram)", who, N);
    SCORE_ARG(!pool || (int64_t)B * N < (1LL << 23), "%s: B * N = %lld pooled points must stay below 2^23 (a point adds 256 to a 32-bit histogram)",
             who, (long long)B * N);
    SCORE_ARG(H > 0 && W > 0 && (int64_t)H * W < 0x7fffffffLL, "%s: H = %d, W = %d: both positive and H*W < 2^31", who, H, W);
    SCORE_ARG(min_depth >= 0.0 && std::isfinite(min_depth), "%s: min_depth = %g must be finite and >= 0", who, min_depth);
    SCORE_ARG(std::isfinite(lo) && std::isfinite(hi) && lo < hi, "%s: value range lo = %g, hi = %g: finite and lo < hi", who, (double)lo, (double)hi);
    const float width = hi - lo;
    *scale = (float)bins / width;
    SCORE_ARG(std::isfinite(width) && std::isfinite(*scale) && *scale > 0.f,
             "%s: value range lo = %g, hi = %g: bins / (hi - lo) is not a finite float32", who, (double)lo, (double)hi);
    return EFGH_OK;
}
}  // namespace

namespace {
int launch_soft_hist(const char *who, bool masked, const float *pc, int64_t pc_bstride, int64_t pc_cstride, int32_t B, int32_t N,
                     const float *value, int64_t value_bstride, const double *P, int32_t K, const uint8_t *img, int32_t H, int32_t W,
                     int32_t bins, float lo, float hi, double min_depth, int32_t pool, const uint32_t *mask, uint32_t *hist, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    SCORE_ARG(pc && value && P && img && hist, "%s: null pointer (pc %p, value %p, P %p, img %p, hist %p)", who, (const void *)pc,
             (const void *)value, (const void *)P, (const void *)img, (void *)hist);
    SCORE_ARG(!masked || mask, "%s: null pointer (mask %p)", who, (const void *)mask);
    float scale = 0.f;
    if (int rc = check_points(who, B, N, K, H, W, bins, lo, hi, min_depth, pool, &scale)) return rc;
    if (hipMemsetAsync(hist, 0, (size_t)4 * (pool ? 1 : B) * K * bins * bins, st) != hipSuccess) {
        efgh_set_error("%s: memset failed", who);
        return EFGH_E_LAUNCH;
    }
    const dim3 grid(cdiv(N, EFGH_SCORE_CHUNK), K, B);
    if (masked)
        k_soft_hist<true><<<grid, TPB, 0, st>>>(pc, pc_bstride, pc_cstride, N, value, value_bstride, P, K, img, H, W, bins, lo, scale,
                                                min_depth, pool, mask, hist);
    else
        k_soft_hist<false><<<grid, TPB, 0, st>>>(pc, pc_bstride, pc_cstride, N, value, value_bstride, P, K, img, H, W, bins, lo, scale,
                                                 min_depth, pool, nullptr, hist);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

int launch_soft_grad(const char *who, bool masked, const float *pc, int64_t pc_bstride, int64_t pc_cstride, int32_t B, int32_t N,
                     const float *value, int64_t value_bstride, const double *P, int32_t K, const uint8_t *img, int32_t H, int32_t W,
                     int32_t bins, float lo, float hi, double min_depth, int32_t pool, const double *table, const uint8_t *flag,
                     const uint32_t *total, const uint32_t *mask, double *part, void *stream) {
    SCORE_ARG(pc && value && P && img && table && flag && total && part,
             "%s: null pointer (pc %p, value %p, P %p, img %p, table %p, flag %p, total %p, part %p)", who, (const void *)pc,
             (const void *)value, (const void *)P, (const void *)img, (const void *)table, (const void *)flag, (const void *)total, (void *)part);
    SCORE_ARG(!masked || mask, "%s: null pointer (mask %p)", who, (const void *)mask);
    float scale = 0.f;
    if (int rc = check_points(who, B, N, K, H, W, bins, lo, hi, min_depth, pool, &scale)) return rc;
    const dim3 grid(cdiv(N, EFGH_SCORE_CHUNK), K, B);
    if (masked)
        k_soft_grad<true><<<grid, TPB, 0, (hipStream_t)stream>>>(pc, pc_bstride, pc_cstride, N, value, value_bstride, P, K, img, H, W, bins,
                                                                 lo, scale, min_depth, pool, table, flag, total, mask, part);
    else
        k_soft_grad<false><<<grid, TPB, 0, (hipStream_t)stream>>>(pc, pc_bstride, pc_cstride, N, value, value_bstride, P, K, img, H, W, bins,
                                                                  lo, scale, min_depth, pool, table, flag, total, nullptr, part);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}
}  // namespace

extern "C" int efgh_score_soft_hist(const float *pc, int64_t pc_bstride, int64_t pc_cstride, int32_t B, int32_t N, const float *value,
                                    int64_t value_bstride, const double *P, int32_t K, const uint8_t *img, int32_t H, int32_t W,
                                    int32_t bins, float lo, float hi, double min_depth, int32_t pool, uint32_t *hist, void *stream) {
    return launch_soft_hist("efgh_score_soft_hist", false, pc, pc_bstride, pc_cstride, B, N, value, value_bstride, P, K, img, H, W, bins, lo,
                            hi, min_depth, pool, nullptr, hist, stream);
}

extern "C" int efgh_score_soft_hist_masked(const float *pc, int64_t pc_bstride, int64_t pc_cstride, int32_t B, int32_t N,
                                           const float *value, int64_t value_bstride, const double *P, int32_t K, const uint8_t *img,
                                           int32_t H, int32_t W, int32_t bins, float lo, float hi, double min_depth, int32_t pool,
                                           const uint32_t *mask, uint32_t *hist, void *stream) {
    return launch_soft_hist("efgh_score_soft_hist_masked", true, pc, pc_bstride, pc_cstride, B, N, value, value_bstride, P, K, img, H, W,
                            bins, lo, hi, min_depth, pool, mask, hist, stream);
}

extern "C" int efgh_score_soft_table(const uint32_t *hist, int32_t n_hist, int32_t bins, double *table, uint8_t *flag, uint32_t *total,
                                     void *stream) {
    SCORE_ARG(hist && table && flag && total, "efgh_score_soft_table: null pointer (hist %p, table %p, flag %p, total %p)", (const void *)hist,
             (void *)table, (void *)flag, (void *)total);
    SCORE_ARG(bins_ok(bins), "efgh_score_soft_table: bins = %d, supported are 8, 16, 32 and 64", (int)bins);
    SCORE_ARG(n_hist > 0 && (int64_t)n_hist <= 65535LL * MAX_K, "efgh_score_soft_table: n_hist = %d histograms, supported are 1 .. %lld",
             (int)n_hist, 65535LL * MAX_K);
    k_soft_table<<<n_hist, TPB, 0, (hipStream_t)stream>>>(hist, bins, table, flag, total);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_score_soft_grad(const float *pc, int64_t pc_bstride, int64_t pc_cstride, int32_t B, int32_t N, const float *value,
                                    int64_t value_bstride, const double *P, int32_t K, const uint8_t *img, int32_t H, int32_t W,
                                    int32_t bins, float lo, float hi, double min_depth, int32_t pool, const double *table,
                                    const uint8_t *flag, const uint32_t *total, double *part, void *stream) {
    return launch_soft_grad("efgh_score_soft_grad", false, pc, pc_bstride, pc_cstride, B, N, value, value_bstride, P, K, img, H, W, bins, lo,
                            hi, min_depth, pool, table, flag, total, nullptr, part, stream);
}

extern "C" int efgh_score_soft_grad_masked(const float *pc, int64_t pc_bstride, int64_t pc_cstride, int32_t B, int32_t N,
                                           const float *value, int64_t value_bstride, const double *P, int32_t K, const uint8_t *img,
                                           int32_t H, int32_t W, int32_t bins, float lo, float hi, double min_depth, int32_t pool,
                                           const double *table, const uint8_t *flag, const uint32_t *total, const uint32_t *mask,
                                           double *part, void *stream) {
    return launch_soft_grad("efgh_score_soft_grad_masked", true, pc, pc_bstride, pc_cstride, B, N, value, value_bstride, P, K, img, H, W,
                            bins, lo, hi, min_depth, pool, table, flag, total, mask, part, stream);
}

extern "C" int efgh_score_soft_fold(const double *part, int32_t B, int32_t K, int32_t n_chunk, double *grad, void *stream) {
    SCORE_ARG(part && grad, "efgh_score_soft_fold: null pointer (part %p, grad %p)", (const void *)part, (void *)grad);
    SCORE_ARG(K > 0 && K <= MAX_K && B > 0 && B <= 65535, "efgh_score_soft_fold: B = %d (1 .. 65535), K = %d (1 .. %d)", (int)B, (int)K, MAX_K);
    SCORE_ARG(n_chunk > 0 && n_chunk <= MAX_FOLD, "efgh_score_soft_fold: n_chunk = %d, supported are 1 .. %d", (int)n_chunk, MAX_FOLD);
    int npow = 1;
    while (npow < n_chunk) npow <<= 1;
    k_soft_fold<<<B * K, TPB, 0, (hipStream_t)stream>>>(part, n_chunk, npow, grad);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}
