// Scoring candidate poses of a LiDAR / camera pair without ground truth ("Scoring poses"): the mutual information between
// a per-point scalar (reflectance, a range) and the image grey level under the projected point, for K candidate matrices per sample
// in one launch.  Two kernels:
//   k_score_hist   grid (point chunk, k, b): the block's points through fuse_project.h's projection under candidate k, an in-frame
//                  point adds 1 to cell (value bin, grey bin) of a bins x bins histogram in LDS (integer LDS atomics); the non-zero
//                  cells then go to the global histogram with integer atomicAdd
//   k_score_mi     one workgroup per (b, k): marginals, total, and in float64 the three sums of c log c through a fixed pairwise
//                  tree of plain LDS stores; entropies, mi, nmi
// Integer sums do not depend on their order, and the float64 tree has one shape and one order: the same bits on every schedule and
// run.  There is no floating-point atomic.  k_score_hist has ONE body and two instances: the plain one asks nothing about occlusion;
// the MASKED one (efgh_score_hist_masked) also wants the point's bit in a per-candidate visibility mask, which score_vis.hip builds
// from a coarse z-buffer per candidate (efgh_score_zmin, efgh_score_visible).  The Miller-Madow correction of the sparse
// histogram's bias is formed from efgh_score_occupancy's counts (score_vis.hip) in efgh_amd/common/score_vis.py.  Built with
// -ffp-contract=off for the projection and for the value bin, whose subtraction and product round separately
// (tests/score_contract.py restates both in numpy).
#include "score_common.h"

namespace {
template <bool MASKED>
__global__ void __launch_bounds__(TPB)
k_score_hist(const float *__restrict__ pc, long long bs, long long cs, int N, const float *__restrict__ value, long long vbs,
             const double *__restrict__ P, int K, const uint8_t *__restrict__ img, int H, int W, int bins, float lo, float scale,
             double min_depth, const unsigned *__restrict__ mask, unsigned *__restrict__ hist) {
    __shared__ unsigned cnt[MAX_BINS * MAX_BINS];
    const int k = blockIdx.y, b = blockIdx.z, nb = bins * bins;
    for (int c = threadIdx.x; c < nb; c += TPB) cnt[c] = 0u;
    __syncthreads();
    const float *__restrict__ pcb = pc + b * bs;
    const float *__restrict__ vb = value + b * vbs;
    const double *__restrict__ T = P + 12 * ((long long)b * K + k);
    const uint8_t *__restrict__ imgb = img + (long long)b * H * W * 3;
    const unsigned *__restrict__ mk = MASKED ? mask + ((long long)b * K + k) * mask_words(N) : nullptr;
    const float top = (float)(bins - 1);
    const long long first = (long long)blockIdx.x * EFGH_SCORE_CHUNK;
    const long long end = min(first + EFGH_SCORE_CHUNK, (long long)N);
    for (long long j = first + threadIdx.x; j < end; j += TPB) {  // (64-bit: j + TPB may pass 2^31 in the last chunk of the largest N)
        const int i = (int)j;
        const float v = vb[i];
        if (!(v == v)) continue;                                 // a NaN value drops the point
        if (MASKED && !mask_bit(mk, i)) continue;                // hidden under this candidate (or not in frame: the mask is a subset)
        const Hit h = project(pcb, cs, i, T, H, W, min_depth);
        if (h.state != ST_OCCLUDED) continue;                    // in frame; whether it is hidden is the mask's business
        const float t = (v - lo) * scale;                        // two float32 operations
        // clamped BEFORE the conversion: (int) of an infinity is undefined
        const int x = t >= top ? bins - 1 : (t > 0.f ? (int)t : 0);
        const int y = (luma(imgb + ((long long)h.r * W + h.c) * 3) * bins) >> 8;
        atomicAdd(&cnt[x * bins + y], 1u);
    }
    __syncthreads();
    unsigned *__restrict__ out = hist + ((long long)b * K + k) * nb;
    for (int c = threadIdx.x; c < nb; c += TPB) {
        const unsigned n = cnt[c];
        if (n) atomicAdd(out + c, n);
    }
}

__device__ __forceinline__ double clogc(unsigned c) { return c ? (double)c * log((double)c) : 0.0; }

__global__ void __launch_bounds__(TPB)
k_score_mi(const unsigned *__restrict__ hist, int bins, double *__restrict__ score, int *__restrict__ count) {
    __shared__ double t[MAX_BINS * MAX_BINS];
    __shared__ unsigned row[MAX_BINS], col[MAX_BINS];
    __shared__ unsigned total;
    __shared__ int one[3];                                        // does ONE cell hold everything (joint, rows, columns)?
    const int nb = bins * bins;
    const unsigned *__restrict__ h = hist + (long long)blockIdx.x * nb;
    if (threadIdx.x < MAX_BINS) row[threadIdx.x] = col[threadIdx.x] = 0u;
    if (threadIdx.x < 3) one[threadIdx.x] = 0;
    if (threadIdx.x == 0) total = 0u;
    __syncthreads();
    for (int c = threadIdx.x; c < nb; c += TPB) {
        const unsigned n = h[c];
        t[c] = clogc(n);
        if (n) { atomicAdd(&row[c / bins], n); atomicAdd(&col[c % bins], n); atomicAdd(&total, n); }
    }
    __syncthreads();
    const unsigned n = total;
    for (int c = threadIdx.x; c < nb; c += TPB) if (n && h[c] == n) one[0] = 1;
    const double sxy = tree_sum(t, nb);
    if (threadIdx.x < bins) { t[threadIdx.x] = clogc(row[threadIdx.x]); if (n && row[threadIdx.x] == n) one[1] = 1; }
    const double sx = tree_sum(t, bins);
    if (threadIdx.x < bins) { t[threadIdx.x] = clogc(col[threadIdx.x]); if (n && col[threadIdx.x] == n) one[2] = 1; }
    const double sy = tree_sum(t, bins);
    if (threadIdx.x == 0) {
        double *o = score + 5 * (long long)blockIdx.x;
        double hx = 0.0, hy = 0.0, hxy = 0.0;
        if (n) {
            // a distribution on one cell has entropy 0 by definition: log n - (n log n) / n need not round to it
            const double ln = log((double)n), dn = (double)n;
            hx = one[1] ? 0.0 : ln - sx / dn;
            hy = one[2] ? 0.0 : ln - sy / dn;
            hxy = one[0] ? 0.0 : ln - sxy / dn;
        }
        const double sum = hx + hy;
        o[0] = sum - hxy;
        o[1] = hxy == 0.0 ? 0.0 : sum / hxy;
        o[2] = hx; o[3] = hy; o[4] = hxy;
        count[blockIdx.x] = (int)n;
    }
}

}  // namespace

extern "C" int32_t efgh_score_chunk(void) { return EFGH_SCORE_CHUNK; }

namespace {
// the plain and the masked entry point: the same checks, the same zeroing, the same grid
int launch_hist(const char *who, bool masked, const float *pc, int64_t pc_bstride, int64_t pc_cstride, int32_t B, int32_t N,
                const float *value, int64_t value_bstride, const double *P, int32_t K, const uint8_t *img, int32_t H, int32_t W,
                int32_t bins, float lo, float hi, double min_depth, const uint32_t *mask, uint32_t *hist, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    SCORE_ARG(pc && value && P && img && hist, "%s: null pointer (pc %p, value %p, P %p, img %p, hist %p)", who, (const void *)pc,
              (const void *)value, (const void *)P, (const void *)img, (void *)hist);
    SCORE_ARG(!masked || mask, "%s: null pointer (mask %p)", who, (const void *)mask);
    SCORE_ARG(bins_ok(bins), "%s: bins = %d, supported are 8, 16, 32 and 64 (the counters live in LDS)", who, (int)bins);
    SCORE_ARG(K > 0 && K <= MAX_K, "%s: K = %d candidates, supported are 1 .. %d", who, (int)K, MAX_K);
    SCORE_ARG(B > 0 && B <= 65535, "%s: B = %d, supported are 1 .. 65535", who, (int)B);
    SCORE_ARG(N > 0 && (int64_t)N < 0x7fffffffLL, "%s: N = %d must be positive and below 2^31", who, (int)N);
    SCORE_ARG(H > 0 && W > 0 && (int64_t)H * W < 0x7fffffffLL, "%s: H = %d, W = %d: both positive and H*W < 2^31", who, (int)H, (int)W);
    SCORE_ARG(min_depth >= 0.0 && std::isfinite(min_depth), "%s: min_depth = %g must be finite and >= 0", who, min_depth);
    SCORE_ARG(std::isfinite(lo) && std::isfinite(hi) && lo < hi, "%s: value range lo = %g, hi = %g: finite and lo < hi", who,
              (double)lo, (double)hi);
    const float width = hi - lo;
    const float scale = (float)bins / width;                    // formed once, here, in float32
    SCORE_ARG(std::isfinite(width) && std::isfinite(scale) && scale > 0.f,
              "%s: value range lo = %g, hi = %g: bins / (hi - lo) is not a finite float32", who, (double)lo, (double)hi);
    if (hipMemsetAsync(hist, 0, (size_t)4 * B * K * bins * bins, st) != hipSuccess) {
        efgh_set_error("%s: memset failed", who);
        return EFGH_E_LAUNCH;
    }
    const dim3 grid(cdiv(N, EFGH_SCORE_CHUNK), K, B);
    if (masked)
        k_score_hist<true><<<grid, TPB, 0, st>>>(pc, pc_bstride, pc_cstride, N, value, value_bstride, P, K, img, H, W, bins, lo, scale,
                                                 min_depth, mask, hist);
    else
        k_score_hist<false><<<grid, TPB, 0, st>>>(pc, pc_bstride, pc_cstride, N, value, value_bstride, P, K, img, H, W, bins, lo, scale,
                                                  min_depth, nullptr, hist);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}
}  // namespace

extern "C" int efgh_score_hist(const float *pc, int64_t pc_bstride, int64_t pc_cstride, int32_t B, int32_t N, const float *value,
                               int64_t value_bstride, const double *P, int32_t K, const uint8_t *img, int32_t H, int32_t W,
                               int32_t bins, float lo, float hi, double min_depth, uint32_t *hist, void *stream) {
    return launch_hist("efgh_score_hist", false, pc, pc_bstride, pc_cstride, B, N, value, value_bstride, P, K, img, H, W, bins, lo, hi,
                       min_depth, nullptr, hist, stream);
}

extern "C" int efgh_score_hist_masked(const float *pc, int64_t pc_bstride, int64_t pc_cstride, int32_t B, int32_t N, const float *value,
                                      int64_t value_bstride, const double *P, int32_t K, const uint8_t *img, int32_t H, int32_t W,
                                      int32_t bins, float lo, float hi, double min_depth, const uint32_t *mask, uint32_t *hist,
                                      void *stream) {
    return launch_hist("efgh_score_hist_masked", true, pc, pc_bstride, pc_cstride, B, N, value, value_bstride, P, K, img, H, W, bins, lo,
                       hi, min_depth, mask, hist, stream);
}

extern "C" int efgh_score_mi(const uint32_t *hist, int32_t B, int32_t K, int32_t bins, double *score, int32_t *count, void *stream) {
    SCORE_ARG(hist && score && count, "efgh_score_mi: null pointer (hist %p, score %p, count %p)", (const void *)hist, (void *)score,
              (void *)count);
    SCORE_ARG(bins_ok(bins), "efgh_score_mi: bins = %d, supported are 8, 16, 32 and 64", (int)bins);
    SCORE_ARG(K > 0 && K <= MAX_K && B > 0 && B <= 65535, "efgh_score_mi: B = %d (1 .. 65535), K = %d (1 .. %d)", (int)B, (int)K, MAX_K);
    k_score_mi<<<B * K, TPB, 0, (hipStream_t)stream>>>(hist, bins, score, count);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}
