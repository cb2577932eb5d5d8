// Scoring poses on VISIBLE points only ("Scoring on visible points"): a depth test per candidate, and the occupancy counts
// of the Miller-Madow correction.  LiDAR and camera sit apart, so a point on a far surface can land on a pixel that shows a nearer
// one; which points those are changes with the candidate, so every (b, k) gets a coarse z-buffer of its own.  The image is cut into
// cells of cell_h x cell_w pixels (clipped at the right and bottom edges: Hc = ceil(H / cell_h), Wc = ceil(W / cell_w)).  Kernels:
//   k_score_zmin      grid (point chunk, k, b), k_score_hist's shape: an in-frame point takes the unsigned minimum of its float32
//                     depth's bit pattern with its cell of zmin [B][K][Hc][Wc] - ONE no-return 32-bit global atomicMin a point, no
//                     load in front of it (fuse.hip built that variant: several times slower, profiles/fuse.txt), no CAS loop, no
//                     floating-point atomic.  Depths are positive floats, whose bit patterns order like unsigned integers; the buffer
//                     starts as +inf (0x7f800000).  The point's value plays no part: a point with a NaN reflectance still occludes
//   k_score_visible   a SEPARATE launch behind it: projects again, visible iff in frame and (double)d <= (double)zmin (1 + rel_tol) +
//                     abs_tol (efgh_fuse_resolve's expression, in its order); a wave's ballot is two mask words, written with plain
//                     stores by lanes 0 and 32.  mask [B][K][ceil(N / 32)]: bit i % 32 of word i / 32; bits past N are zero.  Every
//                     word is written: the mask takes no atomic and no memset
//   k_score_occ       one workgroup per histogram: the non-empty rows, columns and cells as integers
// An integer minimum does not depend on the order of its operands: the same bits on every schedule.  Built with -ffp-contract=off for
// the projection and for the bound, whose product and sum round separately (tests/score_vis_contract.py restates both in numpy).
// The masked histograms and the masked gradient are the MASKED instances of score.hip's and score_soft.hip's kernels.
#include "score_common.h"

namespace {
constexpr unsigned INF_BITS = 0x7f800000u;
constexpr int MAX_CELL = 64;
constexpr long long MAX_ZMIN_CELLS = 1LL << 29;                  // a memory sanity cap (2 GiB of workspace), not a measurement

__global__ void __launch_bounds__(TPB)
k_score_zmin(const float *__restrict__ pc, long long bs, long long cs, int N, const double *__restrict__ P, int K, int H, int W,
             int cell_h, int cell_w, int Wc, long long cells, double min_depth, unsigned *__restrict__ zmin) {
    const int k = blockIdx.y, b = blockIdx.z;
    const float *__restrict__ pcb = pc + b * bs;
    const double *__restrict__ T = P + 12 * ((long long)b * K + k);
    unsigned *__restrict__ z = zmin + ((long long)b * K + k) * cells;          // (64-bit: B K Hc Wc goes up to 2^29)
    const long long first = (long long)blockIdx.x * EFGH_SCORE_CHUNK;
    const long long end = min(first + EFGH_SCORE_CHUNK, (long long)N);
    for (long long j = first + threadIdx.x; j < end; j += TPB) {
        const Hit h = project(pcb, cs, (int)j, T, H, W, min_depth);
        if (h.state != ST_OCCLUDED) continue;                    // not in frame
        // r < H and c < W: the cell index is below Hc * Wc.  The result is not used: the no-return form
        atomicMin(z + ((long long)(h.r / cell_h) * Wc + h.c / cell_w), __float_as_uint(h.d));
    }
}

__global__ void __launch_bounds__(TPB)
k_score_visible(const float *__restrict__ pc, long long bs, long long cs, int N, const double *__restrict__ P, int K, int H, int W,
                int cell_h, int cell_w, int Wc, long long cells, double min_depth, double rel_tol, double abs_tol,
                const unsigned *__restrict__ zmin, unsigned *__restrict__ mask) {
    const int k = blockIdx.y, b = blockIdx.z;
    const float *__restrict__ pcb = pc + b * bs;
    const double *__restrict__ T = P + 12 * ((long long)b * K + k);
    const unsigned *__restrict__ z = zmin + ((long long)b * K + k) * cells;
    unsigned *__restrict__ mk = mask + ((long long)b * K + k) * mask_words(N);
    const long long first = (long long)blockIdx.x * EFGH_SCORE_CHUNK;
    const long long end = min(first + EFGH_SCORE_CHUNK, (long long)N);
    const int lane = threadIdx.x & 63;
    // the trip count is the block's, not the thread's: every lane of a wave reaches the ballot.  first and TPB are multiples of 64,
    // so a wave holds 64 consecutive points that start on a word boundary
    for (long long j0 = first; j0 < end; j0 += TPB) {
        const long long j = j0 + threadIdx.x;
        bool vis = false;
        if (j < end) {
            const Hit h = project(pcb, cs, (int)j, T, H, W, min_depth);
            if (h.state == ST_OCCLUDED) {
                const float zm = __uint_as_float(z[(long long)(h.r / cell_h) * Wc + h.c / cell_w]);
                const double bound = (double)zm * (1.0 + rel_tol) + abs_tol;
                vis = (double)h.d <= bound;
            }
        }
        const unsigned long long m = __ballot(vis);
        // point j starts a word iff j % 32 == 0; the word exists iff that point does
        if (lane == 0 && j < end) mk[j >> 5] = (unsigned)m;
        if (lane == 32 && j < end) mk[j >> 5] = (unsigned)(m >> 32);
    }
}

__global__ void __launch_bounds__(TPB)
k_score_occ(const unsigned *__restrict__ hist, int bins, int *__restrict__ occ) {
    __shared__ int row[MAX_BINS], col[MAX_BINS];
    __shared__ int n[3];
    const int nb = bins * bins;
    const unsigned *__restrict__ h = hist + (long long)blockIdx.x * nb;
    if (threadIdx.x < MAX_BINS) row[threadIdx.x] = col[threadIdx.x] = 0;
    if (threadIdx.x < 3) n[threadIdx.x] = 0;
    __syncthreads();
    int mine = 0;
    for (int c = threadIdx.x; c < nb; c += TPB)
        if (h[c]) { ++mine; atomicOr(&row[c / bins], 1); atomicOr(&col[c % bins], 1); }
    if (mine) atomicAdd(&n[2], mine);
    __syncthreads();
    if (threadIdx.x < bins) {
        if (row[threadIdx.x]) atomicAdd(&n[0], 1);
        if (col[threadIdx.x]) atomicAdd(&n[1], 1);
    }
    __syncthreads();
    if (threadIdx.x < 3) occ[3 * (long long)blockIdx.x + threadIdx.x] = n[threadIdx.x];
}

// the checks efgh_score_zmin and efgh_score_visible share -> Hc, Wc
int check_vis(const char *who, const void *pc, int B, int N, const void *P, int K, int H, int W, int cell_h, int cell_w, double min_depth,
              int *Hc, int *Wc) {
    SCORE_ARG(pc && P, "%s: null pointer (pc %p, P %p)", who, pc, P);
    SCORE_ARG(K > 0 && K <= MAX_K, "%s: K = %d candidates, supported are 1 .. %d", who, K, MAX_K);
    SCORE_ARG(B > 0 && B <= 65535, "%s: B = %d, supported are 1 .. 65535", who, B);
    SCORE_ARG(N > 0 && (int64_t)N < 0x7fffffffLL, "%s: N = %d must be positive and below 2^31", who, N);
    SCORE_ARG(H > 0 && W > 0 && (int64_t)H * W < 0x7fffffffLL, "%s: H = %d, W = %d: both positive and H*W < 2^31", who, H, W);
    SCORE_ARG(cell_h >= 1 && cell_h <= MAX_CELL && cell_w >= 1 && cell_w <= MAX_CELL,
              "%s: cell_h = %d, cell_w = %d, supported are 1 .. %d each", who, cell_h, cell_w, MAX_CELL);
    SCORE_ARG(min_depth >= 0.0 && std::isfinite(min_depth), "%s: min_depth = %g must be finite and >= 0", who, min_depth);
    *Hc = cdiv(H, cell_h);
    *Wc = cdiv(W, cell_w);
    const long long cells = (long long)B * K * *Hc * *Wc;
    SCORE_ARG(cells <= MAX_ZMIN_CELLS, "%s: B = %d, K = %d, cell %d x %d on %d x %d: %lld cells (%lld bytes) are more than 2^29", who, B, K,
              cell_h, cell_w, H, W, cells, 4 * cells);
    return EFGH_OK;
}
}  // namespace

extern "C" int64_t efgh_score_zmin_bytes(int32_t B, int32_t K, int32_t H, int32_t W, int32_t cell_h, int32_t cell_w) {
    if (B < 1 || B > 65535 || K < 1 || K > MAX_K || H < 1 || W < 1 || (int64_t)H * W >= 0x7fffffffLL || cell_h < 1 || cell_h > MAX_CELL ||
        cell_w < 1 || cell_w > MAX_CELL)
        return -1;
    const int64_t cells = (int64_t)B * K * cdiv(H, cell_h) * cdiv(W, cell_w);
    return cells > MAX_ZMIN_CELLS ? -1 : 4 * cells;
}

extern "C" int efgh_score_zmin(const float *pc, int64_t pc_bstride, int64_t pc_cstride, int32_t B, int32_t N, const double *P, int32_t K,
                               int32_t H, int32_t W, int32_t cell_h, int32_t cell_w, double min_depth, uint32_t *zmin, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    int Hc = 0, Wc = 0;
    if (int rc = check_vis("efgh_score_zmin", pc, B, N, P, K, H, W, cell_h, cell_w, min_depth, &Hc, &Wc)) return rc;
    SCORE_ARG(zmin, "efgh_score_zmin: null pointer (zmin %p)", (void *)zmin);
    const long long cells = (long long)Hc * Wc;
    if (hipMemsetD32Async((hipDeviceptr_t)zmin, (int)INF_BITS, (size_t)B * K * cells, st) != hipSuccess) {
        efgh_set_error("efgh_score_zmin: memset failed");
        return EFGH_E_LAUNCH;
    }
    k_score_zmin<<<dim3(cdiv(N, EFGH_SCORE_CHUNK), K, B), TPB, 0, st>>>(pc, pc_bstride, pc_cstride, N, P, K, H, W, cell_h, cell_w, Wc, cells,
                                                                         min_depth, zmin);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_score_visible(const float *pc, int64_t pc_bstride, int64_t pc_cstride, int32_t B, int32_t N, const double *P,
                                  int32_t K, int32_t H, int32_t W, int32_t cell_h, int32_t cell_w, double min_depth, double rel_tol,
                                  double abs_tol, const uint32_t *zmin, uint32_t *mask, void *stream) {
    int Hc = 0, Wc = 0;
    if (int rc = check_vis("efgh_score_visible", pc, B, N, P, K, H, W, cell_h, cell_w, min_depth, &Hc, &Wc)) return rc;
    SCORE_ARG(zmin && mask, "efgh_score_visible: null pointer (zmin %p, mask %p)", (const void *)zmin, (void *)mask);
    SCORE_ARG(rel_tol >= 0.0 && std::isfinite(rel_tol), "efgh_score_visible: rel_tol = %g must be finite and >= 0", rel_tol);
    SCORE_ARG(abs_tol >= 0.0 && std::isfinite(abs_tol), "efgh_score_visible: abs_tol = %g must be finite and >= 0", abs_tol);
    k_score_visible<<<dim3(cdiv(N, EFGH_SCORE_CHUNK), K, B), TPB, 0, (hipStream_t)stream>>>(
        pc, pc_bstride, pc_cstride, N, P, K, H, W, cell_h, cell_w, Wc, (long long)Hc * Wc, min_depth, rel_tol, abs_tol, zmin, mask);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_score_occupancy(const uint32_t *hist, int32_t n_hist, int32_t bins, int32_t *occ, void *stream) {
    SCORE_ARG(hist && occ, "efgh_score_occupancy: null pointer (hist %p, occ %p)", (const void *)hist, (void *)occ);
    SCORE_ARG(bins_ok(bins), "efgh_score_occupancy: bins = %d, supported are 8, 16, 32 and 64", (int)bins);
    SCORE_ARG(n_hist > 0 && (int64_t)n_hist <= 65535LL * MAX_K, "efgh_score_occupancy: n_hist = %d histograms, supported are 1 .. %lld",
              (int)n_hist, 65535LL * MAX_K);
    k_score_occ<<<n_hist, TPB, 0, (hipStream_t)stream>>>(hist, bins, occ);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}
