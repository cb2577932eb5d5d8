// Climbing from many start poses at once ("Many starts"): what `refine` does between two scorings with about forty torch
// launches - the chain rule from dMI/dP to six rigid parameters, Adam, the next pose, the best-so-far bookkeeping - as ONE launch
// for every start, and the selection of the starts from a scored grid.  Two kernels:
//   k_refine_step    one THREAD per parameter row ((b, s), or s alone when the batch shares its parameters): bookkeeping for the
//                    iterate just scored, chain rule, Adam, the next pose for every b of the row
//   k_refine_select  one workgroup per row of K <= 4096 values held in LDS: `keep` rounds of a block arg-max
// Both are small and latency-bound by design: a launch is a few hundred threads doing a few hundred float64 operations each.  They
// are there to replace launches and host work, not for device throughput (tools/bench_refine_multi.py is the tool that times them).
// Float64 with every operation rounded on its own (-ffp-contract=off; tests/refine_contract.py restates it in numpy), plain stores
// only, no atomic: the same bits on every run and for every grid shape.  The argument checks are api.cpp's.
#include "refine.h"

namespace {
constexpr int STEP_TPB = 64;                     // one wave: a thread is a row, and 4096 rows are 64 workgroups
constexpr int SEL_TPB = 256;
constexpr double BETA1 = 0.9, BETA2 = 0.999, ADAM_EPS = 1e-8;      // torch.optim.Adam's defaults; lr = 1 is in step_size

// the nine entries of R = Rz Ry Rx as score.py's _rigid writes them, from the sines and cosines of the three angles
__device__ __forceinline__ void rotation(double sx, double cx, double sy, double cy, double sz, double cz, double R[3][3]) {
    R[0][0] = cz * cy; R[0][1] = cz * sy * sx - sz * cx; R[0][2] = cz * sy * cx + sz * sx;
    R[1][0] = sz * cy; R[1][1] = sz * sy * sx + cz * cx; R[1][2] = sz * sy * cx - cz * sx;
    R[2][0] = -sy;     R[2][1] = cy * sx;                R[2][2] = cy * cx;
}

__global__ void __launch_bounds__(STEP_TPB)
k_refine_step(const double *__restrict__ G, const double *__restrict__ Pstart, double *__restrict__ P, const double *__restrict__ mi,
              int B, int S, int pool, double *__restrict__ z, double *__restrict__ m, double *__restrict__ v,
              double *__restrict__ best_mi, long long *__restrict__ best_iter, double *__restrict__ best_pose, double *__restrict__ trace,
              efgh_refine_scale scale, int it, double step_size, double bc2_sqrt, int last) {
    const int rows = pool ? S : B * S;
    const int r = blockIdx.x * STEP_TPB + threadIdx.x;
    if (r >= rows) return;
    // the samples of this row: b0 .. b0 + nb - 1, at matrix (b S + s)
    const int s = pool ? r : r % S, b0 = pool ? 0 : r / S, nb = pool ? B : 1;

    // 1. bookkeeping for the iterate that P holds
    const double now = mi[r];
    trace[(long long)it * rows + r] = now;
    if (it == 0 || now > best_mi[r]) {
        best_mi[r] = now;
        best_iter[r] = it;
        for (int b = b0; b < b0 + nb; ++b) {
            const long long o = ((long long)b * S + s) * 12;
            for (int e = 0; e < 12; ++e) best_pose[o + e] = P[o + e];
        }
    }
    if (last) return;

    // 2. chain rule at p = z * scale
    double zz[6], p[6];
    for (int a = 0; a < 6; ++a) { zz[a] = z[(long long)r * 6 + a]; p[a] = zz[a] * scale.s[a]; }
    double tot[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    {
        const double sx = sin(p[0]), cx = cos(p[0]), sy = sin(p[1]), cy = cos(p[1]), sz = sin(p[2]), cz = cos(p[2]);
        double R[3][3], dR[3][3][3];
        rotation(sx, cx, sy, cy, sz, cz, R);
        for (int i = 0; i < 3; ++i) { dR[0][i][0] = 0.0; dR[0][i][1] = R[i][2]; dR[0][i][2] = -R[i][1]; }
        dR[1][0][0] = -(cz * sy); dR[1][0][1] = cz * cy * sx;  dR[1][0][2] = cz * cy * cx;
        dR[1][1][0] = -(sz * sy); dR[1][1][1] = sz * cy * sx;  dR[1][1][2] = sz * cy * cx;
        dR[1][2][0] = -cy;        dR[1][2][1] = -(sy * sx);    dR[1][2][2] = -(sy * cx);
        for (int j = 0; j < 3; ++j) { dR[2][0][j] = -R[1][j]; dR[2][1][j] = R[0][j]; dR[2][2][j] = 0.0; }
        for (int b = b0; b < b0 + nb; ++b) {
            const double *__restrict__ A = Pstart + ((long long)b * S + s) * 12;
            const double *__restrict__ g = G + ((long long)b * S + s) * 12;
            for (int a = 0; a < 3; ++a) {
                double sub = 0.0;
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) {
                        const double gij = g[i * 4 + j];
                        if (gij != 0.0) sub = sub + gij * ((A[i * 4 + 0] * dR[a][0][j] + A[i * 4 + 1] * dR[a][1][j]) + A[i * 4 + 2] * dR[a][2][j]);
                    }
                tot[a] = tot[a] + sub;
            }
            for (int k = 0; k < 3; ++k) {
                double sub = 0.0;
                for (int i = 0; i < 3; ++i) {
                    const double gi3 = g[i * 4 + 3];
                    if (gi3 != 0.0) sub = sub + gi3 * A[i * 4 + k];
                }
                tot[3 + k] = tot[3 + k] + sub;
            }
        }
    }

    // 3. Adam on -mi
    bool moved = false;
    for (int a = 0; a < 6; ++a) {
        const double grad = scale.s[a] == 0.0 ? 0.0 : -(scale.s[a] * tot[a]);
        const long long o = (long long)r * 6 + a;
        const double ma = BETA1 * m[o] + (1.0 - BETA1) * grad;
        const double va = BETA2 * v[o] + (1.0 - BETA2) * (grad * grad);
        const double denom = sqrt(va) / bc2_sqrt + ADAM_EPS;
        zz[a] = zz[a] - step_size * (ma / denom);
        m[o] = ma; v[o] = va; z[o] = zz[a];
        p[a] = zz[a] * scale.s[a];
        moved = moved || zz[a] != 0.0;
    }

    // 4. the next pose for every b of the row; an all-zero z is the start itself, not the start times a computed identity
    double R[3][3];
    if (moved) rotation(sin(p[0]), cos(p[0]), sin(p[1]), cos(p[1]), sin(p[2]), cos(p[2]), R);
    for (int b = b0; b < b0 + nb; ++b) {
        const long long o = ((long long)b * S + s) * 12;
        const double *__restrict__ A = Pstart + o;
        for (int i = 0; i < 3; ++i) {
            const double a0 = A[i * 4 + 0], a1 = A[i * 4 + 1], a2 = A[i * 4 + 2], a3 = A[i * 4 + 3];
            if (moved) {
                for (int j = 0; j < 3; ++j) P[o + i * 4 + j] = (a0 * R[0][j] + a1 * R[1][j]) + a2 * R[2][j];
                P[o + i * 4 + 3] = ((a0 * p[3] + a1 * p[4]) + a2 * p[5]) + a3;
            } else {
                P[o + i * 4 + 0] = a0; P[o + i * 4 + 1] = a1; P[o + i * 4 + 2] = a2; P[o + i * 4 + 3] = a3;
            }
        }
    }
}

// does (a, ia) rank in front of (b, ib)?  An index < 0 is no entry.  Larger first, equals by ascending index, a NaN behind every number
__device__ __forceinline__ bool in_front(double a, int ia, double b, int ib) {
    if (ia < 0) return false;
    if (ib < 0) return true;
    const bool na = a != a, nb = b != b;
    if (na != nb) return nb;
    if (!na && a != b) return a > b;
    return ia < ib;
}

__global__ void __launch_bounds__(SEL_TPB)
k_refine_select(const double *__restrict__ val, int K, int keep, int *__restrict__ idx) {
    __shared__ double sv[EFGH_REFINE_MAX_S];
    __shared__ unsigned char taken[EFGH_REFINE_MAX_S];
    __shared__ double wv[SEL_TPB / 64];
    __shared__ int wi[SEL_TPB / 64];
    const double *__restrict__ row = val + (long long)blockIdx.x * K;
    for (int i = threadIdx.x; i < K; i += SEL_TPB) { sv[i] = row[i]; taken[i] = 0; }
    __syncthreads();
    for (int round = 0; round < keep; ++round) {
        double bv = 0.0;
        int bi = -1;
        for (int i = threadIdx.x; i < K; i += SEL_TPB)
            if (!taken[i] && in_front(sv[i], i, bv, bi)) { bv = sv[i]; bi = i; }
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (in_front(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if ((threadIdx.x & 63) == 0) { wv[threadIdx.x >> 6] = bv; wi[threadIdx.x >> 6] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < SEL_TPB / 64; ++w)
                if (in_front(wv[w], wi[w], bv, bi)) { bv = wv[w]; bi = wi[w]; }
            idx[(long long)blockIdx.x * keep + round] = bi;      // (keep <= K: there is always an entry left)
            taken[bi] = 1;
        }
        __syncthreads();
    }
}
}  // namespace

int efgh_launch_refine_step(const double *G, const double *Pstart, double *P, const double *mi, int B, int S, int pool, double *z, double *m,
                            double *v, double *best_mi, int64_t *best_iter, double *best_pose, double *trace, efgh_refine_scale scale, int it,
                            double step_size, double bc2_sqrt, int last, hipStream_t st) {
    const int rows = pool ? S : B * S;
    k_refine_step<<<cdiv(rows, STEP_TPB), STEP_TPB, 0, st>>>(G, Pstart, P, mi, B, S, pool, z, m, v, best_mi, (long long *)best_iter, best_pose,
                                                             trace, scale, it, step_size, bc2_sqrt, last);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

int efgh_launch_refine_select(const double *val, int rows, int K, int keep, int32_t *idx, hipStream_t st) {
    k_refine_select<<<rows, SEL_TPB, 0, st>>>(val, K, keep, idx);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}
