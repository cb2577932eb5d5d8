// Gradient guard of the fused training step: global-norm clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) and skipping of
// non-finite steps, decided on the device.  Three launches, no host read, no atomics - the first two are here:
//   k_guard_measure  one pass over the flat gradient (HBM-bound, 4n bytes): float64 sum of squares and an exact count of inf / NaN
//                    elements per run of EFGH_GUARD_RUN elements, one workgroup per run, fixed tree
//   k_guard_decide   one workgroup folds the runs per segment (fixed tree) and writes the state block: norms, clip coefficient,
//                    skip flag, step counters, Adam's bias corrections
//   k_adam_flat<true>  Adam (adam.hip) with scale, bias corrections and skip flag read from the state block
#include "common.h"

namespace {
constexpr int RUN = EFGH_GUARD_RUN;
constexpr int GTPB = 256;
static_assert(RUN % (4 * GTPB) == 0, "a run is a whole number of float4 sweeps of the workgroup");

struct GuardSegs {
    long long b[EFGH_GUARD_MAX_SEGMENTS + 1];
    int nseg;
};

__device__ __forceinline__ long long runs_of(long long len) { return (len + RUN - 1) / RUN; }

__device__ __forceinline__ void guard_take(float x, double &acc, int &bad) {
    const double d = (double)x;                    // widened BEFORE the square: no fp32 product exists that could overflow or flush
    acc += d * d;
    bad += ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) ? 1 : 0;
}

// sum over the 256 threads in a fixed tree: xor butterfly inside each wave (both partners add the same two values, so every lane
// holds the same bits), then (w0 + w1) + (w2 + w3) by thread 0.  The result is valid in thread 0 only.
template <typename T>
__device__ __forceinline__ T block_tree(T v, T *sh) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const T r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();                               // sh is reused by the caller's next reduction
    return r;
}

// run r (numbered segment by segment) covers [a, e) of its segment.  Lane mapping by ABSOLUTE float4 index (a rounded down to a
// multiple of 4), so every vector load is 16-byte aligned whatever the segment start; a float4 that straddles a or e is read
// element by element (nothing outside [a, e) is touched: the buffer may end at e).  Which thread sums which element, and in which
// order, depends on the indices alone.
__global__ void __launch_bounds__(GTPB)
k_guard_measure(const float *__restrict__ g, GuardSegs sg, long long total_runs, double *__restrict__ part, int *__restrict__ cnt) {
    __shared__ double sh_s[4];
    __shared__ int sh_c[4];
    for (long long r = blockIdx.x; r < total_runs; r += gridDim.x) {
        int s = 0;
        long long r0 = r;
        for (; s < sg.nseg - 1; ++s) {
            const long long nr = runs_of(sg.b[s + 1] - sg.b[s]);
            if (r0 < nr) break;
            r0 -= nr;
        }
        const long long a = sg.b[s] + r0 * RUN;
        const long long e = a + RUN < sg.b[s + 1] ? a + RUN : sg.b[s + 1];
        double acc = 0.0;
        int bad = 0;
        // an unaligned run spans SWEEPS + 1 sweeps of the workgroup; the whole float4s are loaded up front (all in flight together),
        // then summed in sweep order
        constexpr int SWEEPS = RUN / (4 * GTPB);
        const long long i0 = (a & ~3LL) + 4 * (long long)threadIdx.x;
        float4 x[SWEEPS + 1];
#pragma unroll
        for (int k = 0; k <= SWEEPS; ++k) {
            const long long i = i0 + (long long)k * 4 * GTPB;
            if (i >= a && i + 4 <= e) x[k] = *reinterpret_cast<const float4 *>(g + i);
        }
#pragma unroll
        for (int k = 0; k <= SWEEPS; ++k) {
            const long long i = i0 + (long long)k * 4 * GTPB;
            if (i >= a && i + 4 <= e) {
                guard_take(x[k].x, acc, bad); guard_take(x[k].y, acc, bad); guard_take(x[k].z, acc, bad); guard_take(x[k].w, acc, bad);
            } else if (i < e) {
                for (int q = 0; q < 4; ++q)
                    if (i + q >= a && i + q < e) guard_take(g[i + q], acc, bad);
            }
        }
        const double rs = block_tree(acc, sh_s);
        const int rc = block_tree(bad, sh_c);
        if (threadIdx.x == 0) { part[r] = rs; cnt[r] = rc; }
    }
}

__global__ void __launch_bounds__(GTPB)
k_guard_decide(const double *__restrict__ part, const int *__restrict__ cnt, GuardSegs sg, efgh_guard_state *__restrict__ st,
               double max_norm, float grad_scale, int skip_nonfinite, float b1, float b2, int host_step, float host_bc1,
               float host_bc2_sqrt) {
    __shared__ double sh_s[4];
    __shared__ long long sh_c[4];
    double seg_sum[EFGH_GUARD_MAX_SEGMENTS];           // (thread 0's copies are the ones used)
    long long seg_bad[EFGH_GUARD_MAX_SEGMENTS];
    long long base = 0;
#pragma unroll
    for (int s = 0; s < EFGH_GUARD_MAX_SEGMENTS; ++s) {
        seg_sum[s] = 0.0; seg_bad[s] = 0;
        if (s < sg.nseg) {                             // (uniform over the workgroup)
            const long long nr = runs_of(sg.b[s + 1] - sg.b[s]);
            double acc = 0.0;
            long long bad = 0;
            for (long long r = threadIdx.x; r < nr; r += GTPB) { acc += part[base + r]; bad += cnt[base + r]; }
            seg_sum[s] = block_tree(acc, sh_s);
            seg_bad[s] = block_tree(bad, sh_c);
            base += nr;
        }
    }
    if (threadIdx.x != 0) return;
    double total = 0.0;
    long long bad = 0;
#pragma unroll
    for (int s = 0; s < EFGH_GUARD_MAX_SEGMENTS; ++s) {
        st->sumsq[s] = seg_sum[s]; st->nonfinite[s] = seg_bad[s];
        if (s < sg.nseg) { total += seg_sum[s]; bad += seg_bad[s]; }
    }
    const double norm = sqrt(total) * (double)grad_scale;
    const double c = max_norm / (norm + 1e-6);         // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1); a NaN stays
    const float coef = (float)(c > 1.0 ? 1.0 : c);
    long long applied = st->applied, skipped = st->skipped;
    int skip = 0;
    float bc1 = host_bc1, bc2_sqrt = host_bc2_sqrt;
    if (skip_nonfinite) {
        if (bad != 0) { skip = 1; skipped += 1; } else applied += 1;
        const float p1 = (float)pow((double)b1, (double)applied), p2 = (float)pow((double)b2, (double)applied);
        bc1 = 1.f - p1;
        bc2_sqrt = sqrtf(1.f - p2);
    } else {
        applied = host_step;
    }
    st->sumsq_total = total; st->norm = norm; st->nonfinite_total = bad;
    st->applied = applied; st->skipped = skipped;
    st->coef = coef; st->scale = grad_scale * coef;
    st->bc1 = bc1; st->bc2_sqrt = bc2_sqrt;
    st->skip = skip; st->nseg = sg.nseg;
}

long long max_runs(long long n) { return n / RUN + EFGH_GUARD_MAX_SEGMENTS; }      // sum of ceil(len_s / RUN) over <= 8 segments
}  // namespace

extern "C" int64_t efgh_grad_guard_workspace(int64_t n) {
    if (n < 1 || n >= (1ll << 31)) return -1;
    return (max_runs(n) * 12 + 15) / 16 * 16;
}

extern "C" int efgh_grad_guard_measure(const float *g, int64_t n, const int64_t *bounds, int32_t nseg, double max_norm,
                                       float grad_scale, int32_t skip_nonfinite, float beta1, float beta2, int32_t step,
                                       void *workspace, efgh_guard_state *state, int32_t grid, void *stream) {
    EFGH_CHECK_ARG(g && bounds && workspace && state);
    EFGH_CHECK_ARG(n >= 1 && n < (1ll << 31));
    EFGH_CHECK_ARG(nseg >= 1 && nseg <= EFGH_GUARD_MAX_SEGMENTS);
    EFGH_CHECK_ARG(bounds[0] == 0 && bounds[nseg] == n);
    for (int s = 0; s < nseg; ++s) EFGH_CHECK_ARG(bounds[s] < bounds[s + 1]);       // sorted, no empty segment
    EFGH_CHECK_ARG(max_norm > 0.0);                                                 // (false for a NaN)
    EFGH_CHECK_ARG(grad_scale == grad_scale && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f);
    EFGH_CHECK_ARG(skip_nonfinite || step >= 1);
    EFGH_CHECK_ARG(grid >= 0);
    EFGH_CHECK_ARG((((uintptr_t)g) & 15) == 0 && ((((uintptr_t)workspace) | ((uintptr_t)state)) & 7) == 0);
    GuardSegs sg;
    long long total_runs = 0;
    for (int s = 0; s <= EFGH_GUARD_MAX_SEGMENTS; ++s) sg.b[s] = bounds[s < nseg ? s : nseg];
    for (int s = 0; s < nseg; ++s) total_runs += (bounds[s + 1] - bounds[s] + RUN - 1) / RUN;
    sg.nseg = nseg;
    double *part = (double *)workspace;
    int *cnt = (int *)(part + max_runs(n));
    const long long blocks = grid > 0 ? grid : (total_runs > 16384 ? 16384 : total_runs);
    efgh_bias_corr bc = {0.f, 0.f};
    if (!skip_nonfinite) bc = efgh_bias_corrections(beta1, beta2, step);
    k_guard_measure<<<(int)blocks, GTPB, 0, (hipStream_t)stream>>>(g, sg, total_runs, part, cnt);
    EFGH_CHECK_LAUNCH();
    k_guard_decide<<<1, GTPB, 0, (hipStream_t)stream>>>(part, cnt, sg, state, max_norm, grad_scale, skip_nonfinite ? 1 : 0, beta1,
                                                        beta2, step, bc.bc1, bc.bc2_sqrt);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}
