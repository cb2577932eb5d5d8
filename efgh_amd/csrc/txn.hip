// Transactional BatchNorm state of the guarded training step (train.BnTransaction): every running_mean / running_var of the model
// lives in ONE fp32 vector `live`, every num_batches_tracked in one int64 vector, and a skipped optimizer step puts both back.
// Three launches per optimizer step, no host read, no floating-point atomics:
//   k_txn_snapshot  shadow = live (floats and counters) before the first forward; clears the per-step fields of efgh_txn_state
//   k_txn_probe     after the last forward: exact count of the elements that are inf / NaN in live and were finite in shadow, the
//                   smallest buffer index that holds one, and one count per non-finite loss scalar.  Integer atomics only (one add
//                   and one min per workgroup that saw something): counts and minima do not depend on the arrival order
//   k_txn_resolve   after the guard's decide launch: turns a non-finite forward into a skipped step (the guard block is rewritten as
//                   k_guard_decide, guard.hip, would have left it had it skipped) and, when the step is skipped, live = shadow
// The vectors are a few tens of thousands of elements (well under 1 MB moved per step), so the launches cost their launch floor.
// float4 over the 16-byte-aligned body [0, n & ~3), the n & 3 tail elements one by one (as k_grad_drain, accum.hip); both base
// pointers are 16-byte aligned (checked); where a BUFFER starts inside the vector matters to the buffer lookup only.
#include <math.h>

#include "common.h"

namespace {
constexpr int TPB = 256;

static inline int grid_for(long long items) {
    long long b = (items + TPB - 1) / TPB;
    return (int)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// dst = src: nf floats (float4 body + tail) and nc 64-bit counters, grid-stride; bit copies (NaN payloads and -0 survive)
__device__ __forceinline__ void copy_state(float *__restrict__ dst_f, const float *__restrict__ src_f, long long nf,
                                           long long *__restrict__ dst_c, const long long *__restrict__ src_c, long long nc) {
    const long long t0 = (long long)blockIdx.x * TPB + threadIdx.x, step = (long long)gridDim.x * TPB;
    const long long n4 = nf >> 2;
    for (long long i = t0; i < n4; i += step)
        reinterpret_cast<float4 *>(dst_f)[i] = reinterpret_cast<const float4 *>(src_f)[i];
    for (long long i = (n4 << 2) + t0; i < nf; i += step) dst_f[i] = src_f[i];
    for (long long i = t0; i < nc; i += step) dst_c[i] = src_c[i];
}

__global__ void __launch_bounds__(TPB)
k_txn_snapshot(const float *__restrict__ live_f, float *__restrict__ shadow_f, long long nf, const long long *__restrict__ live_c,
               long long *__restrict__ shadow_c, long long nc, efgh_txn_state *__restrict__ txn) {
    copy_state(shadow_f, live_f, nf, shadow_c, live_c, nc);
    if (blockIdx.x == 0 && threadIdx.x == 0) { txn->forward_nonfinite = 0; txn->first_bad = -1; txn->vetoed = 0; }
}

// index of the buffer element i belongs to: the last s with starts[s] <= i (starts[0] = 0, starts[nseg] = nf)
__device__ __forceinline__ int segment_of(const long long *__restrict__ starts, int nseg, long long i) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void probe_take(float l, float s, long long i, const long long *__restrict__ starts, int nseg,
                                           int &bad, unsigned &first) {
    if (nonfinite(l) && !nonfinite(s)) {               // (rare: the lookup is paid by spoiled elements only)
        bad += 1;
        const unsigned seg = (unsigned)segment_of(starts, nseg, i);
        first = seg < first ? seg : first;
    }
}

// first_bad is kept as an UNSIGNED minimum: -1 (nothing found) is the largest value, so atomicMin needs no special case
__global__ void __launch_bounds__(TPB)
k_txn_probe(const float *__restrict__ live_f, const float *__restrict__ shadow_f, long long nf, const long long *__restrict__ starts,
            int nseg, const float *__restrict__ losses, int k, long long loss_stride, efgh_txn_state *__restrict__ txn) {
    const long long t0 = (long long)blockIdx.x * TPB + threadIdx.x, step = (long long)gridDim.x * TPB;
    const long long n4 = nf >> 2;
    int bad = 0;                                        // (a thread sees at most nf / TPB + k < 2^31 values)
    unsigned first = 0xffffffffu;
    for (long long i = t0; i < n4; i += step) {
        const float4 l = reinterpret_cast<const float4 *>(live_f)[i], s = reinterpret_cast<const float4 *>(shadow_f)[i];
        probe_take(l.x, s.x, 4 * i, starts, nseg, bad, first); probe_take(l.y, s.y, 4 * i + 1, starts, nseg, bad, first);
        probe_take(l.z, s.z, 4 * i + 2, starts, nseg, bad, first); probe_take(l.w, s.w, 4 * i + 3, starts, nseg, bad, first);
    }
    for (long long i = (n4 << 2) + t0; i < nf; i += step) probe_take(live_f[i], shadow_f[i], i, starts, nseg, bad, first);
    if (blockIdx.x == 0)
        for (int j = threadIdx.x; j < k; j += TPB) bad += nonfinite(losses[(long long)j * loss_stride]) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bad += __shfl_xor(bad, o);
        const unsigned other = __shfl_xor(first, o);
        first = other < first ? other : first;
    }
    __shared__ int sh_bad[TPB / 64];
    __shared__ unsigned sh_first[TPB / 64];
    if ((threadIdx.x & 63) == 0) { sh_bad[threadIdx.x >> 6] = bad; sh_first[threadIdx.x >> 6] = first; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        unsigned f = 0xffffffffu;
        for (int w = 0; w < TPB / 64; ++w) { total += (unsigned long long)sh_bad[w]; f = sh_first[w] < f ? sh_first[w] : f; }
        if (total) atomicAdd(reinterpret_cast<unsigned long long *>(&txn->forward_nonfinite), total);
        if (f != 0xffffffffu) atomicMin(reinterpret_cast<unsigned *>(&txn->first_bad), f);
    }
}

// The restore decision is taken by every workgroup from fields this launch only READS: guard->nonfinite_total (k_guard_decide set
// skip = (nonfinite_total != 0), the guard runs with skip_nonfinite) and txn->forward_nonfinite.  guard->skip, applied, skipped and
// the bias corrections are read and rewritten by thread 0 of workgroup 0 alone.
__global__ void __launch_bounds__(TPB)
k_txn_resolve(float *__restrict__ live_f, const float *__restrict__ shadow_f, long long nf, long long *__restrict__ live_c,
              const long long *__restrict__ shadow_c, long long nc, efgh_guard_state *__restrict__ guard,
              efgh_txn_state *__restrict__ txn, float b1, float b2) {
    const bool forward_bad = txn->forward_nonfinite != 0;
    const bool skip = forward_bad || guard->nonfinite_total != 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (forward_bad && guard->skip == 0) {          // veto: the finite gradient of a non-finite forward is not applied
            const long long applied = guard->applied - 1;
            // k_guard_decide's expressions for the bias corrections of step `applied`
            const float p1 = (float)pow((double)b1, (double)applied), p2 = (float)pow((double)b2, (double)applied);
            guard->bc1 = 1.f - p1;
            guard->bc2_sqrt = sqrtf(1.f - p2);
            guard->applied = applied;
            guard->skipped += 1;
            guard->skip = 1;
            txn->vetoed = 1;
            txn->vetoed_total += 1;
        }
        if (skip) txn->rolled_back += 1;
    }
    if (skip) copy_state(live_f, shadow_f, nf, live_c, shadow_c, nc);
}

bool aligned(const void *a, const void *b, uintptr_t mask) { return ((((uintptr_t)a) | ((uintptr_t)b)) & mask) == 0; }

// [a, a + bytes) and [b, b + bytes) do not overlap
bool apart(const void *a, const void *b, uint64_t bytes) {
    return (uintptr_t)a + bytes <= (uintptr_t)b || (uintptr_t)b + bytes <= (uintptr_t)a;
}

int check_vectors(const float *live_f, const float *shadow_f, int64_t nf, const int64_t *live_c, const int64_t *shadow_c, int64_t nc) {
    EFGH_CHECK_ARG(live_f && shadow_f && nf >= 1 && nf < (1ll << 31));
    EFGH_CHECK_ARG(nc >= 0 && nc < (1ll << 31) && (nc == 0 || (live_c && shadow_c)));
    EFGH_CHECK_ARG(aligned(live_f, shadow_f, 15) && aligned(live_c, shadow_c, 7));
    EFGH_CHECK_ARG(apart(live_f, shadow_f, 4ull * (uint64_t)nf) && (nc == 0 || apart(live_c, shadow_c, 8ull * (uint64_t)nc)));
    return EFGH_OK;
}

int copy_grid(int64_t nf, int64_t nc) { return grid_for(((nf >> 2) + 3 > nc ? (nf >> 2) + 3 : nc)); }
}  // namespace

extern "C" int efgh_txn_snapshot(const float *live_f, float *shadow_f, int64_t nf, const int64_t *live_c, int64_t *shadow_c,
                                 int64_t nc, efgh_txn_state *txn, void *stream) {
    if (int rc = check_vectors(live_f, shadow_f, nf, live_c, shadow_c, nc)) return rc;
    EFGH_CHECK_ARG(txn && (((uintptr_t)txn) & 7) == 0);
    k_txn_snapshot<<<copy_grid(nf, nc), TPB, 0, (hipStream_t)stream>>>(live_f, shadow_f, nf, (const long long *)live_c,
                                                                       (long long *)shadow_c, nc, txn);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_txn_probe(const float *live_f, const float *shadow_f, int64_t nf, const int64_t *starts, int32_t nseg,
                              const float *losses, int32_t k, int64_t loss_stride, efgh_txn_state *txn, void *stream) {
    EFGH_CHECK_ARG(live_f && shadow_f && starts && txn && nf >= 1 && nf < (1ll << 31) && nseg >= 1);
    EFGH_CHECK_ARG(k >= 0 && (k == 0 || (losses && loss_stride >= 1)));
    EFGH_CHECK_ARG(aligned(live_f, shadow_f, 15) && aligned(starts, txn, 7) && (((uintptr_t)losses) & 3) == 0);
    k_txn_probe<<<grid_for((nf >> 2) + 3), TPB, 0, (hipStream_t)stream>>>(live_f, shadow_f, nf, (const long long *)starts, nseg, losses,
                                                                          k, loss_stride, txn);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_txn_resolve(float *live_f, const float *shadow_f, int64_t nf, int64_t *live_c, const int64_t *shadow_c,
                                int64_t nc, efgh_guard_state *guard, efgh_txn_state *txn, float beta1, float beta2,
                                void *stream) {
    if (int rc = check_vectors(live_f, shadow_f, nf, live_c, shadow_c, nc)) return rc;
    EFGH_CHECK_ARG(guard && txn && aligned(guard, txn, 7));
    EFGH_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f);
    k_txn_resolve<<<copy_grid(nf, nc), TPB, 0, (hipStream_t)stream>>>(live_f, shadow_f, nf, (long long *)live_c,
                                                                      (const long long *)shadow_c, nc, guard, txn, beta1, beta2);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}
