// Gradient accumulation over micro-batches (train.GradAccumulator / Trainer.step_accumulated):
//   k_grad_drain        acc = g (first micro-batch) or acc = acc + g, and g = 0, in ONE pass over the flat gradient: 12n / 16n bytes.
//                       One IEEE fp32 add per element, no scale (the 1 / (k * world) factor stays in the optimizer kernel), so the
//                       accumulator holds the bits of the sequential sum ((g1 + g2) + g3) + ...
//   k_gimg_valid_count  pixels with gdep4[..][3] > 0 && img_mask > 0 - the `valid` predicate of k_gimg_loss_fwd (loss.hip) - added
//                       to a 64-bit device counter: block reduction, one integer atomic per workgroup (integer sums do not depend
//                       on the arrival order; there is no floating-point atomic in this file)
#include "common.h"

namespace {
constexpr int TPB = 256;

static inline int grid_for(long long items) {
    long long b = (items + TPB - 1) / TPB;
    return (int)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}

// float4 over the aligned body [0, n & ~3), the n & 3 tail elements by the first threads of workgroup 0; 64-bit indices.
// FIRST: acc is never read (it may hold anything).  The zero written to g is +0.
template <bool FIRST, bool NT>
__global__ void __launch_bounds__(TPB)
k_grad_drain(float *__restrict__ acc, float *__restrict__ g, long long n) {
    const long long n4 = n >> 2;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n4; i += (long long)gridDim.x * TPB) {
        float4 x = ld_stream<NT>(g + 4 * i);
        if (!FIRST) {
            const float4 a = ld_stream<NT>(acc + 4 * i);
            x.x = a.x + x.x; x.y = a.y + x.y; x.z = a.z + x.z; x.w = a.w + x.w;
        }
        st_stream<NT>(acc + 4 * i, x);
        st_stream<NT>(g + 4 * i, zero);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long long i = (n4 << 2) + threadIdx.x;
        const float x = g[i];
        acc[i] = FIRST ? x : acc[i] + x;
        g[i] = 0.f;
    }
}

__global__ void __launch_bounds__(TPB)
k_gimg_valid_count(const float *__restrict__ gdep4, const uint8_t *__restrict__ img_mask, long long total,
                   unsigned long long *__restrict__ count) {
    int c = 0;                                      // (a thread sees at most total / TPB + 1 < 2^31 pixels for total < 2^39)
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB)
        c += (gdep4[i * 4 + 3] > 0.f && img_mask[i] > 0) ? 1 : 0;       // (a NaN depth compares false)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    __shared__ int sh[TPB / 64];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < TPB / 64; ++w) s += (unsigned long long)sh[w];
        if (s) atomicAdd(count, s);
    }
}
}  // namespace

extern "C" int efgh_grad_drain(float *acc, float *g, int64_t n, int32_t first, void *stream) {
    EFGH_CHECK_ARG(acc && g && acc != g && n >= 1);
    EFGH_CHECK_ARG(((((uintptr_t)acc) | ((uintptr_t)g)) & 15) == 0);
    // the two buffers must not overlap at all: an element zeroed through g would be lost from acc
    EFGH_CHECK_ARG((uintptr_t)acc + 4ull * (uint64_t)n <= (uintptr_t)g || (uintptr_t)g + 4ull * (uint64_t)n <= (uintptr_t)acc);
    const int grid = grid_for((n >> 2) > 0 ? (n >> 2) : 1);
    const bool nt = efgh_stream_nt(4ll * n);
    hipStream_t st = (hipStream_t)stream;
    if (first) {
        if (nt) k_grad_drain<true, true><<<grid, TPB, 0, st>>>(acc, g, n);
        else k_grad_drain<true, false><<<grid, TPB, 0, st>>>(acc, g, n);
    } else {
        if (nt) k_grad_drain<false, true><<<grid, TPB, 0, st>>>(acc, g, n);
        else k_grad_drain<false, false><<<grid, TPB, 0, st>>>(acc, g, n);
    }
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_gimg_valid_count(const float *gdep4, const uint8_t *img_mask, int32_t B, int64_t HW, int64_t *count,
                                     void *stream) {
    EFGH_CHECK_ARG(gdep4 && img_mask && count && B > 0 && HW > 0);
    EFGH_CHECK_ARG((int64_t)B * HW < (1ll << 39));
    EFGH_CHECK_ARG((((uintptr_t)count) & 7) == 0 && (((uintptr_t)gdep4) & 3) == 0);
    const long long total = (long long)B * HW;
    long long blocks = (total + 4 * TPB - 1) / (4 * TPB);           // ~4 pixels per thread, at most 2048 workgroups (and atomics)
    blocks = blocks > 2048 ? 2048 : (blocks < 1 ? 1 : blocks);
    k_gimg_valid_count<<<(int)blocks, TPB, 0, (hipStream_t)stream>>>(gdep4, img_mask, total, (unsigned long long *)count);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}
