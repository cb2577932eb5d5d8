// Exponential moving average of the flat weights (train.WeightEma), kept next to flat.w and updated by one launch behind Adam:
//   k_ema_update  e = fmaf(1 - d, w - e, e) in ONE pass over the flat buffer (12n bytes: reads w and e, writes e).  The decay d and
//                 the skip decision come from the guard's state block when there is one, so a skipped step leaves the average alone
//                 and the warm-up counts applied steps only - without a host read.
//   k_ema_swap    exchanges two flat buffers by bits (16n bytes): the averaged weights go under the model, and back.
// Launch shape of k_adam_flat (adam.hip): 256 threads, float4 grid-stride, at most 16384 workgroups, the n & 3 tail by workgroup 0.
// No atomics, no workspace, nothing outside [0, n) is touched.
#include <math.h>

#include "common.h"

namespace {
constexpr int TPB = 256;

static inline int ema_grid(long long n) {
    long long blocks = (n / 4 + 1 + TPB - 1) / TPB;         // the grid of efgh_adam_step
    return (int)(blocks > 16384 ? 16384 : (blocks < 1 ? 1 : blocks));
}

// torch.optim.swa_utils.get_ema_multi_avg_fn's lerp in the fused form: where w == e the value does not move (a -0 may become +0)
__device__ __forceinline__ float ema_one(float e, float w, float omd) { return fmaf(omd, w - e, e); }

__global__ void __launch_bounds__(TPB)
k_ema_update(float *__restrict__ ema, const float *__restrict__ w, long long n, float decay, int warmup, long long step,
             const efgh_guard_state *__restrict__ st) {
    long long t = step;
    if (st) {
        if (st->skip) return;
        t = st->applied;
    }
    // min(decay, (1 + t) / (10 + t)) in float64, rounded once
    const double ramp = warmup ? (1.0 + (double)t) / (10.0 + (double)t) : 1.0;
    const float d = (float)fmin((double)decay, ramp);
    const float omd = 1.f - d;
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n4; i += (long long)gridDim.x * TPB) {
        const float4 ww = reinterpret_cast<const float4 *>(w)[i];
        float4 ee = reinterpret_cast<float4 *>(ema)[i];
        ee.x = ema_one(ee.x, ww.x, omd); ee.y = ema_one(ee.y, ww.y, omd);
        ee.z = ema_one(ee.z, ww.z, omd); ee.w = ema_one(ee.w, ww.w, omd);
        reinterpret_cast<float4 *>(ema)[i] = ee;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long long i = (n4 << 2) + threadIdx.x;
        ema[i] = ema_one(ema[i], w[i], omd);
    }
}

// as 32-bit integers: no floating-point instruction sees the values, so NaN payloads and -0 survive
__global__ void __launch_bounds__(TPB)
k_ema_swap(unsigned int *__restrict__ a, unsigned int *__restrict__ b, long long n) {
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n4; i += (long long)gridDim.x * TPB) {
        const uint4 x = reinterpret_cast<uint4 *>(a)[i], y = reinterpret_cast<uint4 *>(b)[i];
        reinterpret_cast<uint4 *>(a)[i] = y;
        reinterpret_cast<uint4 *>(b)[i] = x;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long long i = (n4 << 2) + threadIdx.x;
        const unsigned int x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
}

static inline bool disjoint(const void *a, const void *b, int64_t n) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    const uint64_t bytes = 4ull * (uint64_t)n;
    return pa + bytes <= pb || pb + bytes <= pa;
}
}  // namespace

extern "C" int efgh_ema_update(float *ema, const float *w, int64_t n, float decay, int32_t warmup, int64_t step,
                               const efgh_guard_state *state, void *stream) {
    EFGH_CHECK_ARG(ema && w && n >= 1);
    EFGH_CHECK_ARG(((((uintptr_t)ema) | ((uintptr_t)w)) & 15) == 0 && (((uintptr_t)state) & 7) == 0);
    EFGH_CHECK_ARG(disjoint(ema, w, n));
    EFGH_CHECK_ARG(decay > 0.f && decay < 1.f);             // (false for a NaN)
    EFGH_CHECK_ARG(state || step >= 1);
    k_ema_update<<<ema_grid(n), TPB, 0, (hipStream_t)stream>>>(ema, w, n, decay, warmup ? 1 : 0, step, state);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_ema_swap(float *a, float *b, int64_t n, void *stream) {
    EFGH_CHECK_ARG(a && b && n >= 1);
    EFGH_CHECK_ARG(((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0);
    EFGH_CHECK_ARG(disjoint(a, b, n));
    k_ema_swap<<<ema_grid(n), TPB, 0, (hipStream_t)stream>>>((unsigned int *)a, (unsigned int *)b, n);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}
