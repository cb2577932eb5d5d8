// Fused Adam over one flat parameter buffer whose elements belong to parameter groups (torch.optim's param_groups: a learning rate,
// a weight decay and the coupled / decoupled choice per group; betas, eps, the step count and the gradient scale are shared).
// One launch, HBM-bound (28 bytes per element) like k_adam (elementwise.hip) and k_adam_guarded (guard.hip), whose expressions the
// element update repeats, expression for expression: a segment of a coupled group gets the bits those kernels leave when run on the
// segment alone with the group's values; a decoupled group (AdamW) first multiplies the weight by decay = 1 - lr * weight_decay
// (one fp32 product, torch.optim.AdamW's param.mul_) and then takes the same expressions with weight_decay = 0.
//
// The segment table (ascending ends + one group id per segment) lives in device memory.  Every float4 of the flat buffers lies wholly
// inside [0, n) whatever the cuts, so all accesses stay 16-byte vectors except the n & 3 tail; a float4 that straddles a segment end
// only selects other per-group values per lane.  A workgroup finds the segment of its sweep's first element with one uniform binary
// search (continued from the previous sweep's); a sweep that lies inside one segment - nearly all of them: 353 tensors in 47.8 M
// elements - uses that segment's values for every lane, otherwise a thread searches the at most 4 * threadIdx.x + 1 table entries
// its own float4 can lie in.  The per-group values are staged in LDS once per workgroup.
#include <math.h>

#include "common.h"

namespace {
constexpr int ATPB = 256;
constexpr int MAXG = EFGH_ADAM_MAX_GROUPS;

struct GroupLds {
    float lrb[MAXG];      // lr / bc1
    float wd[MAXG];       // weight decay of the coupled form (0 for a decoupled group)
    float dec[MAXG];      // decay factor of the decoupled form
    int dcp[MAXG];
};

// One element with its group's values (lrb = lr / bc1).  The arithmetic is WRITTEN OUT - fused multiply-adds as fmaf, everything else
// under contract(off) - as hipcc compiles k_adam and k_adam_guarded (read off their ISA; both kernels agree):
//   float4 body   gr = fma(g, gscale, wd * w), m = fma(b1, m, (1 - b1) * gr), v = fma(b2, v, ((1 - b2) * gr) * gr),
//                 w = fma(-(lr / bc1), m / (sqrt(v) / bc2_sqrt + eps), w)
//   n & 3 tail    the same, except that m and v are a product and a sum, rounded twice (the vectoriser pairs those two sums with
//                 other work before they can be contracted)
// `tail`: the element is one of the last (length & 3) of its segment, i.e. those kernels, run on the segment alone, would update it
// in their tail - so that a segment holds their bits whatever its length and wherever it starts.
template <bool BODY_ONLY = false>
__device__ __forceinline__ void adam_elem(float &w, float g, float &m, float &v, float lrb, float wd, float dec, int dcp, bool tail,
                                          float b1, float b2, float eps, float bc2_sqrt, float gscale) {
#pragma clang fp contract(off)
    const float wq = dcp ? w * dec : w;           // decoupled: a product of its own (torch.optim.AdamW's param.mul_)
    const float gr = fmaf(g, gscale, wd * wq);
    const float a = (1.f - b1) * gr, c = ((1.f - b2) * gr) * gr;
    const float m_fused = fmaf(b1, m, a), v_fused = fmaf(b2, v, c);
    if (BODY_ONLY) {                              // (no element of the sweep is in its segment's tail)
        m = m_fused;
        v = v_fused;
    } else {
        const float m_plain = b1 * m + a, v_plain = b2 * v + c;
        m = tail ? m_plain : m_fused;
        v = tail ? v_plain : v_fused;
    }
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    w = fmaf(-lrb, m / denom, wq);
}

// first element of segment s's tail: the last (length & 3) elements
__device__ __forceinline__ long long tail_start(long long start, long long end) { return end - ((end - start) & 3); }

// smallest s in [lo, hi] with ends[s] > e (ends ascending, ends[hi] > e)
__device__ __forceinline__ int seg_of(const long long *__restrict__ ends, int lo, int hi, long long e) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ends[mid] > e) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ void __launch_bounds__(ATPB)
k_adam_groups(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, long long n,
              const long long *__restrict__ ends, const unsigned char *__restrict__ gid, int nseg, efgh_adam_groups hp,
              float host_bc1, float host_bc2_sqrt, const efgh_guard_state *__restrict__ st) {
    __shared__ GroupLds sh;
    if (st && st->skip) return;
    const float bc1 = st ? st->bc1 : host_bc1, bc2_sqrt = st ? st->bc2_sqrt : host_bc2_sqrt;
    const float gscale = st ? st->scale : hp.grad_scale;
    const float b1 = hp.beta1, b2 = hp.beta2, eps = hp.eps;
    if (threadIdx.x < MAXG) {
        float lr = 0.f, wd = 0.f, dec = 1.f;
        int dcp = 0;
#pragma unroll
        for (int k = 0; k < MAXG; ++k)
            if (k == (int)threadIdx.x) { lr = hp.lr[k]; wd = hp.weight_decay[k]; dec = hp.decay[k]; dcp = hp.decoupled[k]; }
        sh.lrb[threadIdx.x] = lr / bc1;
        sh.wd[threadIdx.x] = dcp ? 0.f : wd;
        sh.dec[threadIdx.x] = dec;
        sh.dcp[threadIdx.x] = dcp;
    }
    __syncthreads();
    const long long n4 = n >> 2;
    int s0 = 0;
    for (long long base = (long long)blockIdx.x * ATPB; base < n4; base += (long long)gridDim.x * ATPB) {      // (uniform)
        // the loads do not depend on the table: issue them first, the search below runs while they are in flight
        const long long i = base + threadIdx.x;
        const bool act = i < n4;
        float4 ww, gg, mm, vv;
        if (act) {
            ww = reinterpret_cast<float4 *>(w)[i]; gg = reinterpret_cast<const float4 *>(g)[i];
            mm = reinterpret_cast<float4 *>(m)[i]; vv = reinterpret_cast<float4 *>(v)[i];
        }
        const long long first = base << 2;
        const long long last = ((base + ATPB < n4 ? base + ATPB : n4) << 2) - 1;
        if (ends[s0] <= first) s0 = seg_of(ends, s0 + 1, nseg - 1, first);       // (else: still the previous sweep's segment)
        const bool one = ends[s0] > last;                    // the whole sweep lies in segment s0
        if (!act) continue;
        float *wp = &ww.x, *gp = &gg.x, *mp = &mm.x, *vp = &vv.x;
        const long long e0 = i << 2;
        if (one) {
            const int k = gid[s0] & (MAXG - 1);
            const float lrb = sh.lrb[k], wd = sh.wd[k], dec = sh.dec[k];
            const int dcp = sh.dcp[k];
            const long long ts = tail_start(s0 > 0 ? ends[s0 - 1] : 0, ends[s0]);
            if (ts > last) {                                 // (uniform) the common sweep: k_adam's float4 body, nothing else
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    adam_elem<true>(wp[q], gp[q], mp[q], vp[q], lrb, wd, dec, dcp, false, b1, b2, eps, bc2_sqrt, gscale);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    adam_elem(wp[q], gp[q], mp[q], vp[q], lrb, wd, dec, dcp, e0 + q >= ts, b1, b2, eps, bc2_sqrt, gscale);
            }
        } else {
            // segments are not empty: element first + j lies in a segment <= s0 + j
            long long hi = (long long)s0 + 4 * (long long)threadIdx.x;
            int s = seg_of(ends, s0, hi < nseg - 1 ? (int)hi : nseg - 1, e0);
            long long start = s > 0 ? ends[s - 1] : 0, end = ends[s];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                while (end <= e0 + q && s < nseg - 1) { start = end; end = ends[++s]; }      // (e0 + q < n = ends[nseg - 1])
                const int k = gid[s] & (MAXG - 1);
                adam_elem(wp[q], gp[q], mp[q], vp[q], sh.lrb[k], sh.wd[k], sh.dec[k], sh.dcp[k], e0 + q >= tail_start(start, end),
                          b1, b2, eps, bc2_sqrt, gscale);
            }
        }
        reinterpret_cast<float4 *>(w)[i] = ww;
        reinterpret_cast<float4 *>(m)[i] = mm;
        reinterpret_cast<float4 *>(v)[i] = vv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long long i = (n4 << 2) + threadIdx.x;
        const int sg = seg_of(ends, 0, nseg - 1, i);
        const int k = gid[sg] & (MAXG - 1);
        adam_elem(w[i], g[i], m[i], v[i], sh.lrb[k], sh.wd[k], sh.dec[k], sh.dcp[k], i >= tail_start(sg > 0 ? ends[sg - 1] : 0, ends[sg]),
                  b1, b2, eps, bc2_sqrt, gscale);
    }
}
}  // namespace

extern "C" int efgh_adam_step_groups(float *w, const float *g, float *m, float *v, int64_t n, const int64_t *seg_ends,
                                     const uint8_t *seg_group, int32_t nseg, const int64_t *host_ends, const uint8_t *host_group,
                                     const efgh_adam_groups *groups, const efgh_guard_state *state, int32_t grid, void *stream) {
    EFGH_CHECK_ARG(w && g && m && v && seg_ends && seg_group && host_ends && host_group && groups && n > 0);
    EFGH_CHECK_ARG(((((uintptr_t)w) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0);
    EFGH_CHECK_ARG(((((uintptr_t)seg_ends) | ((uintptr_t)state)) & 7) == 0);
    EFGH_CHECK_ARG(nseg >= 1 && nseg <= EFGH_ADAM_MAX_SEGMENTS);
    EFGH_CHECK_ARG(groups->n_groups >= 1 && groups->n_groups <= EFGH_ADAM_MAX_GROUPS);
    EFGH_CHECK_ARG(grid >= 0);
    EFGH_CHECK_ARG(state || groups->step >= 1);
    EFGH_CHECK_ARG(host_ends[0] > 0 && host_ends[nseg - 1] == n);
    for (int s = 0; s < nseg; ++s) {
        EFGH_CHECK_ARG(s == 0 || host_ends[s - 1] < host_ends[s]);                  // ascending, no empty segment
        EFGH_CHECK_ARG(host_group[s] < groups->n_groups);
    }
    for (int k = 0; k < groups->n_groups; ++k) {
        EFGH_CHECK_ARG(groups->lr[k] >= 0.f && isfinite(groups->lr[k]));
        EFGH_CHECK_ARG(groups->weight_decay[k] >= 0.f && isfinite(groups->weight_decay[k]));
        EFGH_CHECK_ARG(!groups->decoupled[k] || isfinite(groups->decay[k]));
    }
    float bc1 = 0.f, bc2_sqrt = 0.f;
    if (!state) {                                   // as efgh_adam_step computes them
        bc1 = 1.f - powf(groups->beta1, (float)groups->step);
        bc2_sqrt = sqrtf(1.f - powf(groups->beta2, (float)groups->step));
    }
    long long blocks = (n / 4 + 1 + 255) / 256;     // the grid of efgh_adam_step
    blocks = blocks > 16384 ? 16384 : (blocks < 1 ? 1 : blocks);
    if (grid > 0) blocks = grid;
    k_adam_groups<<<(int)blocks, ATPB, 0, (hipStream_t)stream>>>(w, g, m, v, n, (const long long *)seg_ends, seg_group, nseg, *groups,
                                                                bc1, bc2_sqrt, state);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}
