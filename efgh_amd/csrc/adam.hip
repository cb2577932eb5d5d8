// Fused Adam over one flat fp32 parameter buffer (torch.optim.Adam semantics, main.py:181-183): ONE written-out element update,
// adam_elem, and the three kernels that apply it - all HBM-bound, 28 bytes per element, 256 threads, float4 grid-stride, at most
// 16384 workgroups, the n & 3 tail by workgroup 0:
//   k_adam_flat<false>  efgh_adam_step          one learning rate and weight decay; scale and bias corrections passed by value
//   k_adam_flat<true>   efgh_adam_step_guarded  the same with scale, bias corrections and skip flag read from the guard's state block
//   k_adam_groups       efgh_adam_step_groups   every element takes the values of its parameter group (torch.optim's param_groups: a
//                                               learning rate, a weight decay and the coupled / decoupled choice per group; betas,
//                                               eps, the step count and the gradient scale are shared), with or without a state block
// A segment of a coupled group gets the bits the flat kernels leave when run on the segment alone with the group's values; a
// decoupled group (AdamW) first multiplies the weight by decay = 1 - lr * weight_decay (one fp32 product, torch.optim.AdamW's
// param.mul_) and then takes the same update with weight_decay = 0.
//
// The grouped kernel's segment table (ascending ends + one group id per segment) lives in device memory.  Every float4 of the flat
// buffers lies wholly inside [0, n) whatever the cuts, so all accesses stay 16-byte vectors except the n & 3 tail; a float4 that
// straddles a segment end only selects other per-group values per lane.  A workgroup finds the segment of its sweep's first element
// with one uniform binary search (continued from the previous sweep's); a sweep that lies inside one segment - nearly all of them:
// 353 tensors in 47.8 M elements - uses that segment's values for every lane, otherwise a thread searches the at most
// 4 * threadIdx.x + 1 table entries its own float4 can lie in.  The per-group values are staged in LDS once per workgroup.
#include "common.h"

namespace {
constexpr int ATPB = 256;
constexpr int MAXG = EFGH_ADAM_MAX_GROUPS;

// Adam's update of one element (lrb = lr / bc1, formed once per thread or group).  This is the DEFINITION, and the only place the
// library spells it: fused multiply-adds are fmaf, everything else is rounded where it is written (contract(off)).
//   gr = fma(g, gscale, wd * w)
//   body (BODY_ONLY, or !tail)   m = fma(b1, m, (1 - b1) * gr)       v = fma(b2, v, ((1 - b2) * gr) * gr)
//   tail                         m = b1 * m + (1 - b1) * gr          v = b2 * v + ((1 - b2) * gr) * gr       (a product and a sum)
//   w = fma(-lrb, m / (sqrt(v) / bc2_sqrt + eps), w)
// `tail`: the element is one of the last (length & 3) of its buffer or segment - the elements a flat launch over that range alone
// updates outside its float4 body - so that a segment holds the flat kernels' bits whatever its length and wherever it starts.
// The two forms are kept because every checkpoint written so far holds them (tests/test_gpu_adam_bits.py).
template <bool BODY_ONLY = false>
__device__ __forceinline__ void adam_elem(float &w, float g, float &m, float &v, float lrb, float wd, float dec, int dcp, bool tail,
                                          float b1, float b2, float eps, float bc2_sqrt, float gscale) {
#pragma clang fp contract(off)
    const float wq = dcp ? w * dec : w;           // decoupled: a product of its own (torch.optim.AdamW's param.mul_)
    const float gr = fmaf(g, gscale, wd * wq);
    const float a = (1.f - b1) * gr, c = ((1.f - b2) * gr) * gr;
    const float m_fused = fmaf(b1, m, a), v_fused = fmaf(b2, v, c);
    if (BODY_ONLY) {                              // (no element of the sweep is in a tail)
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

// GUARDED: gscale, bc1, bc2_sqrt and the skip flag come from the state block, else from the arguments
template <bool GUARDED>
__global__ void __launch_bounds__(ATPB)
k_adam_flat(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, long long n, float lr,
            float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale, const efgh_guard_state *__restrict__ st) {
    if (GUARDED) {
        if (st->skip) return;
        bc1 = st->bc1; bc2_sqrt = st->bc2_sqrt; gscale = st->scale;
    }
    const float lrb = lr / bc1;
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * ATPB + threadIdx.x; i < n4; i += (long long)gridDim.x * ATPB) {
        float4 ww = reinterpret_cast<float4 *>(w)[i], gg = reinterpret_cast<const float4 *>(g)[i];
        float4 mm = reinterpret_cast<float4 *>(m)[i], vv = reinterpret_cast<float4 *>(v)[i];
        float *wp = &ww.x, *gp = &gg.x, *mp = &mm.x, *vp = &vv.x;
#pragma unroll
        for (int q = 0; q < 4; ++q) adam_elem<true>(wp[q], gp[q], mp[q], vp[q], lrb, wd, 1.f, 0, false, b1, b2, eps, bc2_sqrt, gscale);
        reinterpret_cast<float4 *>(w)[i] = ww;
        reinterpret_cast<float4 *>(m)[i] = mm;
        reinterpret_cast<float4 *>(v)[i] = vv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long long i = (n4 << 2) + threadIdx.x;
        adam_elem(w[i], g[i], m[i], v[i], lrb, wd, 1.f, 0, true, b1, b2, eps, bc2_sqrt, gscale);
    }
}

struct GroupLds {
    float lrb[MAXG];      // lr / bc1
    float wd[MAXG];       // weight decay of the coupled form (0 for a decoupled group)
    float dec[MAXG];      // decay factor of the decoupled form
    int dcp[MAXG];
};

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
            if (ts > last) {                                 // (uniform) the common sweep: the flat kernels' float4 body, nothing else
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

// ---- host side, shared by the three entry points ----
// the flat buffers are read as float4: all there, not empty, 16-byte aligned
bool buffers_ok(const float *w, const float *g, const float *m, const float *v, int64_t n) {
    return w && g && m && v && n > 0 && ((((uintptr_t)w) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;
}

// one thread per float4, and one more for the n & 3 tail; the grid-stride loops take the rest beyond 16384 workgroups
int adam_grid(int64_t n) {
    const long long blocks = (n / 4 + 1 + ATPB - 1) / ATPB;
    return (int)(blocks > 16384 ? 16384 : blocks);
}
}  // namespace

extern "C" int efgh_adam_step(float *w, const float *g, float *m, float *v, int64_t n, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int32_t step, float grad_scale,
                              void *stream) {
    EFGH_CHECK_ARG(buffers_ok(w, g, m, v, n) && step >= 1);
    const efgh_bias_corr bc = efgh_bias_corrections(beta1, beta2, step);
    k_adam_flat<false><<<adam_grid(n), ATPB, 0, (hipStream_t)stream>>>(w, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bc.bc1,
                                                                      bc.bc2_sqrt, grad_scale, nullptr);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_adam_step_guarded(float *w, const float *g, float *m, float *v, int64_t n, float lr, float beta1,
                                      float beta2, float eps, float weight_decay, const efgh_guard_state *state,
                                      void *stream) {
    EFGH_CHECK_ARG(buffers_ok(w, g, m, v, n) && state && (((uintptr_t)state) & 7) == 0);
    k_adam_flat<true><<<adam_grid(n), ATPB, 0, (hipStream_t)stream>>>(w, g, m, v, n, lr, beta1, beta2, eps, weight_decay, 0.f, 0.f, 0.f,
                                                                     state);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_adam_step_groups(float *w, const float *g, float *m, float *v, int64_t n, const int64_t *seg_ends,
                                     const uint8_t *seg_group, int32_t nseg, const int64_t *host_ends, const uint8_t *host_group,
                                     const efgh_adam_groups *groups, const efgh_guard_state *state, int32_t grid, void *stream) {
    EFGH_CHECK_ARG(buffers_ok(w, g, m, v, n) && seg_ends && seg_group && host_ends && host_group && groups);
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
    efgh_bias_corr bc = {0.f, 0.f};
    if (!state) bc = efgh_bias_corrections(groups->beta1, groups->beta2, groups->step);
    k_adam_groups<<<grid > 0 ? grid : adam_grid(n), ATPB, 0, (hipStream_t)stream>>>(w, g, m, v, n, (const long long *)seg_ends, seg_group,
                                                                                  nseg, *groups, bc.bc1, bc.bc2_sqrt, state);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}
