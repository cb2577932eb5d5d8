// Fusing a registered LiDAR / camera pair ("Fusing a registered pair"): which pixel every point falls on, whether the camera
// sees it or a nearer surface hides it, and the colour it has there.  Three launches over one z-buffer of 64-bit keys:
//   k_fuse_zbuffer   one thread per point: atomicMin of (float32 depth bits << 32 | point index) over the point's window
//   k_fuse_resolve   one thread per four points: state, colour and pixel coordinates, read against the finished z-buffer
//   k_fuse_maps      one thread per pixel: the winner's depth and index as two images
// The key order is the depth order (depths are positive floats) with the lower index winning a tie, and an integer minimum does not
// depend on the order of its operands: the result is the same on every schedule.  The projection is float64 with every operation
// written out (tests/fuse_contract.py restates it in numpy), and this file is built with -ffp-contract=off so that none of them is
// fused: a multiply-add rounds once where the contract rounds twice.  The projection itself is in fuse_project.h.
#include "fuse_project.h"               // Hit, ST_*, project: shared with score.hip

namespace {
constexpr int TPB = 256;
constexpr unsigned long long EMPTY = ~0ull;
constexpr int MAX_RADIUS = 8;
#ifndef EFGH_FUSE_PEEK
#define EFGH_FUSE_PEEK 0
#endif

__global__ void __launch_bounds__(TPB)
k_fuse_zbuffer(const float *__restrict__ pc, long long bs, long long cs, int N, const double *__restrict__ P, int H, int W, int radius,
               double min_depth, unsigned long long *__restrict__ zbuf) {
    const int i = blockIdx.x * TPB + threadIdx.x, b = blockIdx.y;
    if (i >= N) return;
    const Hit h = project(pc + b * bs, cs, i, P + 12 * b, H, W, min_depth);
    if (h.state != ST_OCCLUDED) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(h.d) << 32) | (unsigned)i;
    unsigned long long *__restrict__ z = zbuf + (long long)b * H * W;
    const int r0 = max(h.r - radius, 0), r1 = min(h.r + radius, H - 1), c0 = max(h.c - radius, 0), c1 = min(h.c + radius, W - 1);
    // The atomics carry no return value: a thread's whole window issues back to back.  -DEFGH_FUSE_PEEK=1 (an experiment switch) puts
    // a plain load in front that skips the atomic when the slot already holds a smaller key (slots only ever decrease, so a stale
    // value decides nothing wrongly): the same bits, and several times the kernel time at radius 2, because every atomic then waits
    // for its load (profiles/fuse.txt)
    for (int r = r0; r <= r1; ++r)
        for (int c = c0; c <= c1; ++c) {
            unsigned long long *slot = z + (long long)r * W + c;
#if EFGH_FUSE_PEEK
            if (!(*slot > key)) continue;
#endif
            atomicMin(slot, key);
        }
}

struct Out { int state; unsigned r, g, b; float u, v; };

__device__ __forceinline__ unsigned lerp2(int a, int b, int c, int d, double tx, double ty) {
    const double top = (double)a + (double)(b - a) * tx;
    const double bot = (double)c + (double)(d - c) * tx;
    const double val = top + (bot - top) * ty;
    return (unsigned)(uint8_t)(int)(val + 0.5);
}

__device__ __forceinline__ Out resolve1(const float *__restrict__ pc, long long cs, int i, const double *__restrict__ T,
                                        const uint8_t *__restrict__ img, int H, int W, int bilinear, double min_depth, double rel_tol,
                                        double abs_tol, const unsigned long long *__restrict__ z) {
    const Hit h = project(pc, cs, i, T, H, W, min_depth);
    Out o;
    o.state = h.state; o.r = o.g = o.b = 0;
    const float nan = __uint_as_float(0x7fc00000u);
    o.u = h.state == ST_BEHIND ? nan : (float)h.u;
    o.v = h.state == ST_BEHIND ? nan : (float)h.v;
    if (h.state != ST_OCCLUDED) return o;
    const float zmin = __uint_as_float((unsigned)(z[(long long)h.r * W + h.c] >> 32));
    const double bound = (double)zmin * (1.0 + rel_tol) + abs_tol;
    if ((double)h.d <= bound) o.state = ST_VISIBLE;
    if (!bilinear) {
        const uint8_t *p = img + ((long long)h.r * W + h.c) * 3;
        o.r = p[0]; o.g = p[1]; o.b = p[2];
        return o;
    }
    const double fx = h.u - 0.5, fy = h.v - 0.5;
    const double x0 = floor(fx), y0 = floor(fy);
    const double tx = fx - x0, ty = fy - y0;
    const int xi = (int)x0, yi = (int)y0;
    const int xa = min(max(xi, 0), W - 1), xb = min(max(xi + 1, 0), W - 1);
    const int ya = min(max(yi, 0), H - 1), yb = min(max(yi + 1, 0), H - 1);
    const uint8_t *p00 = img + ((long long)ya * W + xa) * 3, *p01 = img + ((long long)ya * W + xb) * 3;
    const uint8_t *p10 = img + ((long long)yb * W + xa) * 3, *p11 = img + ((long long)yb * W + xb) * 3;
    o.r = lerp2(p00[0], p01[0], p10[0], p11[0], tx, ty);
    o.g = lerp2(p00[1], p01[1], p10[1], p11[1], tx, ty);
    o.b = lerp2(p00[2], p01[2], p10[2], p11[2], tx, ty);
    return o;
}

// one thread owns four consecutive points of a sample: rgb leaves as three dwords and state as one where the sample's rows start on
// a dword (`vec`: N a multiple of 4, or the first sample), byte by byte otherwise; the N & 3 points of the tail go one a thread
__global__ void __launch_bounds__(TPB)
k_fuse_resolve(const float *__restrict__ pc, long long bs, long long cs, int N, const double *__restrict__ P,
               const uint8_t *__restrict__ img, int H, int W, int bilinear, double min_depth, double rel_tol, double abs_tol,
               const unsigned long long *__restrict__ zbuf, uint8_t *__restrict__ state, uint8_t *__restrict__ rgb,
               float *__restrict__ uv) {
    const int b = blockIdx.y, n4 = N >> 2;
    const int t = blockIdx.x * TPB + threadIdx.x;
    const int items = n4 + (N & 3);
    if (t >= items) return;
    const float *__restrict__ pcb = pc + b * bs;
    const double *__restrict__ T = P + 12 * b;
    const uint8_t *__restrict__ imgb = img + (long long)b * H * W * 3;
    const unsigned long long *__restrict__ z = zbuf + (long long)b * H * W;
    uint8_t *__restrict__ sb = state + (long long)b * N;
    uint8_t *__restrict__ cb = rgb + (long long)b * N * 3;
    float2 *__restrict__ uvb = uv ? reinterpret_cast<float2 *>(uv) + (long long)b * N : nullptr;
    if (t < n4) {
        Out o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = resolve1(pcb, cs, 4 * t + k, T, imgb, H, W, bilinear, min_depth, rel_tol, abs_tol, z);
        const bool vec = (((uintptr_t)sb | (uintptr_t)cb) & 3u) == 0;
        if (vec) {
            reinterpret_cast<unsigned *>(sb)[t] = (unsigned)o[0].state | ((unsigned)o[1].state << 8) | ((unsigned)o[2].state << 16) |
                                                  ((unsigned)o[3].state << 24);
            unsigned *c32 = reinterpret_cast<unsigned *>(cb) + 3 * (long long)t;
            c32[0] = o[0].r | (o[0].g << 8) | (o[0].b << 16) | (o[1].r << 24);
            c32[1] = o[1].g | (o[1].b << 8) | (o[2].r << 16) | (o[2].g << 24);
            c32[2] = o[2].b | (o[3].r << 8) | (o[3].g << 16) | (o[3].b << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long i = 4 * (long long)t + k;
                sb[i] = (uint8_t)o[k].state;
                cb[3 * i] = (uint8_t)o[k].r; cb[3 * i + 1] = (uint8_t)o[k].g; cb[3 * i + 2] = (uint8_t)o[k].b;
            }
        }
        if (uvb) {
#pragma unroll
            for (int k = 0; k < 4; ++k) uvb[4 * (long long)t + k] = make_float2(o[k].u, o[k].v);
        }
    } else {
        const int i = 4 * n4 + (t - n4);
        const Out o = resolve1(pcb, cs, i, T, imgb, H, W, bilinear, min_depth, rel_tol, abs_tol, z);
        sb[i] = (uint8_t)o.state;
        cb[3 * (long long)i] = (uint8_t)o.r; cb[3 * (long long)i + 1] = (uint8_t)o.g; cb[3 * (long long)i + 2] = (uint8_t)o.b;
        if (uvb) uvb[i] = make_float2(o.u, o.v);
    }
}

__global__ void __launch_bounds__(TPB)
k_fuse_maps(const unsigned long long *__restrict__ zbuf, long long n, float *__restrict__ depth, int *__restrict__ index) {
    const long long p = (long long)blockIdx.x * TPB + threadIdx.x;
    if (p >= n) return;
    const unsigned long long key = zbuf[p];
    const bool empty = key == EMPTY;
    if (depth) depth[p] = empty ? 0.f : __uint_as_float((unsigned)(key >> 32));
    if (index) index[p] = empty ? -1 : (int)(unsigned)key;
}

#define FUSE_ARG(cond, ...)                                                          \
    do {                                                                             \
        if (!(cond)) {                                                               \
            efgh_set_error(__VA_ARGS__);                                             \
            return EFGH_E_INVALID;                                                   \
        }                                                                            \
    } while (0)

// the checks the two projecting entry points share
int check_common(const char *who, const void *pc, int B, int N, const void *P, int H, int W, double min_depth, const void *zbuf) {
    FUSE_ARG(pc && P && zbuf, "%s: null pointer (pc %p, P %p, zbuf %p)", who, pc, P, zbuf);
    FUSE_ARG(B > 0 && B <= 65535 && N > 0, "%s: B = %d (1 .. 65535) and N = %d must be positive", who, B, N);
    FUSE_ARG(H > 0 && W > 0 && (int64_t)H * W < 0x7fffffffLL, "%s: H = %d, W = %d: both positive and H*W < 2^31", who, H, W);
    FUSE_ARG(((uintptr_t)zbuf & 7u) == 0, "%s: zbuf is not 8-byte aligned", who);
    FUSE_ARG(min_depth >= 0.0 && std::isfinite(min_depth), "%s: min_depth = %g must be finite and >= 0", who, min_depth);
    return 0;
}
}  // namespace

extern "C" int64_t efgh_fuse_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (B < 1 || H < 1 || W < 1 || (int64_t)H * W >= 0x7fffffffLL) return -1;
    return 8 * (int64_t)B * H * W;
}

extern "C" int efgh_fuse_zbuffer(const float *pc, int64_t pc_bstride, int64_t pc_cstride, int32_t B, int32_t N, const double *P,
                                 int32_t H, int32_t W, int32_t radius, double min_depth, void *zbuf, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const int rc = check_common("efgh_fuse_zbuffer", pc, B, N, P, H, W, min_depth, zbuf);
    if (rc) return rc;
    FUSE_ARG(radius >= 0 && radius <= MAX_RADIUS, "efgh_fuse_zbuffer: radius = %d, supported are 0 .. %d", (int)radius, MAX_RADIUS);
    if (hipMemsetAsync(zbuf, 0xff, (size_t)8 * B * H * W, st) != hipSuccess) {
        efgh_set_error("efgh_fuse_zbuffer: memset failed");
        return EFGH_E_LAUNCH;
    }
    k_fuse_zbuffer<<<dim3(cdiv(N, TPB), B), TPB, 0, st>>>(pc, pc_bstride, pc_cstride, N, P, H, W, radius, min_depth,
                                                         (unsigned long long *)zbuf);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_fuse_resolve(const float *pc, int64_t pc_bstride, int64_t pc_cstride, int32_t B, int32_t N, const double *P,
                                 const uint8_t *img, int32_t H, int32_t W, int32_t bilinear, double min_depth, double rel_tol,
                                 double abs_tol, const void *zbuf, uint8_t *state, uint8_t *rgb, float *uv, void *stream) {
    const int rc = check_common("efgh_fuse_resolve", pc, B, N, P, H, W, min_depth, zbuf);
    if (rc) return rc;
    FUSE_ARG(img && state && rgb, "efgh_fuse_resolve: null pointer (img %p, state %p, rgb %p)", (const void *)img, (void *)state, (void *)rgb);
    FUSE_ARG(bilinear == 0 || bilinear == 1, "efgh_fuse_resolve: bilinear = %d must be 0 or 1", (int)bilinear);
    FUSE_ARG(rel_tol >= 0.0 && std::isfinite(rel_tol), "efgh_fuse_resolve: rel_tol = %g must be finite and >= 0", rel_tol);
    FUSE_ARG(abs_tol >= 0.0 && std::isfinite(abs_tol), "efgh_fuse_resolve: abs_tol = %g must be finite and >= 0", abs_tol);
    FUSE_ARG(((uintptr_t)uv & 7u) == 0, "efgh_fuse_resolve: uv is not 8-byte aligned");
    const int items = (N >> 2) + (N & 3);
    k_fuse_resolve<<<dim3(cdiv(items, TPB), B), TPB, 0, (hipStream_t)stream>>>(
        pc, pc_bstride, pc_cstride, N, P, img, H, W, bilinear, min_depth, rel_tol, abs_tol, (const unsigned long long *)zbuf, state, rgb,
        uv);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_fuse_maps(const void *zbuf, int32_t B, int64_t HW, float *depth, int32_t *index, void *stream) {
    FUSE_ARG(zbuf && ((uintptr_t)zbuf & 7u) == 0, "efgh_fuse_maps: zbuf is null or not 8-byte aligned");
    FUSE_ARG(B > 0 && HW > 0 && HW < 0x7fffffffLL, "efgh_fuse_maps: B = %d and HW = %lld: both positive and HW < 2^31", (int)B, (long long)HW);
    FUSE_ARG(depth || index, "efgh_fuse_maps: neither a depth nor an index map was asked for");
    const long long n = (long long)B * HW;
    FUSE_ARG(n <= 0x7fffffffLL * TPB, "efgh_fuse_maps: B*HW = %lld pixels are more than one launch covers", n);
    k_fuse_maps<<<cdiv(n, TPB), TPB, 0, (hipStream_t)stream>>>((const unsigned long long *)zbuf, n, depth, index);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}
