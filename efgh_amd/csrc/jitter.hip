// Photometric jitter of the camera image in sample preparation: torchvision's ColorJitter on PIL images (brightness, contrast,
// saturation, hue, each once, in a drawn order), reproduced byte for byte.  The arithmetic is Pillow's (Blend.c, Convert.c's
// rgb2l / rgb2hsv / hsv2rgb, ImageStat's mean) and is spelled out in tests/jitter_contract.py; this file is built with
// -ffp-contract=off because Pillow's blend is a float32 multiply followed by a float32 add, and an FMA gives other bytes.
//
// Two launches whatever the ops: k_jitter_sum (only with contrast among them) leaves one integer partial sum of L per workgroup,
// k_jitter_apply folds them in every workgroup, forms the mean and runs the whole op list per pixel in registers.
// Two restatements of Pillow's hue arithmetic that give the same bits and are checked on all 2^24 triplets (tests/test_gpu_jitter.py):
// fmod(x, 1.0) as x - floor(x) for the x in [5/6, 11/6] that occur, and hsv2rgb's terms of H alone and of S alone from a 256-entry
// table a workgroup fills for itself.
#include "common.h"
#include <cmath>

namespace {
constexpr int TPB = 256;
constexpr int MAX_PARTIALS = 1024;        // grid cap of k_jitter_sum: what one workgroup of k_jitter_apply folds in four loads a thread
constexpr int MAX_OPS = EFGH_JITTER_MAX_OPS;

// how Pillow's blend treats a factor (decided on the float32 value, as Blend.c does)
enum { BLEND_DEG = 0, BLEND_IMG = 1, BLEND_TRUNC = 2, BLEND_CLIP = 3 };

struct Jitter {
    int n_ops;                 // ops run by the kernel: all of them (apply), those in front of contrast (sum)
    int op[MAX_OPS];           // EFGH_JITTER_*
    int mode[MAX_OPS];         // BLEND_*
    float f[MAX_OPS];
    int hue_k;                 // H' = (H + hue_k) & 255
};

struct Px { int r, g, b; };

__device__ __forceinline__ int luma(const Px &p) { return (19595 * p.r + 38470 * p.g + 7471 * p.b + 0x8000) >> 16; }

// Image.blend(deg, img, f) of one channel: t = deg + f * (img - deg), float32, multiply and add apart
__device__ __forceinline__ int blend1(int deg, int img, float f, int mode) {
    if (mode == BLEND_DEG) return deg;
    if (mode == BLEND_IMG) return img;
    const float d = (float)deg;
    const float prod = f * ((float)img - d);
    const float t = d + prod;
    if (mode == BLEND_TRUNC) return (int)t;                       // 0 <= f <= 1 keeps t inside [min, max] of the two
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ Px blend3(int deg, const Px &p, float f, int mode) {
    return {blend1(deg, p.r, f, mode), blend1(deg, p.g, f, mode), blend1(deg, p.b, f, mode)};
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// what hsv2rgb derives from H and from S alone, one entry per byte value: filled by the 256 threads of a workgroup when hue is among
// the ops, so the two float64 divisions and the floor are paid 256 times a workgroup and not once a pixel
struct HueLut { float f[256], fs[256]; unsigned char sextant[256]; };

__device__ __forceinline__ void fill_hue_lut(HueLut &lut) {
    const int b = threadIdx.x;                                   // TPB == 256
    const double h6 = (double)b * 6.0 / 255.0, fl = floor(h6);
    lut.f[b] = (float)(h6 - fl);
    lut.sextant[b] = (unsigned char)((int)fl % 6);
    lut.fs[b] = (float)((double)b / 255.0);
    __syncthreads();
}

// Convert.c:rgb2hsv_row, then the shift of H, then Convert.c:hsv2rgb
__device__ __forceinline__ Px hue_shift(const Px &p, int k, const HueLut &lut) {
    const int maxc = max(max(p.r, p.g), p.b), minc = min(min(p.r, p.g), p.b);
    if (maxc == minc) return p;                                  // H = S = 0, and S = 0 comes back as the gray V
    const int V = maxc;
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - p.r) / cr, gc = (float)(maxc - p.g) / cr, bc = (float)(maxc - p.b) / cr;
    float h;
    if (p.r == maxc) h = bc - gc;
    else if (p.g == maxc) h = (float)((2.0 + (double)rc) - (double)bc);
    else h = (float)((4.0 + (double)gc) - (double)rc);
    const double x = (double)h / 6.0 + 1.0;                      // in [5/6, 11/6]: fmod(x, 1.0) is x - floor(x), exactly
    h = (float)(x - floor(x));
    const int H = (clip8((int)((double)h * 255.0)) + k) & 255;
    const int S = clip8((int)((double)s * 255.0));
    if (S == 0) return {V, V, V};
    const float f = lut.f[H], fs = lut.fs[S];
    const double v = (double)V;
    const float fsf = fs * f, fsg = fs * (1.0f - f);             // float32 products; the rest of p, q, t is float64
    const int pp = clip8((int)round(v * (1.0 - (double)fs)));
    const int q = clip8((int)round(v * (1.0 - (double)fsf)));
    const int t = clip8((int)round(v * (1.0 - (double)fsg)));
    switch (lut.sextant[H]) {
    case 0: return {V, t, pp};
    case 1: return {q, V, pp};
    case 2: return {pp, V, t};
    case 3: return {pp, q, V};
    case 4: return {t, pp, V};
    default: return {V, pp, q};
    }
}

// the op list on N pixels, op by op; `mean` is contrast's gray level (unused by k_jitter_sum, which stops in front of contrast).  The
// branches are uniform over the launch: an op that is absent costs nothing
template <int N>
__device__ __forceinline__ void run_ops(const Jitter &j, Px (&p)[N], int mean, const HueLut &lut) {
    for (int i = 0; i < j.n_ops; ++i) {
        const float f = j.f[i];
        const int mode = j.mode[i];
        switch (j.op[i]) {
        case EFGH_JITTER_BRIGHTNESS:
#pragma unroll
            for (int k = 0; k < N; ++k) p[k] = blend3(0, p[k], f, mode);
            break;
        case EFGH_JITTER_CONTRAST:
#pragma unroll
            for (int k = 0; k < N; ++k) p[k] = blend3(mean, p[k], f, mode);
            break;
        case EFGH_JITTER_SATURATION:
#pragma unroll
            for (int k = 0; k < N; ++k) p[k] = blend3(luma(p[k]), p[k], f, mode);
            break;
        default:
#pragma unroll
            for (int k = 0; k < N; ++k) p[k] = hue_shift(p[k], j.hue_k, lut);
            break;
        }
    }
}

__device__ __forceinline__ bool has_hue(const Jitter &j) {
    bool h = false;
    for (int i = 0; i < j.n_ops; ++i) h |= j.op[i] == EFGH_JITTER_HUE;
    return h;
}

// four pixels = three dwords
__device__ __forceinline__ void unpack4(unsigned w0, unsigned w1, unsigned w2, Px (&p)[4]) {
    p[0] = {(int)(w0 & 255), (int)((w0 >> 8) & 255), (int)((w0 >> 16) & 255)};
    p[1] = {(int)(w0 >> 24), (int)(w1 & 255), (int)((w1 >> 8) & 255)};
    p[2] = {(int)((w1 >> 16) & 255), (int)(w1 >> 24), (int)(w2 & 255)};
    p[3] = {(int)((w2 >> 8) & 255), (int)((w2 >> 16) & 255), (int)(w2 >> 24)};
}

// block sum of one uint64 per thread, in every thread: shuffles inside the wave, the four wave sums through LDS
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v) {
    __shared__ unsigned long long wsum[TPB / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) t += wsum[w];
    return t;
}

// n4 groups of four pixels are read as dwords (0 when the image is not dword aligned), the pixels from 4 * n4 on one by one
__global__ void __launch_bounds__(TPB) k_jitter_sum(const uint8_t *__restrict__ in, long long n, long long n4, Jitter j,
                                                    unsigned long long *__restrict__ partial) {
    __shared__ HueLut lut;
    if (has_hue(j)) fill_hue_lut(lut);
    unsigned long long acc = 0;
    const long long t0 = (long long)blockIdx.x * TPB + threadIdx.x, step = (long long)gridDim.x * TPB;
    const unsigned *__restrict__ in32 = reinterpret_cast<const unsigned *>(in);
    for (long long g = t0; g < n4; g += step) {
        Px q[4];
        unpack4(in32[3 * g], in32[3 * g + 1], in32[3 * g + 2], q);
        run_ops(j, q, 0, lut);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += (unsigned)luma(q[k]);
    }
    for (long long i = 4 * n4 + t0; i < n; i += step) {
        Px p[1] = {{in[3 * i], in[3 * i + 1], in[3 * i + 2]}};
        run_ops(j, p, 0, lut);
        acc += (unsigned)luma(p[0]);
    }
    acc = block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(TPB) k_jitter_apply(const uint8_t *__restrict__ in, long long n, long long n4, Jitter j,
                                                      const unsigned long long *__restrict__ partial, int n_partial,
                                                      uint8_t *__restrict__ out) {
    __shared__ HueLut lut;
    if (has_hue(j)) fill_hue_lut(lut);
    int mean = 0;
    if (partial) {                        // int(sum / n + 0.5) with the quotient in float64, ImageStat.Stat(...).mean[0]
        unsigned long long s = 0;
        for (int k = threadIdx.x; k < n_partial; k += TPB) s += partial[k];
        s = block_sum(s);
        mean = (int)((double)s / (double)n + 0.5);
    }
    const long long t0 = (long long)blockIdx.x * TPB + threadIdx.x, step = (long long)gridDim.x * TPB;
    const unsigned *__restrict__ in32 = reinterpret_cast<const unsigned *>(in);
    unsigned *__restrict__ out32 = reinterpret_cast<unsigned *>(out);
    for (long long g = t0; g < n4; g += step) {
        Px q[4];
        unpack4(in32[3 * g], in32[3 * g + 1], in32[3 * g + 2], q);
        run_ops(j, q, mean, lut);
        out32[3 * g] = (unsigned)q[0].r | ((unsigned)q[0].g << 8) | ((unsigned)q[0].b << 16) | ((unsigned)q[1].r << 24);
        out32[3 * g + 1] = (unsigned)q[1].g | ((unsigned)q[1].b << 8) | ((unsigned)q[2].r << 16) | ((unsigned)q[2].g << 24);
        out32[3 * g + 2] = (unsigned)q[2].b | ((unsigned)q[3].r << 8) | ((unsigned)q[3].g << 16) | ((unsigned)q[3].b << 24);
    }
    for (long long i = 4 * n4 + t0; i < n; i += step) {
        Px p[1] = {{in[3 * i], in[3 * i + 1], in[3 * i + 2]}};
        run_ops(j, p, mean, lut);
        out[3 * i] = (uint8_t)p[0].r; out[3 * i + 1] = (uint8_t)p[0].g; out[3 * i + 2] = (uint8_t)p[0].b;
    }
}

int sum_blocks(long long n) {
    const long long g = (n + 4LL * TPB - 1) / (4LL * TPB);
    return (int)(g > MAX_PARTIALS ? MAX_PARTIALS : (g < 1 ? 1 : g));
}

// the shared argument contract: 1 .. 4 ops, each kind at most once, finite factors.  `upto_contrast`: keep the ops in front of
// contrast only (k_jitter_sum); EFGH_E_INVALID with a message otherwise.  *contrast_at = position of contrast or -1.
int make_jitter(const int32_t *ops, const float *factors, int32_t n_ops, int32_t hue_shift, bool upto_contrast, Jitter *j,
                int *contrast_at) {
    if (!ops || !factors || n_ops < 1 || n_ops > MAX_OPS) {
        efgh_set_error("jitter: %d ops (or null op / factor arrays), supported are 1 .. %d", (int)n_ops, MAX_OPS);
        return EFGH_E_INVALID;
    }
    unsigned seen = 0;
    *contrast_at = -1;
    *j = Jitter();
    for (int i = 0; i < n_ops; ++i) {
        if (ops[i] < 0 || ops[i] >= MAX_OPS || (seen >> ops[i] & 1u)) {
            efgh_set_error("jitter: op %d at position %d is unknown or appears twice", (int)ops[i], i);
            return EFGH_E_INVALID;
        }
        seen |= 1u << ops[i];
        const float f = factors[i];
        if (ops[i] != EFGH_JITTER_HUE && !std::isfinite(f)) {
            efgh_set_error("jitter: factor %g at position %d is not finite", (double)f, i);
            return EFGH_E_INVALID;
        }
        if (ops[i] == EFGH_JITTER_CONTRAST) *contrast_at = i;
        j->op[i] = ops[i];
        j->f[i] = f;
        j->mode[i] = f == 0.f ? BLEND_DEG : (f == 1.f ? BLEND_IMG : (f >= 0.f && f <= 1.f ? BLEND_TRUNC : BLEND_CLIP));
    }
    if (hue_shift < -255 || hue_shift > 255) {
        efgh_set_error("jitter: hue shift %d, supported are -255 .. 255", (int)hue_shift);
        return EFGH_E_INVALID;
    }
    j->hue_k = hue_shift;
    j->n_ops = upto_contrast ? (*contrast_at < 0 ? 0 : *contrast_at) : n_ops;
    return 0;
}

bool dword_aligned(const void *p) { return ((uintptr_t)p & 3u) == 0; }
} // namespace

extern "C" int32_t efgh_prep_jitter_partials(int64_t n_pixels) { return n_pixels < 1 ? 0 : sum_blocks(n_pixels); }

extern "C" int efgh_prep_jitter_sum(const uint8_t *in, int64_t n_pixels, const int32_t *ops_host, const float *factors_host,
                                    int32_t n_ops, int32_t hue_shift, void *partials, void *stream) {
    EFGH_CHECK_ARG(in && partials && n_pixels >= 1);
    EFGH_CHECK_ARG(((uintptr_t)partials & 7u) == 0);
    Jitter j;
    int contrast_at;
    const int rc = make_jitter(ops_host, factors_host, n_ops, hue_shift, true, &j, &contrast_at);
    if (rc) return rc;
    if (contrast_at < 0) {
        efgh_set_error("jitter: efgh_prep_jitter_sum without contrast among the ops");
        return EFGH_E_INVALID;
    }
    const long long n4 = dword_aligned(in) ? n_pixels / 4 : 0;
    k_jitter_sum<<<sum_blocks(n_pixels), TPB, 0, (hipStream_t)stream>>>(in, n_pixels, n4, j, (unsigned long long *)partials);
    EFGH_CHECK_LAUNCH();
    return 0;
}

extern "C" int efgh_prep_jitter_apply(const uint8_t *in, int64_t n_pixels, const int32_t *ops_host, const float *factors_host,
                                      int32_t n_ops, int32_t hue_shift, const void *partials, uint8_t *out, void *stream) {
    EFGH_CHECK_ARG(in && out && n_pixels >= 1);
    EFGH_CHECK_ARG((uintptr_t)out + 3 * n_pixels <= (uintptr_t)in || (uintptr_t)in + 3 * n_pixels <= (uintptr_t)out);         // never in place: the input is the caller's
    EFGH_CHECK_ARG(((uintptr_t)partials & 7u) == 0);
    Jitter j;
    int contrast_at;
    const int rc = make_jitter(ops_host, factors_host, n_ops, hue_shift, false, &j, &contrast_at);
    if (rc) return rc;
    if ((contrast_at >= 0) != (partials != nullptr)) {
        efgh_set_error("jitter: the partial sums of efgh_prep_jitter_sum are needed with contrast among the ops, and only then");
        return EFGH_E_INVALID;
    }
    const long long n4 = dword_aligned(in) && dword_aligned(out) ? n_pixels / 4 : 0;
    const long long items = n4 + (n_pixels - 4 * n4);
    const long long g = (items + TPB - 1) / TPB;
    k_jitter_apply<<<(int)(g > 65535 ? 65535 : g), TPB, 0, (hipStream_t)stream>>>(
        in, n_pixels, n4, j, (const unsigned long long *)partials, sum_blocks(n_pixels), out);
    EFGH_CHECK_LAUNCH();
    return 0;
}
