// GPU-side sample preparation: the per-sample CPU transforms of the reference's loaders
// (`data_loader/loader_utils.py:104-202`: Pillow rotate(expand)/crop/bicubic resize/pad/valid-mask of the camera image,
// radius filter + sub-sampling + random mis-calibration of the sweep) as HBM-bound byte/integer kernels.
// The O(1) geometry (rotation matrix -> 16.16 fixed-point affine coefficients, resample coefficient tables, crop
// offsets) is computed on the host exactly as Pillow / numpy_utils.py do (efgh_amd/data/prepare.py) and handed in.
#include "common.h"
#include <limits.h>

namespace {
constexpr int TPB = 256;

int grid_for(long long total) {
    long long g = (total + TPB - 1) / TPB;
    return (int)(g > 65535 ? 65535 : (g < 1 ? 1 : g));
}

// Image.rotate / ImagingTransformAffine nearest, Geometry.c:affine_fixed:
//   xin = (a2 + a0*x + a1*y) >> 16, yin = (a5 + a3*x + a4*y) >> 16, zero fill outside the source
__global__ void k_affine_nearest_u8(const uint8_t *__restrict__ in, int h, int w, long long a0, long long a1,
                                    long long a2, long long a3, long long a4, long long a5,
                                    uint8_t *__restrict__ out, int nh, int nw) {
    const long long total = (long long)nh * nw;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const int x = (int)(i % nw), y = (int)(i / nw);
        const long long xin = (a2 + a0 * x + a1 * y) >> 16, yin = (a5 + a3 * x + a4 * y) >> 16;
        uint8_t r = 0, g = 0, b = 0;
        if (xin >= 0 && xin < w && yin >= 0 && yin < h) {
            const uint8_t *s = in + (yin * w + xin) * 3;
            r = s[0]; g = s[1]; b = s[2];
        }
        uint8_t *d = out + i * 3;
        d[0] = r; d[1] = g; d[2] = b;
    }
}

// zero_pad_image + crop_image (numpy_utils.py:447-503) as one gather: out[y][x] = in[y+oy][x+ox] or 0
__global__ void k_crop_pad_u8(const uint8_t *__restrict__ in, int h, int w, int oy, int ox,
                              uint8_t *__restrict__ out, int th, int tw) {
    const long long total = (long long)th * tw;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const int x = (int)(i % tw) + ox, y = (int)(i / tw) + oy;
        uint8_t r = 0, g = 0, b = 0;
        if (x >= 0 && x < w && y >= 0 && y < h) {
            const uint8_t *s = in + ((long long)y * w + x) * 3;
            r = s[0]; g = s[1]; b = s[2];
        }
        uint8_t *d = out + i * 3;
        d[0] = r; d[1] = g; d[2] = b;
    }
}

// One pass of Pillow's 8-bit resampling (Resample.c:ImagingResampleHorizontal_8bpc / Vertical_8bpc):
//   out = clip8((2^21 + sum_k in[first + k] * coeff[k]) >> 22) along `axis` (1 = x, 0 = y)
__global__ void k_resample_u8(const uint8_t *__restrict__ in, int h, int w, int axis, int out_size,
                              const int *__restrict__ bounds, const int *__restrict__ coeffs, int ksize,
                              uint8_t *__restrict__ out) {
    const int oh = axis ? h : out_size, ow = axis ? out_size : w;
    const long long total = (long long)oh * ow;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const int x = (int)(i % ow), y = (int)(i / ow);
        const int o = axis ? x : y;
        const int first = bounds[2 * o], n = bounds[2 * o + 1];
        const int *k = coeffs + (long long)o * ksize;
        int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
        const long long step = axis ? 3 : (long long)w * 3;
        const uint8_t *p = in + (axis ? ((long long)y * w + first) * 3 : ((long long)first * w + x) * 3);
        for (int q = 0; q < n; ++q, p += step) {
            const int c = k[q];
            s0 += (int)p[0] * c; s1 += (int)p[1] * c; s2 += (int)p[2] * c;
        }
        s0 >>= 22; s1 >>= 22; s2 >>= 22;
        uint8_t *d = out + i * 3;
        d[0] = (uint8_t)(s0 < 0 ? 0 : (s0 > 255 ? 255 : s0));
        d[1] = (uint8_t)(s1 < 0 ? 0 : (s1 > 255 ? 255 : s1));
        d[2] = (uint8_t)(s2 < 0 ? 0 : (s2 > 255 ? 255 : s2));
    }
}

// (H,W,3) u8 -> (3,H,W) u8 and the valid mask (1,H,W): 0 where all three channels are 0 (numpy_utils.py:505-517)
__global__ void k_hwc_to_chw_u8(const uint8_t *__restrict__ in, long long hw, uint8_t *__restrict__ chw,
                                uint8_t *__restrict__ mask) {
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < hw; i += (long long)gridDim.x * TPB) {
        const uint8_t r = in[i * 3], g = in[i * 3 + 1], b = in[i * 3 + 2];
        if (chw) { chw[i] = r; chw[hw + i] = g; chw[2 * hw + i] = b; }
        if (mask) mask[i] = (r | g | b) ? 1 : 0;
    }
}

// network input: zero_pad_image to (th,tw) + uint8 -> float32, CHW (loader_utils.py:110-114)
__global__ void k_u8_to_f32_chw_pad(const uint8_t *__restrict__ in, int h, int w, int oy, int ox,
                                    float *__restrict__ out, int th, int tw) {
    const long long total = (long long)th * tw;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const int x = (int)(i % tw) - ox, y = (int)(i / tw) - oy;
        float r = 0.f, g = 0.f, b = 0.f;
        if (x >= 0 && x < w && y >= 0 && y < h) {
            const uint8_t *s = in + ((long long)y * w + x) * 3;
            r = (float)s[0]; g = (float)s[1]; b = (float)s[2];
        }
        out[i] = r; out[total + i] = g; out[2 * total + i] = b;
    }
}

// ---- point rows: K packed float32 sweeps, each with its own float64 [3][4] transform into the frame of sweep 0 ---------------------
// (get_accumulated_pc / search_for_accumulation, kitti_odom_loader.py:160-225, rellis3d_loader.py:218-280;
// accumulate_lidar_points / lidar_frame_accumulation, nusc_loader.py:83-146).  The accumulated float64 cloud is never
// written: the point kernels index the concatenation 0 .. n_total-1 and compute q = M_k . (p, 1) where they need it.
// A plain array of rows (the entry points without `sweeps` in their name) is the same struct with K = 0 and no offsets, matrices
// or flags: the kernels take it as SWEEPS = false and touch none of the three.
constexpr int SWEEPS_MAX = 64;

struct SweepSet {
    const float *pts;          // packed rows, `stride` (3 or 4) floats each
    const int *off;            // [K+1] first row of each sweep, off[K] = n_total
    const double *M;           // [K][3][4]
    const int *ident;          // [K] != 0: the sweep passes through untouched (q = (double)p, no arithmetic)
    int K, stride, n_total;    // n_total: the rows an index is checked against (INT_MAX where the entry point is told no row count)
};

// offsets -> LDS, one block-wide load and a barrier; nothing at all for plain rows
template <bool SWEEPS>
__device__ __forceinline__ void stage_offsets(const SweepSet &s, int *lds_off) {
    if (!SWEEPS) return;
    for (int k = threadIdx.x; k <= s.K; k += TPB) lds_off[k] = s.off[k];
    __syncthreads();
}

// the sweep k with off[k] <= i < off[k+1] (empty sweeps have off[k] == off[k+1] and are never returned)
__device__ __forceinline__ int sweep_of(const int *lds_off, int K, int i) {
    int lo = 0, hi = K;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (lds_off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

struct Raw3 { float x, y, z; };

__device__ __forceinline__ Raw3 load_raw(const SweepSet &s, int i) {
    if (s.stride == 4) {
        const float4 v = *reinterpret_cast<const float4 *>(s.pts + 4LL * i);
        return {v.x, v.y, v.z};
    }
    const float *p = s.pts + 3LL * i;
    return {p[0], p[1], p[2]};
}

// q = M_k . (p, 1) in float64, the four terms summed left to right (numpy's product goes through BLAS, which fixes neither
// the order nor the use of FMA: tests/sweeps_contract.py carries the bound that covers every evaluation)
__device__ __forceinline__ void sweep_position(const SweepSet &s, int k, const Raw3 &p, double q[3]) {
    const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
    if (s.ident[k]) { q[0] = x; q[1] = y; q[2] = z; return; }
    const double *m = s.M + 12 * k;
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = ((m[r * 4] * x + m[r * 4 + 1] * y) + m[r * 4 + 2] * z) + m[r * 4 + 3];
}

// where row i stands: in the frame of sweep 0 for a sweep set, (double)p for plain rows (decided at compile time: no search, no flag)
template <bool SWEEPS>
__device__ __forceinline__ void row_position(const SweepSet &s, const int *lds_off, int i, const Raw3 &p, double q[3]) {
    if (SWEEPS) { sweep_position(s, sweep_of(lds_off, s.K, i), p, q); return; }
    q[0] = (double)p.x; q[1] = (double)p.y; q[2] = (double)p.z;
}

// ---- stable compaction: of the candidates j = 0 .. n-1 (n = the device count where there is one, else n_cap) the source rows
// pre[j] (or j) that a predicate keeps, in order.  Three launches: flags counted per block, the block counts scanned by one block,
// and the flags taken again to place every kept row at block offset + kept rows of the waves in front + kept lanes below its own.
// A predicate is a struct passed by value with
//   void stage(int *lds_off)                           what it wants in LDS before the first flag (ends with a barrier if anything)
//   bool operator()(const int *lds_off, int j, const int *pre)     the flag of candidate j < n
// the block's flags: the wave's ballot, and every wave's count in wave_cnt[] behind a barrier
__device__ __forceinline__ unsigned long long block_ballot(bool k, int *wave_cnt) {
    const unsigned long long m = __ballot(k);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    return m;
}

template <class Pred>
__global__ void k_flag_count(Pred f, const int *__restrict__ pre, int n_cap, const int *__restrict__ n_dev,
                             int *__restrict__ block_count) {
    __shared__ int lds_off[SWEEPS_MAX + 1];
    __shared__ int wave_cnt[TPB / 64];
    f.stage(lds_off);
    const int j = blockIdx.x * TPB + threadIdx.x;
    block_ballot(j < rows_of(n_dev, n_cap) && f(lds_off, j, pre), wave_cnt);
    if (threadIdx.x == 0) {
        int c = 0;
        for (int q = 0; q < TPB / 64; ++q) c += wave_cnt[q];
        block_count[blockIdx.x] = c;
    }
}

// single block: the per-block counts -> their exclusive prefix, *total = the kept count
__global__ void k_scan_blocks(int *__restrict__ block_count, int nblocks, int *__restrict__ total) {
    const int t = block_scan_in_place<TPB>(block_count, nblocks);
    if (threadIdx.x == 0) *total = t;
}

template <class Pred>
__global__ void k_compact(Pred f, const int *__restrict__ pre, int n_cap, const int *__restrict__ n_dev,
                          const int *__restrict__ block_off, int *__restrict__ keep_idx) {
    __shared__ int lds_off[SWEEPS_MAX + 1];
    __shared__ int wave_cnt[TPB / 64];
    f.stage(lds_off);
    const int j = blockIdx.x * TPB + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool k = j < rows_of(n_dev, n_cap) && f(lds_off, j, pre);
    const unsigned long long m = block_ballot(k, wave_cnt);
    int o = block_off[blockIdx.x];
    for (int q = 0; q < wave; ++q) o += wave_cnt[q];
    if (k) keep_idx[o + __popcll(m & ((1ull << lane) - 1ull))] = pre ? pre[j] : j;     // o + rank < the kept total <= n_cap
}

// the box predicate of the radius filters: source row i = pre[j] (or j) is kept when it is NOT strictly inside the ego box (float32
// compare on the RAW point, nusc_loader.py:88-93) and inside the half-open radius box (float64 compare on the position, sign-flipped
// by sxy = -1 for RELLIS, loader_utils.py:182-187).  numpy compares plain float32 rows in float32; float64 gives the same flag for
// every row: a float32 is exactly a double, the product with +-1 is exact, the float32 radius converts exactly, and a comparison with
// a NaN is false at either width.
template <bool SWEEPS>
struct BoxPred {
    SweepSet s;
    double radius, sxy;        // radius <= 0: no radius test
    float ego_x, ego_y;        // ego_x <= 0: no ego box
    __device__ __forceinline__ void stage(int *lds_off) const { stage_offsets<SWEEPS>(s, lds_off); }
    __device__ __forceinline__ bool operator()(const int *lds_off, int j, const int *__restrict__ pre) const {
        const int i = pre ? pre[j] : j;
        if (i < 0 || i >= s.n_total) return false;
        const Raw3 p = load_raw(s, i);
        if (ego_x > 0.f) {
            const bool inside = (p.x < ego_x && p.x > -ego_x) && (p.y < ego_y && p.y > -ego_y);
            if (inside) return false;
        }
        if (radius > 0.) {
            double q[3];
            row_position<SWEEPS>(s, lds_off, i, p, q);
            const double x = q[0] * sxy, y = q[1] * sxy;
            return x >= -radius && x < radius && y >= -radius && y < radius;
        }
        return true;
    }
};

template <bool SWEEPS>
void launch_filter(const BoxPred<SWEEPS> &f, const int32_t *pre_idx, int32_t n, int32_t *block_scratch, int32_t *keep_idx,
                   int32_t *count, hipStream_t st) {
    const int nb = (n + TPB - 1) / TPB;
    k_flag_count<<<nb, TPB, 0, st>>>(f, pre_idx, n, nullptr, block_scratch);
    k_scan_blocks<<<1, TPB, 0, st>>>(block_scratch, nb, count);
    k_compact<<<nb, TPB, 0, st>>>(f, pre_idx, n, nullptr, block_scratch, keep_idx);
}

// out[r][j] = (float)(T[r][0]*x + T[r][1]*y + T[r][2]*z + T[r][3]) in float64, (x, y, z) the position of source row
// keep_idx[sel[j]] with x and y times sxy; columns past the population are the transform of (0,0,0,1) (loader_utils.py:190-199)
template <bool SWEEPS>
__global__ void k_gather_transform(SweepSet s, const int *__restrict__ keep_idx, const int *__restrict__ sel, int n_keep,
                                   int n_sel, double sxy, const double *__restrict__ T, int num_points,
                                   float *__restrict__ out32, double *__restrict__ out64) {
    __shared__ int lds_off[SWEEPS_MAX + 1];
    stage_offsets<SWEEPS>(s, lds_off);
    const int j = blockIdx.x * TPB + threadIdx.x;
    if (j >= num_points) return;
    double x = 0., y = 0., z = 0.;
    if (j < n_sel) {
        const int k = sel ? sel[j] : j;
        const int i = k >= 0 && k < n_keep ? keep_idx[k] : -1;
        if (i >= 0 && i < s.n_total) {
            double q[3];
            row_position<SWEEPS>(s, lds_off, i, load_raw(s, i), q);
            x = q[0] * sxy; y = q[1] * sxy; z = q[2];
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        // numpy's (4x4)@(4xN) float64 product: a plain left-to-right sum of the four terms
        const double v = ((T[r * 4] * x + T[r * 4 + 1] * y) + T[r * 4 + 2] * z) + T[r * 4 + 3] * 1.0;
        if (out32) out32[(long long)r * num_points + j] = (float)v;
        if (out64) out64[(long long)r * num_points + j] = v;
    }
}

// the accumulated cloud itself, for the callers that want what get_accumulated_pc returns: out[j] = q of keep_idx[j]
__global__ void k_sweeps_materialize(SweepSet s, const int *__restrict__ keep_idx, int n, double *__restrict__ out) {
    __shared__ int lds_off[SWEEPS_MAX + 1];
    stage_offsets<true>(s, lds_off);
    const int j = blockIdx.x * TPB + threadIdx.x;
    if (j >= n) return;
    const int i = keep_idx ? keep_idx[j] : j;
    double q[3] = {0., 0., 0.};
    if (i >= 0 && i < s.n_total) row_position<true>(s, lds_off, i, load_raw(s, i), q);
    double *d = out + 3LL * j;
    d[0] = q[0]; d[1] = q[1]; d[2] = q[2];
}

// the shared argument contract of the three efgh_prep_sweeps_* entry points; 0 or EFGH_E_INVALID with a message
int sweeps_check(const float *pts, int32_t stride, const int32_t *off, const double *M, const int32_t *ident, int32_t K,
                 int32_t n_total) {
    if (!pts || !off || !M || !ident) {
        efgh_set_error("sweep set: null points, offsets, transforms or identity flags");
        return EFGH_E_INVALID;
    }
    if (K < 1 || K > SWEEPS_MAX) {
        efgh_set_error("sweep set: K = %d sweeps, supported are 1 .. %d", (int)K, SWEEPS_MAX);
        return EFGH_E_INVALID;
    }
    if (n_total < 1 || n_total >= (1 << 29)) {
        efgh_set_error("sweep set: n_total = %d points, supported are 1 .. 2^29 - 1", (int)n_total);
        return EFGH_E_INVALID;
    }
    if (stride != 3 && stride != 4) {
        efgh_set_error("sweep set: row stride %d, supported are 3 and 4 floats", (int)stride);
        return EFGH_E_INVALID;
    }
    if (stride == 4 && ((uintptr_t)pts & 15)) {
        efgh_set_error("sweep set: stride-4 points must be 16-byte aligned");
        return EFGH_E_INVALID;
    }
    return EFGH_OK;
}

// plain [rows][stride] float32 rows as a source.  The radius filter and the gather of plain rows are told no row count, so they have
// none to check an index against (INT_MAX: every index >= 0 passes, as it always did there)
SweepSet plain_rows(const float *pts, int stride = 4, int rows = INT_MAX) {
    return SweepSet{pts, nullptr, nullptr, nullptr, 0, stride, rows};
}

// ---- voxel thinning: of the candidate rows j = 0 .. n-1 keep the FIRST one of every occupied voxel (stable) ---------------
// Row j stands at q (row_position above; before the RELLIS flip and before
// rand_init_l).  Per axis t = floor(q / v) in float64, an IEEE division.  The row is representable when every t is finite and
// |t| < 2^20; its key is (tx + 2^20) | (ty + 2^20) << 21 | (tz + 2^20) << 42: 63 bits, never the empty marker.  Any other row
// (NaN, inf, out of range, or a source index outside the rows) is kept alone and takes no part in the table.
// Table: cap = the smallest power of two >= 2 n_cap (at least 2), keys[cap] u64 and first[cap] u32, both all ones when empty; home
// slot mix64(key) & (cap - 1), linear probing +1 with wrap.  As in lattice.hip every global atomic costs the same ~1/26 ns
// chip-wide, so the pass pays one CAS per VOXEL (the key is looked up with a plain load first: a key never changes once written,
// so a match is final, and a stale empty only sends the row to the CAS, which returns the truth) and at most one atomicMin per ROW
// (first[slot] only decreases: a plain load that already shows a value <= j is final too).  first[slot] ends as the smallest j of
// the voxel whatever the order of insertion, so the kept set depends on neither the schedule nor the grid.  The representative
// is an input row: no floating-point atomic, no centroid.
// The probe loop is bounded by cap.  At load <= 0.5 it cannot run out; if it ever does, the row is kept alone and count[1] is set,
// which the caller turns into an error: a bug becomes a message, not a hang.
constexpr unsigned long long VOX_EMPTY = ~0ull;
constexpr int VOX_ALONE = -1;                            // slot of a row that is kept alone

struct VoxelTable {
    unsigned long long *keys;  // [cap]
    unsigned *first;           // [cap]
    int *slot;                 // [n_cap] the slot of row j, or VOX_ALONE
    unsigned mask;             // cap - 1
};

template <bool SWEEPS>
__device__ __forceinline__ bool voxel_key(const SweepSet &s, const int *lds_off, int i, double v, unsigned long long *key) {
    if (i < 0 || i >= s.n_total) return false;
    double q[3];
    row_position<SWEEPS>(s, lds_off, i, load_raw(s, i), q);
    unsigned long long k = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double t = floor(q[r] / v);
        if (!(fabs(t) < 1048576.0)) return false;        // tested in double, before any integer cast: NaN and inf fail it
        k |= (unsigned long long)((long long)t + 1048576) << (21 * r);
    }
    *key = k;
    return true;
}

// keys and first <- all ones over the whole table, count[0..1] <- 0
__global__ void k_voxel_init(VoxelTable t, int *__restrict__ count) {
    const unsigned i = blockIdx.x * TPB + threadIdx.x;
    if (i <= t.mask) { t.keys[i] = VOX_EMPTY; t.first[i] = ~0u; }
    if (i < 2) count[i] = 0;
}

template <bool SWEEPS>
__global__ void k_voxel_insert(SweepSet s, const int *__restrict__ keep_in, int n_cap, const int *__restrict__ n_dev, double v,
                               VoxelTable t, int *__restrict__ count) {
    __shared__ int lds_off[SWEEPS_MAX + 1];
    stage_offsets<SWEEPS>(s, lds_off);
    const int j = blockIdx.x * TPB + threadIdx.x;
    if (j >= rows_of(n_dev, n_cap)) return;
    unsigned long long key;
    if (!voxel_key<SWEEPS>(s, lds_off, keep_in ? keep_in[j] : j, v, &key)) { t.slot[j] = VOX_ALONE; return; }
    unsigned h = (unsigned)mix64(key) & t.mask;
    int found = VOX_ALONE;
    for (unsigned probe = 0; probe <= t.mask; ++probe) {
        unsigned long long cur = t.keys[h];
        if (cur == VOX_EMPTY) {
            cur = atomicCAS(&t.keys[h], VOX_EMPTY, key);
            if (cur == VOX_EMPTY) cur = key;             // claimed
        }
        if (cur == key) { found = (int)h; break; }
        h = (h + 1) & t.mask;
    }
    t.slot[j] = found;
    if (found == VOX_ALONE) { count[1] = 1; return; }    // table exhausted
    if (t.first[found] > (unsigned)j) atomicMin(&t.first[found], (unsigned)j);
}

// the voxel predicate of the stable compaction above: candidate j is kept alone, or is the first of its voxel
struct VoxelPred {
    VoxelTable t;
    __device__ __forceinline__ void stage(int *) const {}
    __device__ __forceinline__ bool operator()(const int *, int j, const int *) const {
        const int sl = t.slot[j];
        return sl == VOX_ALONE || t.first[sl] == (unsigned)j;
    }
};

long long voxel_capacity(long long n) {
    long long cap = 2;
    while (cap < 2 * n) cap <<= 1;
    return cap;
}

// the argument contract shared by the two efgh_prep_*voxel_keep entry points, then the five launches
template <bool SWEEPS>
int voxel_keep(const SweepSet &s, const int32_t *keep_in, int32_t n_cap, const int32_t *n_dev, double voxel, void *workspace,
               int32_t *keep_out, int32_t *count, hipStream_t st) {
    if (!(voxel > 0.) || !isfinite(voxel)) {
        efgh_set_error("voxel thinning: voxel = %g, the edge length must be positive and finite", voxel);
        return EFGH_E_INVALID;
    }
    if (n_cap < 0 || n_cap >= (1 << 29)) {
        efgh_set_error("voxel thinning: n_cap = %d candidate rows, supported are 0 .. 2^29 - 1", (int)n_cap);
        return EFGH_E_INVALID;
    }
    if (!keep_in && n_cap > s.n_total) {
        efgh_set_error("voxel thinning: n_cap = %d exceeds the %d rows and there is no keep_in", (int)n_cap, s.n_total);
        return EFGH_E_INVALID;
    }
    if (!workspace || ((uintptr_t)workspace & 7)) {
        efgh_set_error("voxel thinning: workspace is null or not 8-byte aligned");
        return EFGH_E_INVALID;
    }
    if (!keep_out || !count) {
        efgh_set_error("voxel thinning: null keep_out or count");
        return EFGH_E_INVALID;
    }
    const long long cap = voxel_capacity(n_cap);
    VoxelTable t;
    t.keys = (unsigned long long *)workspace;
    t.first = (unsigned *)(t.keys + cap);
    t.slot = (int *)(t.first + cap);
    t.mask = (unsigned)(cap - 1);
    int *blocks = t.slot + n_cap;
    k_voxel_init<<<cdiv(cap, TPB), TPB, 0, st>>>(t, count);
    if (n_cap > 0) {
        const int nb = (n_cap + TPB - 1) / TPB;
        k_voxel_insert<SWEEPS><<<nb, TPB, 0, st>>>(s, keep_in, n_cap, n_dev, voxel, t, count);
        k_flag_count<<<nb, TPB, 0, st>>>(VoxelPred{t}, keep_in, n_cap, n_dev, blocks);
        k_scan_blocks<<<1, TPB, 0, st>>>(blocks, nb, count);
        k_compact<<<nb, TPB, 0, st>>>(VoxelPred{t}, keep_in, n_cap, n_dev, blocks, keep_out);
    }
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

}  // namespace

extern "C" int efgh_prep_affine_nearest_u8(const uint8_t *in, int32_t h, int32_t w, const int64_t *coef6,
                                           uint8_t *out, int32_t nh, int32_t nw, void *stream) {
    EFGH_CHECK_ARG(in && out && coef6 && h > 0 && w > 0 && nh > 0 && nw > 0 && h < 32768 && w < 32768);
    k_affine_nearest_u8<<<grid_for((long long)nh * nw), TPB, 0, (hipStream_t)stream>>>(
        in, h, w, coef6[0], coef6[1], coef6[2], coef6[3], coef6[4], coef6[5], out, nh, nw);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_prep_crop_pad_u8(const uint8_t *in, int32_t h, int32_t w, int32_t oy, int32_t ox, uint8_t *out,
                                     int32_t th, int32_t tw, void *stream) {
    EFGH_CHECK_ARG(in && out && h > 0 && w > 0 && th > 0 && tw > 0);
    k_crop_pad_u8<<<grid_for((long long)th * tw), TPB, 0, (hipStream_t)stream>>>(in, h, w, oy, ox, out, th, tw);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_prep_resample_u8(const uint8_t *in, int32_t h, int32_t w, int32_t axis, int32_t out_size,
                                     const int32_t *bounds, const int32_t *coeffs, int32_t ksize, uint8_t *out,
                                     void *stream) {
    EFGH_CHECK_ARG(in && out && bounds && coeffs && h > 0 && w > 0 && out_size > 0 && ksize > 0 && (axis == 0 || axis == 1));
    const long long total = axis ? (long long)h * out_size : (long long)out_size * w;
    k_resample_u8<<<grid_for(total), TPB, 0, (hipStream_t)stream>>>(in, h, w, axis, out_size, bounds, coeffs, ksize, out);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_prep_hwc_to_chw_u8(const uint8_t *in, int32_t h, int32_t w, uint8_t *chw, uint8_t *mask,
                                       void *stream) {
    EFGH_CHECK_ARG(in && (chw || mask) && h > 0 && w > 0);
    k_hwc_to_chw_u8<<<grid_for((long long)h * w), TPB, 0, (hipStream_t)stream>>>(in, (long long)h * w, chw, mask);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_prep_u8_to_f32_chw_pad(const uint8_t *in, int32_t h, int32_t w, int32_t oy, int32_t ox, float *out,
                                           int32_t th, int32_t tw, void *stream) {
    EFGH_CHECK_ARG(in && out && h > 0 && w > 0 && th > 0 && tw > 0);
    k_u8_to_f32_chw_pad<<<grid_for((long long)th * tw), TPB, 0, (hipStream_t)stream>>>(in, h, w, oy, ox, out, th, tw);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int32_t efgh_prep_filter_blocks(int32_t n) { return (n + TPB - 1) / TPB; }

extern "C" int efgh_prep_radius_filter(const float *pcd, const int32_t *pre_idx, int32_t n, int32_t flip_xy,
                                       float radius, int32_t *block_scratch, int32_t *keep_idx, int32_t *count,
                                       void *stream) {
    hipStream_t st = (hipStream_t)stream;
    EFGH_CHECK_ARG(pcd && block_scratch && keep_idx && count && n > 0 && radius > 0.f);
    launch_filter(BoxPred<false>{plain_rows(pcd), (double)radius, flip_xy ? -1. : 1., 0.f, 0.f}, pre_idx, n, block_scratch,
                  keep_idx, count, st);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_prep_gather_transform(const float *pcd, const int32_t *keep_idx, const int32_t *sel, int32_t n_sel,
                                          int32_t flip_xy, const double *T34, int32_t num_points, float *out32,
                                          double *out64, void *stream) {
    EFGH_CHECK_ARG(pcd && keep_idx && T34 && (out32 || out64) && num_points > 0 && n_sel >= 0 && n_sel <= num_points);
    k_gather_transform<false><<<cdiv(num_points, TPB), TPB, 0, (hipStream_t)stream>>>(
        plain_rows(pcd), keep_idx, sel, INT_MAX, n_sel, flip_xy ? -1. : 1., T34, num_points, out32, out64);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_prep_sweeps_filter(const float *pts, int32_t stride, const int32_t *sweep_off, const double *M34,
                                       const int32_t *identity, int32_t K, int32_t n_total, const int32_t *pre_idx,
                                       int32_t n, int32_t flip_xy, double radius, float ego_x_half, float ego_y_half,
                                       int32_t *block_scratch, int32_t *keep_idx, int32_t *count, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const int rc = sweeps_check(pts, stride, sweep_off, M34, identity, K, n_total);
    if (rc) return rc;
    EFGH_CHECK_ARG(block_scratch && keep_idx && count && n > 0 && n < (1 << 29) && (pre_idx || n == n_total));
    EFGH_CHECK_ARG((radius > 0. || ego_x_half > 0.f) && (ego_x_half > 0.f) == (ego_y_half > 0.f));
    const SweepSet s{pts, sweep_off, M34, identity, K, stride, n_total};
    launch_filter(BoxPred<true>{s, radius > 0. ? radius : 0., flip_xy ? -1. : 1., ego_x_half > 0.f ? ego_x_half : 0.f,
                                ego_y_half > 0.f ? ego_y_half : 0.f},
                  pre_idx, n, block_scratch, keep_idx, count, st);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_prep_sweeps_gather_transform(const float *pts, int32_t stride, const int32_t *sweep_off,
                                                 const double *M34, const int32_t *identity, int32_t K, int32_t n_total,
                                                 const int32_t *keep_idx, int32_t n_keep, const int32_t *sel,
                                                 int32_t n_sel, int32_t flip_xy, const double *T34, int32_t num_points,
                                                 float *out32, double *out64, void *stream) {
    const int rc = sweeps_check(pts, stride, sweep_off, M34, identity, K, n_total);
    if (rc) return rc;
    EFGH_CHECK_ARG(keep_idx && T34 && (out32 || out64) && num_points > 0 && n_keep >= 0 && n_sel >= 0 &&
                   n_sel <= num_points && (sel || n_sel <= n_keep));
    const SweepSet s{pts, sweep_off, M34, identity, K, stride, n_total};
    k_gather_transform<true><<<cdiv(num_points, TPB), TPB, 0, (hipStream_t)stream>>>(
        s, keep_idx, sel, n_keep, n_sel, flip_xy ? -1. : 1., T34, num_points, out32, out64);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int efgh_prep_sweeps_materialize(const float *pts, int32_t stride, const int32_t *sweep_off, const double *M34,
                                            const int32_t *identity, int32_t K, int32_t n_total, const int32_t *keep_idx,
                                            int32_t n, double *out, void *stream) {
    const int rc = sweeps_check(pts, stride, sweep_off, M34, identity, K, n_total);
    if (rc) return rc;
    EFGH_CHECK_ARG(out && n > 0 && n < (1 << 29) && (keep_idx || n <= n_total));
    const SweepSet s{pts, sweep_off, M34, identity, K, stride, n_total};
    k_sweeps_materialize<<<cdiv(n, TPB), TPB, 0, (hipStream_t)stream>>>(s, keep_idx, n, out);
    EFGH_CHECK_LAUNCH();
    return EFGH_OK;
}

extern "C" int64_t efgh_prep_voxel_workspace(int32_t n) {
    if (n < 0 || n >= (1 << 29)) return -1;
    return voxel_capacity(n) * 12 + 4LL * n + 4LL * ((n + TPB - 1) / TPB);
}

extern "C" int efgh_prep_voxel_keep(const float *pts, int32_t stride, int32_t n_rows, const int32_t *keep_in, int32_t n_cap,
                                    const int32_t *n_dev, double voxel, void *workspace, int32_t *keep_out, int32_t *count,
                                    void *stream) {
    if (!pts || n_rows < 1 || n_rows >= (1 << 29)) {
        efgh_set_error("voxel thinning: null pts, or n_rows = %d rows, supported are 1 .. 2^29 - 1", (int)n_rows);
        return EFGH_E_INVALID;
    }
    if ((stride != 3 && stride != 4) || (stride == 4 && ((uintptr_t)pts & 15))) {
        efgh_set_error("voxel thinning: row stride %d, supported are 3 and 4 floats (stride 4: 16-byte aligned)", (int)stride);
        return EFGH_E_INVALID;
    }
    return voxel_keep<false>(plain_rows(pts, stride, n_rows), keep_in, n_cap, n_dev, voxel, workspace, keep_out, count, (hipStream_t)stream);
}

extern "C" int efgh_prep_sweeps_voxel_keep(const float *pts, int32_t stride, const int32_t *sweep_off, const double *M34,
                                           const int32_t *identity, int32_t K, int32_t n_total, const int32_t *keep_in,
                                           int32_t n_cap, const int32_t *n_dev, double voxel, void *workspace, int32_t *keep_out,
                                           int32_t *count, void *stream) {
    const int rc = sweeps_check(pts, stride, sweep_off, M34, identity, K, n_total);
    if (rc) return rc;
    const SweepSet s{pts, sweep_off, M34, identity, K, stride, n_total};
    return voxel_keep<true>(s, keep_in, n_cap, n_dev, voxel, workspace, keep_out, count, (hipStream_t)stream);
}
