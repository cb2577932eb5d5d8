// What score.hip, score_soft.hip and score_vis.hip share (all built with -ffp-contract=off): the projection, the block size, the
// limits and the chunk of a launch, Pillow's L, the visibility mask's layout, the fixed pairwise tree, the argument refusals.
#pragma once
#include "fuse_project.h"

namespace {
constexpr int TPB = 256;
constexpr int MAX_BINS = 64;
constexpr int MAX_K = 4096;
// points of one sample and candidate that one workgroup counts into its LDS histogram before it flushes (a multiple of TPB).  The
// flush costs up to bins^2 global atomics a workgroup, the chunk is what it is spread over; profiles/score.txt has the measurement
#ifndef EFGH_SCORE_CHUNK
#define EFGH_SCORE_CHUNK 4096
#endif
static_assert(EFGH_SCORE_CHUNK % TPB == 0 && EFGH_SCORE_CHUNK > 0, "the chunk is whole passes of the block");

// Pillow's L of an RGB pixel (jitter.hip's luma)
__device__ __forceinline__ int luma(const uint8_t *p) { return (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 0x8000) >> 16; }

// bit i % 32 of word i / 32 of one candidate's visibility mask (score_vis.hip writes it): does point i count?
__device__ __forceinline__ bool mask_bit(const unsigned *__restrict__ m, int i) { return (m[i >> 5] >> (i & 31)) & 1u; }
// the mask words of one (b, k): ceil(N / 32)
__device__ __forceinline__ long long mask_words(int N) { return ((long long)N + 31) >> 5; }

// t[0 .. n) (n a power of two) summed in place, pairs a distance n/2, n/4, .. 1 apart: ONE shape and order whatever the block does
__device__ __forceinline__ double tree_sum(double *t, int n) {
    for (int s = n >> 1; s > 0; s >>= 1) {
        __syncthreads();
        for (int i = threadIdx.x; i < s; i += TPB) t[i] = t[i] + t[i + s];
    }
    __syncthreads();
    const double r = t[0];
    __syncthreads();
    return r;
}

#define SCORE_ARG(cond, ...)                                                         \
    do {                                                                             \
        if (!(cond)) {                                                               \
            efgh_set_error(__VA_ARGS__);                                             \
            return EFGH_E_INVALID;                                                   \
        }                                                                            \
    } while (0)

bool bins_ok(int bins) { return bins == 8 || bins == 16 || bins == 32 || bins == 64; }
}  // namespace
