// THE projection of a LiDAR point into an image (fuse.hip, score.hip): float64 with every operation written out, as
// tests/fuse_contract.py::project restates it in numpy.  Every file that includes this is built with -ffp-contract=off
// (efgh_amd/build.py), so that no multiply and add are fused: a multiply-add rounds once where the contract rounds twice.
#pragma once
#include "common.h"
#include <cmath>

namespace {
enum { ST_BEHIND = 0, ST_OUT = 1, ST_OCCLUDED = 2, ST_VISIBLE = 3 };

struct Hit { double u, v; float d; int r, c, state; };          // state: ST_BEHIND, ST_OUT or ST_OCCLUDED (= in frame, not yet resolved)

// every kernel that needs a pixel calls this.  T = one row-major 3x4 matrix
__device__ __forceinline__ Hit project(const float *__restrict__ pc, long long cs, int i, const double *__restrict__ T, int H, int W,
                                       double min_depth) {
    const double px = (double)pc[i], py = (double)pc[cs + i], pz = (double)pc[2 * cs + i];
    const double x = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
    const double y = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
    const double w = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
    const double inf = HUGE_VAL;
    Hit h;
    h.u = x / w; h.v = y / w; h.d = (float)w; h.r = 0; h.c = 0;
    // positive comparisons: a NaN fails every one of them
    if (!(w > min_depth && w < inf && fabs(x) < inf && fabs(y) < inf)) { h.state = ST_BEHIND; return h; }
    if (!(h.u >= 0.0 && h.u < (double)W && h.v >= 0.0 && h.v < (double)H)) { h.state = ST_OUT; return h; }
    h.c = (int)h.u; h.r = (int)h.v;
    h.state = ST_OCCLUDED;
    return h;
}
}  // namespace
