// The launchers of refine.hip, called by the checked entry points of api.cpp (efgh_refine_step, efgh_refine_select): the arguments
// have been checked, these only launch.
#pragma once
#include "common.h"

constexpr int EFGH_REFINE_MAX_S = 4096;          // starts of a call: score.hip's MAX_K, the K axis they ride on
constexpr int EFGH_REFINE_MAX_KEEP = 64;

struct efgh_refine_scale { double s[6]; };       // (internal: the six by-value scales of the entry point, as one kernel argument)

int efgh_launch_refine_step(const double *G, const double *Pstart, double *P, const double *mi, int B, int S, int pool, double *z, double *m,
                            double *v, double *best_mi, int64_t *best_iter, double *best_pose, double *trace, efgh_refine_scale scale, int it,
                            double step_size, double bc2_sqrt, int last, hipStream_t st);
int efgh_launch_refine_select(const double *val, int rows, int K, int keep, int32_t *idx, hipStream_t st);
