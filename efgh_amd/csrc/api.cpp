// Error plumbing of the C-ABI (include/efgh_hip.h), and the checked entry points of refine.hip.
#include "common.h"
#include "refine.h"

static thread_local char g_err[512] = "";

void efgh_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *efgh_last_error(void) { return g_err; }
extern "C" int efgh_version(void) { return EFGH_ABI_VERSION; }

#define REFINE_ARG(cond, ...)                                                        \
    do {                                                                             \
        if (!(cond)) {                                                               \
            efgh_set_error(__VA_ARGS__);                                             \
            return EFGH_E_INVALID;                                                   \
        }                                                                            \
    } while (0)

extern "C" int efgh_refine_step(const double *G, const double *Pstart, double *P, const double *mi, int32_t B, int32_t S, int32_t pool,
                                double *z, double *m, double *v, double *best_mi, int64_t *best_iter, double *best_pose, double *trace,
                                double scale0, double scale1, double scale2, double scale3, double scale4, double scale5, int32_t it,
                                double step_size, double bc2_sqrt, int32_t last, void *stream) {
    const char *who = "efgh_refine_step";
    REFINE_ARG(last == 0 || last == 1, "%s: last = %d must be 0 or 1", who, (int)last);
    REFINE_ARG(Pstart && P && mi && z && m && v && best_mi && best_iter && best_pose && trace && (G || last),
               "%s: null pointer (G %p, Pstart %p, P %p, mi %p, z %p, m %p, v %p, best_mi %p, best_iter %p, best_pose %p, trace %p)", who,
               (const void *)G, (const void *)Pstart, (void *)P, (const void *)mi, (void *)z, (void *)m, (void *)v, (void *)best_mi,
               (void *)best_iter, (void *)best_pose, (void *)trace);
    REFINE_ARG(B > 0 && B <= 65535, "%s: B = %d, supported are 1 .. 65535", who, (int)B);
    REFINE_ARG(S > 0 && S <= EFGH_REFINE_MAX_S, "%s: S = %d starts, supported are 1 .. %d", who, (int)S, EFGH_REFINE_MAX_S);
    REFINE_ARG(pool == 0 || pool == 1, "%s: pool = %d must be 0 or 1", who, (int)pool);
    REFINE_ARG(it >= 0, "%s: it = %d, the iterate's number must be >= 0", who, (int)it);
    const efgh_refine_scale sc = {{scale0, scale1, scale2, scale3, scale4, scale5}};
    for (int a = 0; a < 6; ++a)
        REFINE_ARG(std::isfinite(sc.s[a]) && sc.s[a] >= 0.0, "%s: scale%d = %g must be finite and >= 0 (0 freezes the axis)", who, a, sc.s[a]);
    REFINE_ARG(std::isfinite(step_size) && step_size > 0.0, "%s: step_size = %g must be finite and positive", who, step_size);
    REFINE_ARG(std::isfinite(bc2_sqrt) && bc2_sqrt > 0.0, "%s: bc2_sqrt = %g must be finite and positive", who, bc2_sqrt);
    return efgh_launch_refine_step(G, Pstart, P, mi, B, S, pool, z, m, v, best_mi, best_iter, best_pose, trace, sc, it, step_size, bc2_sqrt,
                                   last, (hipStream_t)stream);
}

extern "C" int efgh_refine_select(const double *val, int32_t rows, int32_t K, int32_t keep, int32_t *idx, void *stream) {
    const char *who = "efgh_refine_select";
    REFINE_ARG(val && idx, "%s: null pointer (val %p, idx %p)", who, (const void *)val, (void *)idx);
    REFINE_ARG(rows > 0 && rows <= 65535, "%s: rows = %d, supported are 1 .. 65535", who, (int)rows);
    REFINE_ARG(K > 0 && K <= EFGH_REFINE_MAX_S, "%s: K = %d values a row, supported are 1 .. %d", who, (int)K, EFGH_REFINE_MAX_S);
    REFINE_ARG(keep > 0 && keep <= EFGH_REFINE_MAX_KEEP && keep <= K, "%s: keep = %d of K = %d, supported are 1 .. min(K, %d)", who, (int)keep,
               (int)K, EFGH_REFINE_MAX_KEEP);
    return efgh_launch_refine_select(val, rows, K, keep, idx, (hipStream_t)stream);
}
