"""The gradient guard's contract restated in numpy float64 (helper of test_grad_guard_host.py / test_gpu_grad_guard*.py; no test
in here).  `decide` is the rule of efgh_grad_guard_measure's second launch, `adam` is torch.optim.Adam's update with the gradient
scale of efgh_adam_step_guarded, `run` chains them over a list of SUMMED gradients the way FusedAdam's guarded step does."""
import math

import numpy as np

# gradient scales of the five-step sequence the tests share (the third step carries a NaN)
SCALES = (1e-3, 1e2, float('nan'), 1e-1, 3e4)


def decide(sumsq, nonfinite, max_norm, grad_scale, skip_nonfinite, applied, skipped, coef_dtype=np.float32):
    """-> dict(norm, coef, scale, skip, applied, skipped).  sumsq / nonfinite: per segment, of the summed gradient.
    coef_dtype: the device rounds the coefficient once to fp32; np.float64 leaves it unrounded (what torch on float64 tensors does)."""
    total = 0.0
    for s in sumsq:                                         # index order
        total += float(s)
    bad = int(sum(int(c) for c in nonfinite))
    norm = math.sqrt(total) * float(grad_scale) if total == total and total >= 0 else float('nan')
    with np.errstate(all='ignore'):
        c = np.float64(max_norm) / (np.float64(norm) + 1e-6)
    coef = coef_dtype(1.0 if c > 1.0 else c)                # clamp(max=1): a NaN stays a NaN; ONE rounding to fp32
    skip = bool(skip_nonfinite and bad != 0)
    if skip:
        skipped += 1
    else:
        applied += 1
    return {'norm': norm, 'coef': coef, 'scale': coef_dtype(grad_scale) * coef, 'skip': skip, 'applied': applied,
            'skipped': skipped, 'nonfinite': bad}


def adam(w, m, v, g, scale, t, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    """one torch.optim.Adam step (step number t) on float64 arrays, gradient g * scale; returns new (w, m, v)"""
    b1, b2 = betas
    gr = g * float(scale) + wd * w
    m = b1 * m + (1 - b1) * gr
    v = b2 * v + (1 - b2) * gr * gr
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    return w - (lr / bc1) * (m / (np.sqrt(v) / math.sqrt(bc2) + eps)), m, v


def gradients(n, seed=0, scales=SCALES):
    """the five summed gradients (float32): scale * N(0,1); a NaN scale -> N(0,1) with one NaN element in the middle"""
    rs = np.random.RandomState(seed)
    out = []
    for s in scales:
        g = rs.standard_normal(n).astype(np.float32)
        if s != s:
            g[n // 2] = np.float32('nan')
        else:
            g = (g * np.float32(s)).astype(np.float32)
        out.append(g)
    return out


def run(w0, grads, max_norm, grad_scale, lr, skip_nonfinite=True, betas=(0.9, 0.999), eps=1e-8, wd=0.0, coef_dtype=np.float32):
    """-> per step (w, m, v, decision) in float64, starting from w0 with zero moments"""
    w = np.asarray(w0, np.float64).copy()
    m, v = np.zeros_like(w), np.zeros_like(w)
    applied = skipped = 0
    out = []
    for g in grads:
        g64 = np.asarray(g, np.float64)
        with np.errstate(all='ignore'):
            d = decide([float(np.sum(g64 * g64))], [int((~np.isfinite(g64)).sum())], max_norm, grad_scale, skip_nonfinite,
                       applied, skipped, coef_dtype)
        applied, skipped = d['applied'], d['skipped']
        if not d['skip']:
            with np.errstate(all='ignore'):
                w, m, v = adam(w, m, v, g64, float(grad_scale) * float(d['coef']), applied, lr, betas, eps, wd)
        out.append((w.copy(), m.copy(), v.copy(), d))
    return out
