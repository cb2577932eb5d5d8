"""What csrc/score.hip computes, restated in numpy (include/efgh_hip.h states it in words).  The projection is
fuse_contract.project, imported; the grey level is Pillow's integer L; the value bin is float32 with every operation rounded on its
own; the histogram is np.add.at.  `hist` and `count` of the GPU are held to this EXACTLY (tests/test_gpu_score.py).  The entropies
come from the counts in float64 with math.fsum - more exact than the kernel's pairwise tree - and the GPU's are held to `bounds`,
derived below and never fitted to an output.  tests/test_score_host.py holds this file to properties that are not taken from it."""
import math

import numpy as np

import fuse_contract as FC

BINS = (8, 16, 32, 64)
# Largest error of the device's float64 log in ulp.  ASSUMED: 1 ulp; the ROCm math accuracy table is not in the toolchain at hand.
U_LOG = 1
EPS = 2.0 ** -53


def luma(rgb):
    """uint8 (..., 3) -> Pillow's L as int64"""
    p = rgb.astype(np.int64)
    return (19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16


def value_bin(v, lo, hi, bins):
    """float32 v -> (bin int64, keep bool): t = (v - lo) * scale with scale = float32(bins) / (hi - lo), all float32 and each rounded
    on its own; bins - 1 where t >= bins - 1, 0 where t <= 0, else trunc(t); a NaN v is dropped"""
    v = np.asarray(v)
    assert v.dtype == np.float32
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(all='ignore'):
        scale = np.float32(bins) / np.float32(hi - lo)
        t = ((v - lo).astype(np.float32) * scale).astype(np.float32)
    keep = ~np.isnan(v)
    top = np.float32(bins - 1)
    safe = np.where((t > 0) & (t < top), t, np.float32(0))
    x = np.where(t >= top, bins - 1, safe.astype(np.int64))
    return x.astype(np.int64), keep


def hist1(pc, value, T, img, bins, lo, hi, min_depth=0.0):
    """one sample, one candidate: pc (C >= 3, N) float32, value (N,) float32, T 3x4, img uint8 (H,W,3) -> int64 (bins, bins),
    [value bin][grey bin]"""
    assert bins in BINS
    H, W = img.shape[:2]
    p = FC.project(pc, T, H, W, min_depth)
    x, keep = value_bin(value, lo, hi, bins)
    f = p['frame'] & keep
    y = (luma(img[p['r'][f], p['c'][f]]) * bins) >> 8
    h = np.zeros((bins, bins), np.int64)
    np.add.at(h, (x[f], y), 1)
    return h


def _entropy(counts, n):
    """log n - (sum c log c) / n over the non-zero entries; 0 where one entry holds all n -> (H, S)"""
    c = counts[counts > 0].astype(np.float64)
    S = math.fsum((c * np.log(c)).tolist())
    if c.shape[0] == 1:
        return 0.0, S
    return math.log(n) - S / n, S


def entropies(h):
    """int (bins, bins) -> dict of mi, nmi, hx, hy, hxy (float, nats), count, and the three sums sx, sy, sxy"""
    h = np.asarray(h, dtype=np.int64)
    n = int(h.sum())
    if n == 0:
        return dict(mi=0.0, nmi=0.0, hx=0.0, hy=0.0, hxy=0.0, count=0, sx=0.0, sy=0.0, sxy=0.0)
    hx, sx = _entropy(h.sum(1), n)
    hy, sy = _entropy(h.sum(0), n)
    hxy, sxy = _entropy(h.reshape(-1), n)
    return dict(mi=(hx + hy) - hxy, nmi=0.0 if hxy == 0.0 else (hx + hy) / hxy, hx=hx, hy=hy, hxy=hxy, count=n, sx=sx, sy=sy, sxy=sxy)


def bounds(e, bins):
    """how far the kernel's float64 results may lie from `entropies`' (dict with the same keys).  With eps = 2^-53:
      * every term c log c: the log is off by at most U ulp, the product rounds once; the pairwise tree adds `depth` levels
        (log2 of its leaves: 2 log2 bins for the joint sum, log2 bins for a marginal), each one rounding.  All terms are >= 0, so the
        sum S is off by at most (U + 1 + depth) eps S - the form the issue sets;
      * H = log n - S / n: the log of n (U + 1) eps log n, the division eps S / n on top of dS / n, the subtraction eps |H|;
      * mi = (Hx + Hy) - Hxy: the three dH, and eps |Hx + Hy| + eps |mi| for its two operations;
      * nmi = (Hx + Hy) / Hxy: (dHx + dHy + eps |Hx + Hy|) / Hxy + |Hx + Hy| dHxy / Hxy^2 + eps |nmi| (first order);
    and a factor 2 of margin over all of it, which also holds this file's own rounding (one log, one product, fsum's single
    rounding per sum)."""
    n = e['count']
    if n == 0:
        return dict(mi=0.0, nmi=0.0, hx=0.0, hy=0.0, hxy=0.0)
    lb = int(math.log2(bins))
    ln = math.log(n)

    def dH(S, H, depth):
        dS = (U_LOG + 1 + depth) * EPS * S
        return (U_LOG + 1) * EPS * ln + dS / n + EPS * S / n + EPS * abs(H)

    dx, dy, dxy = dH(e['sx'], e['hx'], lb), dH(e['sy'], e['hy'], lb), dH(e['sxy'], e['hxy'], 2 * lb)
    s = abs(e['hx'] + e['hy'])
    out = dict(hx=dx, hy=dy, hxy=dxy, mi=dx + dy + dxy + EPS * s + EPS * abs(e['mi']))
    out['nmi'] = 0.0 if e['hxy'] == 0.0 else (dx + dy + EPS * s) / e['hxy'] + s * dxy / e['hxy'] ** 2 + EPS * abs(e['nmi'])
    return {k: 2.0 * v for k, v in out.items()}


def score(pc, img, P, value, lo, hi, bins, min_depth=0.0):
    """the batch: pc (B,C,N) float32, img uint8 (B,H,W,3), P (B,K,3,4), value (B,N) float32 -> dict of hist int32 (B,K,bins,bins),
    count int32 (B,K) and mi, nmi, hx, hy, hxy float64 (B,K), plus 'bound': the same five keys, (B,K) each"""
    B, K = P.shape[:2]
    hist = np.zeros((B, K, bins, bins), np.int32)
    keys = ('mi', 'nmi', 'hx', 'hy', 'hxy')
    out = {k: np.zeros((B, K)) for k in keys}
    bound = {k: np.zeros((B, K)) for k in keys}
    count = np.zeros((B, K), np.int32)
    for b in range(B):
        for k in range(K):
            h = hist1(pc[b], value[b], P[b, k], img[b], bins, lo, hi, min_depth)
            hist[b, k] = h
            e = entropies(h)
            bd = bounds(e, bins)
            count[b, k] = e['count']
            for key in keys:
                out[key][b, k] = e[key]
                bound[key][b, k] = bd[key]
    out.update(hist=hist, count=count, bound=bound)
    return out
