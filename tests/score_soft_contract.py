"""What csrc/score_soft.hip computes, restated in numpy (include/efgh_hip.h states it in words).  The projection is
fuse_contract.project, the value bin and the grey level are score_contract's, the bilinear convention is fuse_contract.resolve's; every
float64 operation is element-wise and in the kernel's order, so the per-point quantities have the kernel's bits.  `hist` and `count` of
the GPU are held to this EXACTLY (tests/test_gpu_score_soft.py); the entropies to score_contract.bounds on the histogram as it is (256 a
point); the gradient to `grad_bound`, derived below and never fitted to an output.  frac=None gives the UNQUANTISED function, whose
derivative the gradient is: tests/test_score_soft_host.py holds it to central differences of that function."""
import math

import numpy as np

import fuse_contract as FC
import score_contract as SC

FRAC = 256
EPS = SC.EPS
TPB = 256                # threads of a workgroup: a thread sums chunk / TPB points in order, the block's tree has log2 TPB levels
# float64 roundings of one point's term in which the device may differ from this file once the table differs in its last bits: the
# table difference, / n, * gu, / w, * X, and for row 2 the product with (gu u + gv v) and the sign
TERM_OPS = 8


def sample(pc, T, img, min_depth=0.0):
    """-> fuse_contract's projection dict, and for the in-frame points g, gu, gv (float64): the bilinear grey level at (u - 0.5, v - 0.5)
    on Pillow's integer L with the neighbours clipped to the frame, and its slopes in u and v"""
    H, W = img.shape[:2]
    p = FC.project(pc, T, H, W, min_depth)
    f = p['frame']
    L = SC.luma(img).astype(np.float64)
    fx, fy = p['u'][f] - 0.5, p['v'][f] - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = fx - x0, fy - y0
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb = np.clip(xi, 0, W - 1), np.clip(xi + 1, 0, W - 1)
    ya, yb = np.clip(yi, 0, H - 1), np.clip(yi + 1, 0, H - 1)
    a, b, c, d = L[ya, xa], L[ya, xb], L[yb, xa], L[yb, xb]
    ba, dc = b - a, d - c
    top = a + ba * tx
    bot = c + dc * tx
    g = top + (bot - top) * ty
    gu = ba + (dc - ba) * ty
    gv = bot - top
    return p, g, gu, gv


def cells(g, bins):
    """grey level -> (j int64, fr in [0, 1], gate s): t = g (bins / 256) - 0.5, j = clip(floor(t), 0, bins - 2), fr = clip(t - j, 0, 1),
    s = 1 iff 0 < t - j < 1"""
    t = g * (bins / 256.0) - 0.5
    j = np.clip(np.floor(t), 0, bins - 2)
    r = t - j
    s = (r > 0.0) & (r < 1.0)
    return j.astype(np.int64), np.clip(r, 0.0, 1.0), s


def points1(pc, value, T, img, bins, lo, hi, min_depth=0.0):
    """one sample, one candidate -> dict of the points that count: idx, x, j, fr, s, q, gu, gv, u, v, w, X (4, n)"""
    assert bins in SC.BINS
    p, g, gu, gv = sample(pc, T, img, min_depth)
    x, keep = SC.value_bin(value, lo, hi, bins)
    k = keep[p['frame']]
    idx = np.nonzero(p['frame'])[0][k]
    j, fr, s = cells(g[k], bins)
    X = np.stack([pc[0, idx], pc[1, idx], pc[2, idx], np.ones(idx.shape[0], np.float32)]).astype(np.float64)
    Tm = np.asarray(T, dtype=np.float64).reshape(12)
    w = ((Tm[8] * X[0] + Tm[9] * X[1]) + Tm[10] * X[2]) + Tm[11]
    return dict(idx=idx, x=x[idx], j=j, fr=fr, s=s, q=np.floor(fr * FRAC + 0.5).astype(np.int64), gu=gu[k], gv=gv[k],
                u=p['u'][idx], v=p['v'][idx], w=w, X=X)


def hist_of(pt, bins, frac=FRAC):
    """int64 (bins, bins) with FRAC a point, or with frac=None float64 with 1 a point and the weights as they are"""
    if frac is None:
        h = np.zeros((bins, bins))
        np.add.at(h, (pt['x'], pt['j']), 1.0 - pt['fr'])
        np.add.at(h, (pt['x'], pt['j'] + 1), pt['fr'])
        return h
    assert frac == FRAC
    h = np.zeros((bins, bins), np.int64)
    np.add.at(h, (pt['x'], pt['j']), FRAC - pt['q'])
    np.add.at(h, (pt['x'], pt['j'] + 1), pt['q'])
    return h


def hist1(pc, value, T, img, bins, lo, hi, min_depth=0.0, frac=FRAC):
    return hist_of(points1(pc, value, T, img, bins, lo, hi, min_depth), bins, frac)


def mi_float(h):
    """MI in nats of a non-negative float histogram (the unquantised function)"""
    n = h.sum()
    if n <= 0:
        return 0.0

    def S(c):
        c = c[c > 0].astype(np.float64)
        return math.fsum((c * np.log(c)).tolist())
    return (S(h.reshape(-1)) - S(h.sum(0)) - S(h.sum(1))) / n + math.log(n)


def table(h):
    """-> Tt (bins, bins) float64 = log h_xy - log h_y where h_xy > 0 and 0 elsewhere, its error bound, the flags h_xy > 0.
    Bound of a cell, with eps = 2^-53: each of the two logs is off by at most U_LOG ulp on the device and rounds once here,
    (U_LOG + 1) eps |log| each; the subtraction rounds once, eps |Tt|"""
    h = np.asarray(h)
    pos = h > 0
    hy = h.sum(0)
    with np.errstate(all='ignore'):
        lxy = np.where(pos, np.log(np.where(pos, h, 1).astype(np.float64)), 0.0)
        ly = np.where(hy > 0, np.log(np.where(hy > 0, hy, 1).astype(np.float64)), 0.0)
    Tt = np.where(pos, lxy - ly[None, :], 0.0)
    dT = np.where(pos, (SC.U_LOG + 1) * EPS * (np.abs(lxy) + np.abs(ly)[None, :]) + EPS * np.abs(Tt), 0.0)
    return Tt, dT, pos


def grad1(pt, h, n, bins, T, chunk, N):
    """the points of one sample and candidate, the histogram they belong to (their own, or the pooled one) and its number of points
    -> (G (3,4), bound (3,4)).

    Per point, in the kernel's order: a = ((Tt[x][j+1] - Tt[x][j]) (bins / 256)) / n where the gate is open and both cells are not
    empty, r0 = (a gu) / w, r1 = (a gv) / w, r2 = -((a (gu u + gv v)) / w), and r0 X, r1 X, r2 X go to rows 0, 1, 2.  Everything but
    the table has the kernel's bits, so the kernel's result differs from this one by
      * the table: |d term| <= |term / dTt| (dTt[x][j] + dTt[x][j+1] + eps |difference|), summed over the points;
      * TERM_OPS roundings of a term that may fall differently once the table does: TERM_OPS eps |term|;
      * the order of the sum: a thread adds its chunk / 256 points one after another, the block's tree has 8 levels, the fold's
        ceil(log2(chunks)) - each level one rounding of a partial sum that is at most the sum of the |term|s - against math.fsum
        here, which rounds once;
    and a factor 2 of margin over all of it, as score_contract.bounds takes."""
    G, bound = np.zeros((3, 4)), np.zeros((3, 4))
    if pt['idx'].shape[0] == 0 or n == 0:
        return G, bound
    Tt, dTt, pos = table(h)
    x, j = pt['x'], pt['j']
    ok = pt['s'] & pos[x, j] & pos[x, j + 1]
    gain = bins / 256.0
    diff = Tt[x, j + 1] - Tt[x, j]
    ddiff = dTt[x, j + 1] + dTt[x, j] + EPS * np.abs(diff)
    with np.errstate(all='ignore'):
        a = np.where(ok, (diff * gain) / float(n), 0.0)
        unit = np.where(ok, gain / float(n), 0.0)                # a per unit of the table difference
        gu, gv, u, v, w = pt['gu'], pt['gv'], pt['u'], pt['v'], pt['w']
        dot = gu * u + gv * v
        r = [(a * gu) / w, (a * gv) / w, -((a * dot) / w)]
        r1 = [np.abs(unit * gu / w), np.abs(unit * gv / w), np.abs(unit * dot / w)]
    n_chunk = -(-N // chunk)
    depth = chunk // TPB + int(math.log2(TPB)) + (int(math.ceil(math.log2(n_chunk))) if n_chunk > 1 else 0) + 1
    for i in range(3):
        for c in range(4):
            term = (r[i] * pt['X'][c])[ok]
            G[i, c] = math.fsum(term.tolist())
            mag = math.fsum(np.abs(term).tolist())
            tab = math.fsum((r1[i] * np.abs(pt['X'][c]) * ddiff)[ok].tolist())
            bound[i, c] = 2.0 * (tab + (TERM_OPS + depth) * EPS * mag)
    return G, bound


def grad_float(pc, value, T, img, bins, lo, hi, min_depth=0.0):
    """(mi, G (3,4)) of the unquantised function at T: what central differences of `mi_float(hist1(.., frac=None))` approach"""
    pt = points1(pc, value, T, img, bins, lo, hi, min_depth)
    h = hist_of(pt, bins, None)
    G, _ = grad1(pt, h, pt['idx'].shape[0], bins, T, 4096, pc.shape[1])
    return mi_float(h), G


def score_soft(pc, img, P, value, lo, hi, bins, min_depth=0.0, pool=False, chunk=4096, want_grad=True):
    """the batch: pc (B,C,N) float32, img uint8 (B,H,W,3), P (B,K,3,4), value (B,N) float32 -> dict of hist int32 (B,K,bins,bins) with
    256 a point, count int32 (B,K): the points, mi, nmi, hx, hy, hxy float64 (B,K) and 'bound' with the same five keys
    (score_contract's, on the histogram as it is), grad and grad_bound float64 (B,K,3,4).  pool=True: one histogram a candidate, summed
    over the samples - hist (K,bins,bins), the other fields (K,), grad still (B,K,3,4).  `chunk` is efgh_score_chunk()."""
    B, K = P.shape[:2]
    N = pc.shape[2]
    keys = ('mi', 'nmi', 'hx', 'hy', 'hxy')
    pts = [[points1(pc[b], value[b], P[b, k], img[b], bins, lo, hi, min_depth) for k in range(K)] for b in range(B)]
    hb = np.stack([np.stack([hist_of(pts[b][k], bins) for k in range(K)]) for b in range(B)])
    hist = hb.sum(0) if pool else hb
    lead = (K,) if pool else (B, K)
    out = {k: np.zeros(lead) for k in keys}
    bound = {k: np.zeros(lead) for k in keys}
    count = np.zeros(lead, np.int32)
    for at in np.ndindex(*lead):
        e = SC.entropies(hist[at])
        bd = SC.bounds(e, bins)
        assert e['count'] % FRAC == 0 and e['count'] < 2 ** 31
        count[at] = e['count'] // FRAC
        for key in keys:
            out[key][at] = e[key]
            bound[key][at] = bd[key]
    out.update(hist=hist.astype(np.int32), count=count, bound=bound)
    if want_grad:
        G, GB = np.zeros((B, K, 3, 4)), np.zeros((B, K, 3, 4))
        for b in range(B):
            for k in range(K):
                at = (k,) if pool else (b, k)
                G[b, k], GB[b, k] = grad1(pts[b][k], hist[at], int(count[at]), bins, P[b, k], chunk, N)
        out.update(grad=G, grad_bound=GB)
    return out
