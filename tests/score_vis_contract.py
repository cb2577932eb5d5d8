"""What csrc/score_vis.hip computes, and what the masked instances of score.hip's and score_soft.hip's kernels compute, restated in
numpy (include/efgh_hip.h states it in words).  The projection is fuse_contract.project; zmin is np.minimum.at on float32 depths over
the in-frame points; the test is fuse_contract.resolve's expression in float64 with every operation rounded on its own.  The masked
histograms and the masked gradient are the EXISTING contracts on a value array that holds NaN at the points hidden under the
candidate: score_contract.hist1 and score_soft_contract.points1 drop a NaN-valued point from the histogram, and points1's `idx` is all
grad1 ever sees, so the gradient drops it too (test_score_vis_host.py checks that).  `zmin` bits, mask words, `hist`, `count` and the
occupancy of the GPU are held to this EXACTLY (tests/test_gpu_score_vis.py); entropies to score_contract.bounds, the gradient to
score_soft_contract's bound, mi_mm to `mm_bound`, derived below."""
import numpy as np

import fuse_contract as FC
import score_contract as SC
import score_soft_contract as SS

EPS = SC.EPS
KEYS = ('mi', 'nmi', 'hx', 'hy', 'hxy')


def cell_pair(cell):
    return (int(cell[0]), int(cell[1])) if isinstance(cell, (tuple, list)) else (int(cell), int(cell))


def grid(H, W, cell):
    ch, cw = cell_pair(cell)
    return -(-H // ch), -(-W // cw)


def zmin1(pc, T, H, W, cell, min_depth=0.0):
    """-> (float32 (Hc, Wc): the smallest depth of a cell over the in-frame points, +inf where empty; the projection dict; the
    cell index of every point (meaningful where in frame))"""
    ch, cw = cell_pair(cell)
    Hc, Wc = grid(H, W, cell)
    p = FC.project(pc, T, H, W, min_depth)
    at = (p['r'] // ch) * Wc + p['c'] // cw
    z = np.full(Hc * Wc, np.inf, np.float32)
    f = p['frame']
    np.minimum.at(z, at[f], p['d'][f])
    return z.reshape(Hc, Wc), p, at


def visible1(pc, T, H, W, cell, rel_tol=0.0, abs_tol=0.0, min_depth=0.0):
    """-> (bool (N,): in frame and (double)d <= (double)zmin (1 + rel_tol) + abs_tol; zmin float32 (Hc, Wc))"""
    z, p, at = zmin1(pc, T, H, W, cell, min_depth)
    f = p['frame']
    vis = np.zeros(p['d'].shape[0], bool)
    with np.errstate(all='ignore'):
        bound = z.reshape(-1)[at[f]].astype(np.float64) * (1.0 + float(rel_tol)) + float(abs_tol)
        vis[f] = p['d'][f].astype(np.float64) <= bound
    return vis, z


def pack(vis):
    """bool (..., N) -> int32 (..., ceil(N / 32)): bit i % 32 of word i // 32, zeros past N"""
    n = vis.shape[-1]
    nw = -(-n // 32)
    pad = np.zeros(vis.shape[:-1] + (nw * 32,), np.uint64)
    pad[..., :n] = vis
    words = (pad.reshape(vis.shape[:-1] + (nw, 32)) << np.arange(32, dtype=np.uint64)).sum(-1)
    return words.astype(np.uint32).view(np.int32)


def visible(pc, P, H, W, cell, rel_tol=0.0, abs_tol=0.0, min_depth=0.0):
    """the batch: pc (B,C,N) float32, P (B,K,3,4) -> dict of vis bool (B,K,N), mask int32 (B,K,ceil(N/32)), zmin float32 (B,K,Hc,Wc),
    frame bool (B,K,N)"""
    B, K = P.shape[:2]
    N = pc.shape[2]
    Hc, Wc = grid(H, W, cell)
    vis, frame, z = np.zeros((B, K, N), bool), np.zeros((B, K, N), bool), np.zeros((B, K, Hc, Wc), np.float32)
    for b in range(B):
        for k in range(K):
            vis[b, k], z[b, k] = visible1(pc[b], P[b, k], H, W, cell, rel_tol, abs_tol, min_depth)
            frame[b, k] = FC.project(pc[b], P[b, k], H, W, min_depth)['frame']
    return dict(vis=vis, mask=pack(vis), zmin=z, frame=frame)


def masked_value(value, vis):
    """float32 (N,) with NaN at the hidden points"""
    return np.where(vis, value, np.float32(np.nan)).astype(np.float32)


def occupancy(h):
    """int (bins, bins) -> (Rx, Ry, Rxy): the non-empty rows (value bins), columns (grey bins) and cells"""
    h = np.asarray(h, np.int64)
    return int(np.count_nonzero(h.sum(1))), int(np.count_nonzero(h.sum(0))), int(np.count_nonzero(h))


def mi_mm(mi, n, occ):
    """mi - (Rxy - Rx - Ry + 1) / (2 n) in float64 from the exact integers; 0 where n = 0 -> (mi_mm, the correction term)"""
    if n == 0:
        return 0.0, 0.0
    rx, ry, rxy = occ
    corr = (((float(rxy) - float(rx)) - float(ry)) + 1.0) / (2.0 * float(n))
    return mi - corr, corr


def mm_bound(mi_bound, mm, corr):
    """how far the device's mi_mm may lie from `mi_mm`: the numerator and 2 n are small exact integers in float64 on both sides and
    the division is correctly rounded on both sides, so the term has the same bits (eps |corr| is allowed for it all the same); the
    subtraction rounds once on each side, eps |mi_mm| each; mi itself differs by at most its own bound"""
    return mi_bound + 2.0 * EPS * (abs(corr) + abs(mm))


def _fill(out, at, h, n, bins):
    e = SC.entropies(h)
    bd = SC.bounds(e, bins)
    for key in KEYS:
        out[key][at] = e[key]
        out['bound'][key][at] = bd[key]
    occ = occupancy(h)
    out['occupancy'][at] = occ
    out['mi_mm'][at], corr = mi_mm(e['mi'], n, occ)
    out['bound']['mi_mm'][at] = mm_bound(bd['mi'], out['mi_mm'][at], corr)
    return e


def _empty(lead, bins):
    out = {k: np.zeros(lead) for k in KEYS + ('mi_mm',)}
    out['bound'] = {k: np.zeros(lead) for k in KEYS + ('mi_mm',)}
    out.update(hist=np.zeros(lead + (bins, bins), np.int32), count=np.zeros(lead, np.int32), occupancy=np.zeros(lead + (3,), np.int32))
    return out


def score_visible(pc, img, P, value, lo, hi, bins, cell, rel_tol=0.0, abs_tol=0.0, min_depth=0.0):
    """the batch -> score_contract.score's dict on the visible points, plus vis, mask, zmin, frame, occupancy int32 (B,K,3), mi_mm and
    bound['mi_mm']"""
    B, K = P.shape[:2]
    H, W = img.shape[1:3]
    out = _empty((B, K), bins)
    out.update(visible(pc, P, H, W, cell, rel_tol, abs_tol, min_depth))
    for b in range(B):
        for k in range(K):
            h = SC.hist1(pc[b], masked_value(value[b], out['vis'][b, k]), P[b, k], img[b], bins, lo, hi, min_depth)
            out['hist'][b, k] = h
            out['count'][b, k] = _fill(out, (b, k), h, int(h.sum()), bins)['count']
    return out


def score_soft_visible(pc, img, P, value, lo, hi, bins, cell, rel_tol=0.0, abs_tol=0.0, min_depth=0.0, pool=False, chunk=4096, want_grad=True):
    """the batch -> score_soft_contract.score_soft's dict on the visible points (hist with 256 a point, count: the points; pooled: one
    histogram a candidate, the mask still per (b, k)), plus vis, mask, zmin, frame, occupancy, mi_mm and bound['mi_mm']"""
    B, K = P.shape[:2]
    N = pc.shape[2]
    H, W = img.shape[1:3]
    lead = (K,) if pool else (B, K)
    out = _empty(lead, bins)
    out.update(visible(pc, P, H, W, cell, rel_tol, abs_tol, min_depth))
    pts = [[SS.points1(pc[b], masked_value(value[b], out['vis'][b, k]), P[b, k], img[b], bins, lo, hi, min_depth) for k in range(K)]
           for b in range(B)]
    hb = np.stack([np.stack([SS.hist_of(pts[b][k], bins) for k in range(K)]) for b in range(B)])
    hist = hb.sum(0) if pool else hb
    for at in np.ndindex(*lead):
        total = int(hist[at].sum())
        assert total % SS.FRAC == 0 and total < 2 ** 31
        out['count'][at] = total // SS.FRAC
        _fill(out, at, hist[at], total // SS.FRAC, bins)
    out['hist'] = hist.astype(np.int32)
    if want_grad:
        G, GB = np.zeros((B, K, 3, 4)), np.zeros((B, K, 3, 4))
        for b in range(B):
            for k in range(K):
                at = (k,) if pool else (b, k)
                G[b, k], GB[b, k] = SS.grad1(pts[b][k], hist[at], int(out['count'][at]), bins, P[b, k], chunk, N)
        out.update(grad=G, grad_bound=GB)
    return out
