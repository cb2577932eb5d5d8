"""`score` and `score_soft` on VISIBLE points only, and the Miller-Madow correction of a sparse histogram's bias (csrc/score_vis.hip;
DESIGN 3).  LiDAR and camera sit apart: a LiDAR point on a far surface can land on a pixel that shows a nearer surface,
and every such point pairs a reflectance with the wrong grey level.  Which points those are changes with the candidate, so every
candidate gets a depth test of its own.  Not in the reference; off unless called.

    occ = Occlusion(cell=(8, 2), rel_tol=0.02, abs_tol=0.1)
    v = visible_mask(pcd, image, poses, occ)           # Visibility: v.mask int32 (B,K,ceil(N/32)), v.zmin float32 (B,K,Hc,Wc)
    v.unpack(), v.count()                              # bool (B,K,N), int32 (B,K)
    s = score_visible(pcd, image, poses, occlusion=occ)               # VisibleScore: Score's fields, mi_mm, occupancy
    s = score_soft_visible(pcd, image, P.requires_grad_(), occlusion=occ)
    r = refine(pcd, image, P0, scorer=functools.partial(score_soft_visible, occlusion=occ))
    occupancy(s.hist), miller_madow(score(pcd, image, poses, want_hist=True))

The test: the image is cut into cells of cell_h x cell_w pixels (clipped at the right and bottom edges); zmin of a cell is the
smallest float32 depth over ALL points in frame under the candidate (a point with a NaN value is still a surface and occludes); a
point is visible iff it is in frame and d <= zmin (1 + rel_tol) + abs_tol, `fuse`'s expression.  Ties are all visible.  cell = 1 is
`fuse` at radius 0.  Rectangular cells suit a spinning LiDAR, dense along a ring and several pixels apart between rings.

Limits: a cell-based test hides an oblique plane from itself (the near end of the plane inside a cell hides the far end) unless the
tolerance allows for the depth range of a surface inside one cell; which tolerance suits a sensor and a scene is the caller's
choice, none is built in.  The Miller-Madow term (Rxy - Rx - Ry + 1) / (2 n), with Rx, Ry, Rxy the non-empty rows, columns and cells,
is the first-order bias of the plug-in MI of n independent draws; with every cell filled it is the (bins - 1)^2 / (2 n) that score.py
names.  On the SOFT histogram it is a heuristic: a point occupies up to two cells there, so the occupancy counts are not those of n
single draws.  No effect on registration accuracy is claimed or was measured."""
import numpy as np
import torch

from .. import _C
from .fuse import _finite_nonneg, _image_u8, _on_the_clouds_device
from .fuse import _fail as _fuse_fail
from .score import BINS, BY, Score, _checked, _checked_poses, _kernel_inputs
from .score_soft import FRAC, MAX_POINTS, _SoftMI

MAX_CELL = 64
MAX_ZMIN_CELLS = 1 << 29     # cells of one call's zmin workspace, 4 bytes each: a memory sanity cap, not a measurement


class Occlusion:
    """the depth test's settings: cell, an int or a pair (cell_h, cell_w) of pixels, 1 .. 64 each | rel_tol, abs_tol finite and >= 0:
    visible iff d <= zmin (1 + rel_tol) + abs_tol"""
    __slots__ = ('cell_h', 'cell_w', 'rel_tol', 'abs_tol')

    def __init__(self, cell=8, rel_tol=0.0, abs_tol=0.0):
        pair = cell if isinstance(cell, (tuple, list)) else (cell, cell)
        if len(pair) != 2 or not all(not isinstance(c, bool) and isinstance(c, (int, np.integer)) and 1 <= c <= MAX_CELL for c in pair):
            raise _C.EfghError('Occlusion: cell: %r, expected an integer or a pair (cell_h, cell_w), 1 .. %d each' % (cell, MAX_CELL))
        for name, v in (('rel_tol', rel_tol), ('abs_tol', abs_tol)):
            _finite_nonneg(name, v, 'Occlusion')
        self.cell_h, self.cell_w, self.rel_tol, self.abs_tol = int(pair[0]), int(pair[1]), float(rel_tol), float(abs_tol)

    @property
    def cell(self):
        return self.cell_h, self.cell_w

    def grid(self, H, W):
        """(Hc, Wc) of an H x W image"""
        return -(-H // self.cell_h), -(-W // self.cell_w)

    def __repr__(self):
        return 'Occlusion(cell=%r, rel_tol=%r, abs_tol=%r)' % (self.cell, self.rel_tol, self.abs_tol)


class Visibility:
    """device tensors of one `visible_mask` call: mask int32 (B,K,ceil(N/32)), bit i % 32 of word i // 32 is point i, bits past N are
    zero | zmin float32 (B,K,Hc,Wc), +inf where a cell is empty | n: N"""
    __slots__ = ('mask', 'zmin', 'n')

    def __init__(self, mask, zmin, n):
        self.mask, self.zmin, self.n = mask, zmin, n

    def unpack(self):
        """bool (B,K,N)"""
        return unpack_mask(self.mask, self.n)

    def count(self):
        """int32 (B,K): the visible points of every candidate"""
        return self.unpack().sum(-1, dtype=torch.int32)


def unpack_mask(mask, n):
    """int32 (..., ceil(n/32)) -> bool (..., n), with torch ops on the mask's device"""
    bits = (mask[..., None] >> torch.arange(32, dtype=torch.int32, device=mask.device)) & 1
    return bits.reshape(mask.shape[:-1] + (-1,))[..., :n].bool()


class VisibleScore(Score):
    """`Score`'s fields on the visible points, and: mi_mm float64, the Miller-Madow estimate (0 where count = 0) | occupancy int32
    (..., 3): the non-empty rows, columns and cells of the histogram | mask int32 (B,K,ceil(N/32)) and zmin float32 (B,K,Hc,Wc) with
    want_mask, else None (per (b, k) also when pooled)"""
    __slots__ = ('mi_mm', 'occupancy', 'mask', 'zmin')

    def __init__(self, **kw):
        for k in Score.__slots__ + VisibleScore.__slots__:      # (Score.__init__ walks the __slots__ of the instance's class: these four)
            setattr(self, k, kw.get(k))


def _occlusion(who, occlusion):
    if occlusion is None:
        return Occlusion()
    if not isinstance(occlusion, Occlusion):
        _fuse_fail('occlusion: expected an Occlusion or None, got %s' % type(occlusion).__name__, who)
    return occlusion


def _workspace(who, occ, B, K, H, W):
    """(Hc, Wc) after the workspace limit"""
    Hc, Wc = occ.grid(H, W)
    cells = B * K * Hc * Wc
    if cells > MAX_ZMIN_CELLS:
        _fuse_fail('occlusion: B = %d, K = %d and cell = %r on %d x %d need a zmin workspace of %d bytes, at most %d cells (2^29): take a '
                   'larger cell or fewer candidates a call' % (B, K, occ.cell, H, W, 4 * cells, MAX_ZMIN_CELLS), who)
    return Hc, Wc


def _mask(L, st, pc, P, B, N, K, H, W, Hc, Wc, occ, min_depth):
    """the two launches (call with the cloud's device current; pc and P as `_kernel_inputs` hands them) -> mask int32, zmin int32"""
    dev = pc.device
    zmin = torch.empty((B, K, Hc, Wc), dtype=torch.int32, device=dev)
    mask = torch.empty((B, K, -(-N // 32)), dtype=torch.int32, device=dev)      # every word is written: no zeroing
    _C.check(L.efgh_score_zmin(_C.ptr(pc), pc.stride(0), pc.stride(1), B, N, _C.ptr(P), K, H, W, occ.cell_h, occ.cell_w, min_depth,
                               _C.ptr(zmin), st()))
    _C.check(L.efgh_score_visible(_C.ptr(pc), pc.stride(0), pc.stride(1), B, N, _C.ptr(P), K, H, W, occ.cell_h, occ.cell_w, min_depth,
                                  occ.rel_tol, occ.abs_tol, _C.ptr(zmin), _C.ptr(mask), st()))
    return mask, zmin


def visible_mask(pc, img, cam_T_velo, occlusion=None, min_depth=0.0):
    """pc float32 (B, C >= 3, N) | img as in `fuse`, or the pair (H, W): the pixels are not read | cam_T_velo (B,K,3,4), or (B,3,4)
    for K = 1 | occlusion an `Occlusion` (None: the default one) -> Visibility.  Inputs are never written, outputs are new tensors,
    nothing is read back to the host."""
    who = 'visible_mask'
    B, N, K, T = _checked_poses(who, pc, cam_T_velo)
    named = [('cam_T_velo', T)]
    if isinstance(img, (tuple, list)):
        if len(img) != 2 or not all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) for v in img) \
                or img[0] < 1 or img[1] < 1 or img[0] * img[1] >= 2 ** 31 - 1:
            _fuse_fail('img: %r, expected an image or (H, W), both positive and H*W < 2^31' % (img,), who)
        H, W = int(img[0]), int(img[1])
    else:
        img, H, W = _image_u8(img, B, who)
        named.append(('img', img))
    occ = _occlusion(who, occlusion)
    _finite_nonneg('min_depth', min_depth, who)
    Hc, Wc = _workspace(who, occ, B, K, H, W)
    _on_the_clouds_device(pc, named, who, 'the visibility test')
    with torch.cuda.device(pc.device):
        if pc.stride(2) != 1:
            pc = pc.contiguous()
        P = T.detach().to(torch.float64).contiguous()
        mask, zmin = _mask(_C.lib(), _C.stream_ptr, pc, P, B, N, K, H, W, Hc, Wc, occ, float(min_depth))
    return Visibility(mask, zmin.view(torch.float32), N)


def occupancy(hist):
    """hist int32 (..., bins, bins) of any `Score` on the GPU -> int32 (..., 3): the non-empty rows (value bins), columns (grey bins)
    and cells, counted on the device"""
    who = 'occupancy'
    if not torch.is_tensor(hist):
        _fuse_fail('hist: expected a tensor (a Score.hist: pass want_hist=True), got %s' % type(hist).__name__, who)
    if hist.dtype != torch.int32:
        _fuse_fail('hist: dtype %s, expected int32' % hist.dtype, who)
    if hist.dim() < 2 or hist.shape[-1] != hist.shape[-2] or hist.shape[-1] not in BINS or hist.numel() == 0:
        _fuse_fail('hist: expected (..., bins, bins) with bins one of %s, got %s' % (', '.join(map(str, BINS)), tuple(hist.shape)), who)
    if not hist.is_cuda:
        _fuse_fail('hist: a CPU tensor; the occupancy is counted on the GPU through libefgh_hip.so only', who)
    bins = hist.shape[-1]
    with torch.cuda.device(hist.device):
        h = hist.contiguous()
        occ = torch.empty(hist.shape[:-2] + (3,), dtype=torch.int32, device=hist.device)
        _C.check(_C.lib().efgh_score_occupancy(_C.ptr(h), h.numel() // (bins * bins), int(bins), _C.ptr(occ), _C.stream_ptr()))
    return occ


def _mi_mm(mi, count, occ):
    """mi - (Rxy - Rx - Ry + 1) / (2 count) in float64 from the exact integers, 0 where count = 0; torch ops, no host read"""
    o = occ.to(torch.float64)
    n = count.to(torch.float64)
    corr = (((o[..., 2] - o[..., 0]) - o[..., 1]) + 1.0) / (2.0 * n.clamp(min=1.0))
    return torch.where(count > 0, mi - corr, torch.zeros_like(mi))


def miller_madow(s):
    """a `Score` with its histogram (`score(..., want_hist=True)`, `score_soft`, or a VisibleScore) -> float64 like s.mi: mi - (Rxy -
    Rx - Ry + 1) / (2 count), and 0 where count = 0.  On a soft histogram it is a heuristic (a point occupies up to two cells)."""
    if not isinstance(s, Score):
        _fuse_fail('s: expected a Score, got %s' % type(s).__name__, 'miller_madow')
    if s.hist is None or s.count is None or s.mi is None:
        _fuse_fail('s: the Score has no hist (pass want_hist=True to the call that made it)', 'miller_madow')
    return _mi_mm(s.mi, s.count, occupancy(s.hist))


def score_visible(pc, img, cam_T_velo, occlusion=None, value=None, value_range=(0.0, 1.0), bins=32, min_depth=0.0, want_hist=False,
                  want_mask=False):
    """`score`'s arguments and its checks, and occlusion (an `Occlusion`; None: the default one) -> VisibleScore: a point counts iff
    it is visible under its candidate and its value is not NaN.  Five launches (zmin, mask, histogram, entropies, occupancy).
    Inputs are never written, outputs are new tensors, nothing is read back to the host; an empty histogram gives zeros."""
    who = 'score_visible'
    occ = _occlusion(who, occlusion)
    B, N, K, T, img, H, W, value, lo, hi = _checked(who, pc, img, cam_T_velo, value, value_range, bins, min_depth,
                                                    more=lambda B, K, H, W: _workspace(who, occ, B, K, H, W))
    Hc, Wc = occ.grid(H, W)

    dev = pc.device
    L, st = _C.lib(), _C.stream_ptr
    bins, min_depth = int(bins), float(min_depth)
    with torch.cuda.device(dev):
        pc, value, P, img = _kernel_inputs(pc, value, T, img)
        mask, zmin = _mask(L, st, pc, P, B, N, K, H, W, Hc, Wc, occ, min_depth)
        hist = torch.empty((B, K, bins, bins), dtype=torch.int32, device=dev)
        out = torch.empty((B, K, 5), dtype=torch.float64, device=dev)
        count = torch.empty((B, K), dtype=torch.int32, device=dev)
        ocp = torch.empty((B, K, 3), dtype=torch.int32, device=dev)
        _C.check(L.efgh_score_hist_masked(_C.ptr(pc), pc.stride(0), pc.stride(1), B, N, _C.ptr(value), value.stride(0), _C.ptr(P), K,
                                          _C.ptr(img), H, W, bins, lo, hi, min_depth, _C.ptr(mask), _C.ptr(hist), st()))
        _C.check(L.efgh_score_mi(_C.ptr(hist), B, K, bins, _C.ptr(out), _C.ptr(count), st()))
        _C.check(L.efgh_score_occupancy(_C.ptr(hist), B * K, bins, _C.ptr(ocp), st()))
        fields = {k: out[:, :, i] for i, k in enumerate(BY)}
        mm = _mi_mm(fields['mi'], count, ocp)
    return VisibleScore(count=count, hist=hist if want_hist else None, mi_mm=mm, occupancy=ocp, mask=mask if want_mask else None,
                        zmin=zmin.view(torch.float32) if want_mask else None, **fields)


def score_soft_visible(pc, img, cam_T_velo, occlusion=None, value=None, value_range=(0.0, 1.0), bins=32, min_depth=0.0, pool=False,
                       want_hist=False, want_mask=False):
    """`score_soft`'s arguments and its checks, and occlusion -> VisibleScore on the soft histogram of the visible points.  pool=True
    keeps its meaning: one mask per (b, k), the histograms summed over b.  Where cam_T_velo requires grad, `mi` and `mi_mm` are
    connected to it as `score_soft`'s mi is; the gradient is that of the function at fixed membership, so it ignores points that
    become visible or hidden, and it skips exactly the points the histogram skipped (the same mask).  mi_mm is a heuristic here."""
    who = 'score_soft_visible'
    if not isinstance(pool, bool):
        raise _C.EfghError('%s: pool: %r, expected True or False' % (who, pool))
    occ = _occlusion(who, occlusion)
    B, N, K, T, img, H, W, value, lo, hi = _checked(who, pc, img, cam_T_velo, value, value_range, bins, min_depth,
                                                    more=lambda B, K, H, W: _workspace(who, occ, B, K, H, W))
    if (B * N if pool else N) >= MAX_POINTS:
        raise _C.EfghError('%s: pc: %d points a histogram, at most 2^23 - 1 (a point adds 256 to a 32-bit cell)' % (who, B * N if pool else N))
    Hc, Wc = occ.grid(H, W)

    dev = pc.device
    L, st = _C.lib(), _C.stream_ptr
    bins, pool_i, nh = int(bins), int(pool), (K if pool else B * K)
    lead = (K,) if pool else (B, K)
    min_depth = float(min_depth)
    with torch.cuda.device(dev):
        pc, value, P, img = _kernel_inputs(pc, value, T, img)
        mask, zmin = _mask(L, st, pc, P, B, N, K, H, W, Hc, Wc, occ, min_depth)
        hist = torch.empty(lead + (bins, bins), dtype=torch.int32, device=dev)
        out = torch.empty(lead + (5,), dtype=torch.float64, device=dev)
        total = torch.empty(lead, dtype=torch.int32, device=dev)
        ocp = torch.empty(lead + (3,), dtype=torch.int32, device=dev)
        _C.check(L.efgh_score_soft_hist_masked(_C.ptr(pc), pc.stride(0), pc.stride(1), B, N, _C.ptr(value), value.stride(0), _C.ptr(P), K,
                                               _C.ptr(img), H, W, bins, lo, hi, min_depth, pool_i, _C.ptr(mask), _C.ptr(hist), st()))
        _C.check(L.efgh_score_mi(_C.ptr(hist), 1 if pool else B, K, bins, _C.ptr(out), _C.ptr(total), st()))
        _C.check(L.efgh_score_occupancy(_C.ptr(hist), nh, bins, _C.ptr(ocp), st()))
        count = torch.div(total, FRAC, rounding_mode='floor')

    def grad_of_P():
        with torch.cuda.device(dev):
            n_chunk = -(-N // int(L.efgh_score_chunk()))
            table = torch.empty((nh, bins, bins), dtype=torch.float64, device=dev)
            flag = torch.empty((nh, bins, bins), dtype=torch.uint8, device=dev)
            tot = torch.empty((nh,), dtype=torch.int32, device=dev)
            part = torch.empty((B, K, n_chunk, 12), dtype=torch.float64, device=dev)
            G = torch.empty((B, K, 3, 4), dtype=torch.float64, device=dev)
            _C.check(L.efgh_score_soft_table(_C.ptr(hist), nh, bins, _C.ptr(table), _C.ptr(flag), _C.ptr(tot), st()))
            _C.check(L.efgh_score_soft_grad_masked(_C.ptr(pc), pc.stride(0), pc.stride(1), B, N, _C.ptr(value), value.stride(0), _C.ptr(P), K,
                                                   _C.ptr(img), H, W, bins, lo, hi, min_depth, pool_i, _C.ptr(table), _C.ptr(flag),
                                                   _C.ptr(tot), _C.ptr(mask), _C.ptr(part), st()))
            _C.check(L.efgh_score_soft_fold(_C.ptr(part), B, K, n_chunk, _C.ptr(G), st()))
        return G

    fields = {k: out[..., i] for i, k in enumerate(BY)}
    if cam_T_velo.requires_grad and torch.is_grad_enabled():
        fields['mi'] = _SoftMI.apply(cam_T_velo, fields['mi'], grad_of_P, pool)
    with torch.cuda.device(dev):
        mm = _mi_mm(fields['mi'], count, ocp)
    return VisibleScore(count=count, hist=hist if want_hist else None, mi_mm=mm, occupancy=ocp, mask=mask if want_mask else None,
                        zmin=zmin.view(torch.float32) if want_mask else None, **fields)
