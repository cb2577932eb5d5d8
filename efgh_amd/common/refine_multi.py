"""Climbing the mutual information from MANY start poses at once, and the chain that joins the grid to the climb (csrc/refine.hip;
DESIGN 3).  `refine` is a local optimiser with one start a sample and about forty small torch launches an iteration
for arithmetic on six numbers.  Here the S starts ride on the K axis of the unchanged scoring kernels, and ONE launch of
efgh_refine_step an iteration does the chain rule from dMI/dP to the six rigid parameters, Adam, the next pose and the best-so-far
bookkeeping for every start.  Not in the reference; off unless called.

    starts = stage_poses(pred, calib)[0]                       # (B,S,3,4): any stack of poses
    r = refine_multi(pcd, image, starts)                       # MultiRefined; every start climbs on its own
    r.pose, r.mi, r.start_mi, r.best_iter, r.trace             # (B,S,3,4), (B,S) x 3, (iters,B,S)
    r.best(), r.best_pose()                                    # (B,) the start that ended highest, (B,3,4) where it ended
    f = search(pcd, image, pred['cam_T_velo'], rot_deg=(0.5,) * 3, trans=(0.05,) * 3, keep=8)
    f.pose, f.kept, f.coarse, f.refined                        # grid -> score -> the 8 best -> climb -> the best end

Everything `refine` says about itself holds here: the gradient is that of the unquantised function at FIXED membership, the
default scorer has no occlusion test (`scorer=functools.partial(score_soft_visible, occlusion=...)` adds one), histograms of very
different `count` are not comparable - a start that pushes points out of the frame can score higher for that alone, and `best()`
compares the uncorrected `mi` across starts.  No effect on registration accuracy is claimed or was measured: there is no dataset
here.  The arithmetic is tests/refine_contract.py's, which is `refine`'s up to the order of its roundings; the two do not give the
same bits beyond iterate 0."""
import math

import torch

from .. import _C
from .score import MAX_CANDIDATES, candidates_around
from .score_soft import score_soft

# tests/test_refine_multi_host.py holds these three to csrc/refine.h, csrc/refine.hip and tests/refine_contract.py
MAX_KEEP = 64            # EFGH_REFINE_MAX_KEEP: starts that efgh_refine_select hands on
BETA1, BETA2 = 0.9, 0.999


class MultiRefined:
    """device tensors of one `refine_multi` call: pose float64 (B,S,3,4), per start the iterate with the largest mi | mi, start_mi
    float64 and best_iter int64 (B,S), or (S,) pooled | trace float64 (iters,B,S) or (iters,S): mi of every iterate"""
    __slots__ = ('pose', 'mi', 'start_mi', 'trace', 'best_iter')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    def best(self):
        """int64 (B,), or () pooled: the start that ended with the largest mi (the first of equals), computed on the device"""
        return torch.argmax(self.mi, dim=-1)

    def best_pose(self):
        """float64 (B,3,4): `pose` at `best()`"""
        i = self.best()
        if self.mi.dim() == 1:                                   # (a 0-dim index would be read back by the host: index_select stays on the device)
            return self.pose.index_select(1, i.reshape(1))[:, 0]
        return self.pose[torch.arange(self.pose.shape[0], device=self.pose.device), i]


class Searched:
    """device tensors of one `search` call: coarse, the Score of the grid (fields (B,K), or (K,) pooled) | kept int32 (B,keep) or
    (keep,): the grid candidates that were climbed from, best first | refined, the MultiRefined of the climb | pose float64 (B,3,4)"""
    __slots__ = ('coarse', 'kept', 'refined', 'pose')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _steps(who, iters, rot_step_deg, trans_step, dof, pool, scorer):
    """`refine`'s checks of its own keywords, with its messages -> the six scales"""
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise _C.EfghError('%s: iters: %r, expected an integer >= 1' % (who, iters))
    try:
        step = [math.radians(float(rot_step_deg))] * 3 + [float(trans_step)] * 3
        free = [float(bool(d)) for d in dof]
    except (TypeError, ValueError):
        step, free = [], []
    if len(free) != 6 or not all(math.isfinite(v) and v > 0 for v in step):
        raise _C.EfghError('%s: rot_step_deg = %r and trans_step = %r: finite and positive; dof = %r: six flags' % (who, rot_step_deg, trans_step, dof))
    if not isinstance(pool, bool):
        raise _C.EfghError('%s: pool: %r, expected True or False' % (who, pool))
    if not callable(scorer):
        raise _C.EfghError('%s: scorer: expected a callable with the signature of score_soft' % who)
    return [s * f for s, f in zip(step, free)]


def _mi_rows(who, mi, rows, dev):
    """a scorer's mi as the kernels read it: float64, `rows` values, on the starts' device, unit stride"""
    if not torch.is_tensor(mi) or mi.dtype != torch.float64 or mi.numel() != rows or mi.device != dev:
        raise _C.EfghError('%s: scorer: its mi is %s, expected float64 with %d values on %s'
                           % (who, '%s %s on %s' % (mi.dtype, tuple(mi.shape), mi.device) if torch.is_tensor(mi) else type(mi).__name__, rows, dev))
    return mi if mi.is_contiguous() else mi.contiguous()


def refine_multi(pc, img, starts, value=None, value_range=(0.0, 1.0), bins=32, iters=100, rot_step_deg=0.2, trans_step=0.02, dof=(1,) * 6,
                 pool=False, scorer=score_soft):
    """starts (B,S,3,4), or (B,3,4) for S = 1, of either float width: any stack of poses (`stage_poses(pred, calib)[0]`,
    `candidates_around(...)`, yesterday's extrinsics next to today's prediction), S <= 4096; every other argument as in `refine`
    -> MultiRefined.  Every start climbs on its own, P[b,s] = starts[b,s] D(z[b,s] * step); with pool=True a start has one z for
    the whole batch and scores on the batch's pooled histogram.  Iterate 0 is `starts` itself, bit for bit.

    An iteration is one `scorer` call on the (B,S,3,4) pose buffer (a float64 leaf), torch.autograd.grad(mi.sum(), P) and ONE
    efgh_refine_step launch; no other torch op, no host read.  There is ONE pose buffer: `score_soft`'s backward reads it when it
    runs, so the step goes behind the gradient on the same stream and writes the next iterate in place.  Adam's two bias terms are
    formed here in Python floats and passed by value."""
    who = 'refine_multi'
    if not torch.is_tensor(starts) or starts.dim() not in (3, 4) or tuple(starts.shape[-2:]) != (3, 4) or starts.dtype not in (torch.float32, torch.float64) \
            or starts.shape[0] < 1 or (starts.dim() == 4 and starts.shape[1] < 1):
        raise _C.EfghError('%s: starts: expected a float (B,S,3,4) or (B,3,4) tensor, got %s'
                           % (who, '%s %s' % (starts.dtype, tuple(starts.shape)) if torch.is_tensor(starts) else type(starts).__name__))
    if starts.dim() == 3:
        starts = starts[:, None]
    B, S = starts.shape[:2]
    if S > MAX_CANDIDATES:
        raise _C.EfghError('%s: starts: S = %d starts, at most %d a call' % (who, S, MAX_CANDIDATES))
    s0, s1, s2, s3, s4, s5 = _steps(who, iters, rot_step_deg, trans_step, dof, pool, scorer)
    if torch.is_tensor(pc) and pc.device != starts.device:
        raise _C.EfghError('%s: starts: on %s, the cloud is on %s' % (who, starts.device, pc.device))
    _C.require_cuda(starts)

    dev = starts.device
    f64 = dict(dtype=torch.float64, device=dev)
    L, st = _C.lib(), _C.stream_ptr
    rows = S if pool else B * S
    lead = (S,) if pool else (B, S)
    kw = dict(value=value, value_range=value_range, bins=bins)
    if pool:
        kw['pool'] = True
    with torch.cuda.device(dev):
        start = starts.detach().to(torch.float64).contiguous()   # float32 -> float64 is exact
        P = start.clone().requires_grad_()
        z, m, v = (torch.zeros((rows, 6), **f64) for _ in range(3))
        best_mi, best_iter, best_pose = torch.empty(lead, **f64), torch.empty(lead, dtype=torch.int64, device=dev), torch.empty((B, S, 3, 4), **f64)
        trace = torch.empty((iters,) + lead, **f64)
        for it in range(iters):
            last = it + 1 == iters
            mi = scorer(pc, img, P, **kw).mi
            G = None
            if not last:                                         # (the last iterate has been scored: no step leads anywhere)
                (G,) = torch.autograd.grad(mi.sum(), P)
                if G.dtype != torch.float64 or not G.is_contiguous():
                    G = G.to(torch.float64).contiguous()
            mi = _mi_rows(who, mi.detach(), rows, dev)
            t = it + 1
            _C.check(L.efgh_refine_step(_C.ptr(G), _C.ptr(start), _C.ptr(P), _C.ptr(mi), B, S, int(pool), _C.ptr(z), _C.ptr(m), _C.ptr(v),
                                        _C.ptr(best_mi), _C.ptr(best_iter), _C.ptr(best_pose), _C.ptr(trace), s0, s1, s2, s3, s4, s5, it,
                                        1.0 / (1.0 - BETA1 ** t), math.sqrt(1.0 - BETA2 ** t), int(last), st()))
    return MultiRefined(pose=best_pose, mi=best_mi, start_mi=trace[0].clone(), trace=trace, best_iter=best_iter)


def select(val, keep):
    """val float64 (rows,K) or (K,) on the device, K <= 4096, keep <= min(K, 64) -> int32 (rows,keep) or (keep,): the keep largest of a
    row in descending order, equal values by ascending index, a NaN below every number (efgh_refine_select)"""
    who = 'select'
    if not torch.is_tensor(val) or val.dtype != torch.float64 or val.dim() not in (1, 2) or val.numel() < 1:
        raise _C.EfghError('%s: val: expected a float64 (rows,K) or (K,) tensor, got %s'
                           % (who, '%s %s' % (val.dtype, tuple(val.shape)) if torch.is_tensor(val) else type(val).__name__))
    K = val.shape[-1]
    if K > MAX_CANDIDATES:
        raise _C.EfghError('%s: val: K = %d values a row, at most %d' % (who, K, MAX_CANDIDATES))
    if isinstance(keep, bool) or not isinstance(keep, int) or keep < 1 or keep > min(K, MAX_KEEP):
        raise _C.EfghError('%s: keep: %r of K = %d, expected an integer in 1 .. min(K, %d)' % (who, keep, K, MAX_KEEP))
    _C.require_cuda(val)
    rows = 1 if val.dim() == 1 else val.shape[0]
    with torch.cuda.device(val.device):
        val = val.detach().contiguous()
        idx = torch.empty(val.shape[:-1] + (keep,), dtype=torch.int32, device=val.device)
        _C.check(_C.lib().efgh_refine_select(_C.ptr(val), rows, K, keep, _C.ptr(idx), _C.stream_ptr()))
    return idx


def search(pc, img, P0, rot_deg, trans, steps=1, keep=8, value=None, value_range=(0.0, 1.0), bins=32, iters=100, rot_step_deg=0.2,
           trans_step=0.02, dof=(1,) * 6, pool=False, scorer=score_soft):
    """P0 (B,3,4), rot_deg, trans, steps as in `candidates_around`; keep <= min(K, 64) grid candidates to climb from; the rest as in
    `refine_multi` -> Searched.  In order: the grid around P0; ONE gradient-free `scorer` call on it (pooled if `pool`);
    efgh_refine_select on its mi; a gather of the kept poses; `refine_multi` from them; `pose` is its `best_pose()`.  Nothing is read
    back to the host.  Candidate 0 of the grid is P0 itself: if it ranks among the kept, the pose handed back never scores below
    what `refine` would have been started from."""
    who = 'search'
    _steps(who, iters, rot_step_deg, trans_step, dof, pool, scorer)
    cands = candidates_around(P0, rot_deg, trans, steps)         # (B,K,3,4) float64; its own checks and messages
    B, K = cands.shape[:2]
    if isinstance(keep, bool) or not isinstance(keep, int) or keep < 1 or keep > min(K, MAX_KEEP):
        raise _C.EfghError('%s: keep: %r of K = %d, expected an integer in 1 .. min(K, %d)' % (who, keep, K, MAX_KEEP))
    kw = dict(value=value, value_range=value_range, bins=bins)
    if pool:
        kw['pool'] = True
    with torch.no_grad():
        coarse = scorer(pc, img, cands, **kw)
    if not hasattr(coarse, 'mi'):
        raise _C.EfghError('%s: scorer: expected a callable with the signature of score_soft' % who)
    mi = _mi_rows(who, coarse.mi, K if pool else B * K, cands.device).reshape((K,) if pool else (B, K))
    kept = select(mi, keep)
    with torch.cuda.device(cands.device):
        i = kept.to(torch.int64)
        starts = cands[:, i] if pool else cands[torch.arange(B, device=cands.device)[:, None], i]
    refined = refine_multi(pc, img, starts, value=value, value_range=value_range, bins=bins, iters=iters, rot_step_deg=rot_step_deg,
                           trans_step=trans_step, dof=dof, pool=pool, scorer=scorer)
    return Searched(coarse=coarse, kept=kept, refined=refined, pose=refined.best_pose())
