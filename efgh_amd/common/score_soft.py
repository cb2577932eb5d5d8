"""The differentiable form of `score` and a local pose refinement on it (csrc/score_soft.hip).  `score`'s
histogram is hard - nearest pixel, integer grey bin - so its MI is piecewise constant in the pose.  Here the grey level is sampled
bilinearly and spread linearly over two neighbouring grey cells (a first-order Parzen window, Mattes' formulation of Pandey et al.'s
objective), which gives the MI an analytic gradient with respect to the projection matrix.  Not in the reference; off unless called.

    s = score_soft(pcd, image, P.requires_grad_())     # Score; s.mi (B,K) float64 carries the gradient to P
    s.mi.sum().backward()                              # P.grad (B,K,3,4)
    r = refine(pcd, image, pred['cam_T_velo'])         # Adam on six rigid parameters a sample
    r.pose, r.mi, r.start_mi, r.best_iter, r.trace

The gradient is the derivative of the UNQUANTISED function (the weights are rounded to 1/256 for the integer histogram) at fixed
membership: it ignores points that enter or leave the frame, and it is zero where the grey coordinate is clamped.  Everything `score`
says about occlusion, about the bias of a sparse histogram and about what was measured holds here too: the depth test per candidate
is `score_soft_visible`, the correction `miller_madow` (both score_vis.py), and `refine` takes the former as its `scorer`."""
import math

import torch

from .. import _C
from .score import BY, Score, _checked, _kernel_inputs, _rigid

FRAC = 256               # weight resolution of the soft histogram: a point adds FRAC to it
MAX_POINTS = 1 << 23     # points of one histogram: FRAC times as much stays below 2^31


class _SoftMI(torch.autograd.Function):
    """mi as a function of cam_T_velo: the forward hands through what the kernels computed, the backward runs table, grad and fold"""
    @staticmethod
    def forward(ctx, T, mi, grad_of_P, pool):
        ctx.grad_of_P, ctx.pool, ctx.shape, ctx.dtype = grad_of_P, pool, T.shape, T.dtype
        return mi.clone()

    @staticmethod
    def backward(ctx, g):
        G = ctx.grad_of_P()                                      # (B,K,3,4) float64
        g = g.to(torch.float64)
        G = G * (g[None, :, None, None] if ctx.pool else g[:, :, None, None])
        return G.reshape(ctx.shape).to(ctx.dtype), None, None, None


def score_soft(pc, img, cam_T_velo, value=None, value_range=(0.0, 1.0), bins=32, min_depth=0.0, pool=False, want_hist=False):
    """`score`'s arguments and its checks -> Score on the soft histogram.  `count` is the number of points (the histogram's total //
    256), `hist` int32 holds 256 a point.  pool=True sums the samples' histograms into one per candidate: every field is (K,), hist
    (K,bins,bins), and B * N must stay below 2^23 (unpooled: N).  Where cam_T_velo requires grad, `mi` is connected to it (a float32
    or float64 leaf; the backward launches three kernels and multiplies by the incoming gradient with torch ops); nmi and the
    entropies are detached.  Without it only the histogram and efgh_score_mi launch.  Nothing is read back to the host."""
    who = 'score_soft'
    if not isinstance(pool, bool):
        raise _C.EfghError('%s: pool: %r, expected True or False' % (who, pool))
    B, N, K, T, img, H, W, value, lo, hi = _checked(who, pc, img, cam_T_velo, value, value_range, bins, min_depth)
    if (B * N if pool else N) >= MAX_POINTS:
        raise _C.EfghError('%s: pc: %d points a histogram, at most 2^23 - 1 (a point adds 256 to a 32-bit cell)' % (who, B * N if pool else N))

    dev = pc.device
    L, st = _C.lib(), _C.stream_ptr
    bins, pool_i, nh = int(bins), int(pool), (K if pool else B * K)
    lead = (K,) if pool else (B, K)
    with torch.cuda.device(dev):
        pc, value, P, img = _kernel_inputs(pc, value, T, img)
        hist = torch.empty(lead + (bins, bins), dtype=torch.int32, device=dev)
        out = torch.empty(lead + (5,), dtype=torch.float64, device=dev)
        total = torch.empty(lead, dtype=torch.int32, device=dev)
        min_depth = float(min_depth)
        _C.check(L.efgh_score_soft_hist(_C.ptr(pc), pc.stride(0), pc.stride(1), B, N, _C.ptr(value), value.stride(0), _C.ptr(P), K,
                                        _C.ptr(img), H, W, bins, lo, hi, min_depth, pool_i, _C.ptr(hist), st()))
        _C.check(L.efgh_score_mi(_C.ptr(hist), 1 if pool else B, K, bins, _C.ptr(out), _C.ptr(total), st()))
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
            _C.check(L.efgh_score_soft_grad(_C.ptr(pc), pc.stride(0), pc.stride(1), B, N, _C.ptr(value), value.stride(0), _C.ptr(P), K,
                                            _C.ptr(img), H, W, bins, lo, hi, min_depth, pool_i, _C.ptr(table), _C.ptr(flag), _C.ptr(tot),
                                            _C.ptr(part), st()))
            _C.check(L.efgh_score_soft_fold(_C.ptr(part), B, K, n_chunk, _C.ptr(G), st()))
        return G

    fields = {k: out[..., i] for i, k in enumerate(BY)}
    if cam_T_velo.requires_grad and torch.is_grad_enabled():
        fields['mi'] = _SoftMI.apply(cam_T_velo, fields['mi'], grad_of_P, pool)
    return Score(count=count, hist=hist if want_hist else None, **fields)


class Refined:
    """device tensors of one `refine` call: pose float64 (B,3,4), the iterate with the largest mi | mi, start_mi float64 (B,), or
    (1,) pooled | trace float64 (iters, B) or (iters, 1): mi of every iterate | best_iter int64, like mi"""
    __slots__ = ('pose', 'mi', 'start_mi', 'trace', 'best_iter')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def refine(pc, img, P0, value=None, value_range=(0.0, 1.0), bins=32, iters=100, rot_step_deg=0.2, trans_step=0.02, dof=(1,) * 6, pool=False,
           scorer=score_soft):
    """P0 (B,3,4) of either float width, the pose to start from; pc, img, value, value_range, bins as in `score_soft` -> Refined.
    Maximises `scorer(...).mi` over six rigid parameters z a sample (one set for the whole batch with pool=True): three Euler angles
    and a translation of the LiDAR frame, P = P0 D(z * step) with D = [Rz Ry Rx | t] as in `candidates_around`, step = rot_step_deg
    (degrees) and trans_step (metres) times dof (a 0 freezes an axis).  torch.optim.Adam(lr=1) on -mi, so an iteration moves an
    axis by about its step; z lives in float64 on P0's device and nothing is read back to the host inside the loop.  Iterate 0 is
    P0 itself, bit for bit.

    It is a LOCAL optimiser: it climbs from P0 and stops at the nearest maximum of a function that has many, so start it from a
    pose that is already close (the network's, yesterday's extrinsics, the best of `candidates_around`).  The default scorer has
    no occlusion test; `scorer=functools.partial(score_soft_visible, occlusion=Occlusion(...))` (score_vis.py) scores every iterate
    on the points visible under it.  MI of a sparse histogram is biased upwards, so histograms of very different `count` are not
    comparable - an iterate that pushes points out of the frame can score higher for that alone; `refine` climbs the uncorrected
    `mi` (the Miller-Madow term of score_vis.py is piecewise constant in the pose).  No effect on registration accuracy is claimed
    or was measured."""
    who = 'refine'
    if not torch.is_tensor(P0) or P0.dim() != 3 or tuple(P0.shape[1:]) != (3, 4) or P0.dtype not in (torch.float32, torch.float64):
        raise _C.EfghError('%s: P0: expected a float (B,3,4) tensor, got %s'
                           % (who, '%s %s' % (P0.dtype, tuple(P0.shape)) if torch.is_tensor(P0) else type(P0).__name__))
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

    f64 = dict(dtype=torch.float64, device=P0.device)
    B = P0.shape[0]
    start = P0.detach().to(torch.float64)
    scale = torch.tensor([s * f for s, f in zip(step, free)], **f64)
    z = torch.zeros((1 if pool else B, 6), requires_grad=True, **f64)
    opt = torch.optim.Adam([z], lr=1.0)
    kw = dict(value=value, value_range=value_range, bins=bins)
    if pool:
        kw['pool'] = True
    trace = torch.empty((iters, z.shape[0]), **f64)
    best_mi = best_iter = best_pose = None
    for it in range(iters):
        opt.zero_grad(set_to_none=True)
        p = z * scale
        P = torch.matmul(start, _rigid(p[:, :3], p[:, 3:]))        # (B,3,4) x (B or 1,4,4)
        mi = scorer(pc, img, P, **kw).mi.reshape(-1)                # (B,), or (1,) pooled
        now, pose = mi.detach(), P.detach()
        trace[it] = now
        if it == 0:
            best_mi, best_pose, best_iter = now.clone(), start.clone(), torch.zeros_like(now, dtype=torch.int64)   # P0, not P0 times a computed identity
        else:
            better = now > best_mi
            best_mi = torch.where(better, now, best_mi)
            best_iter = torch.where(better, torch.full_like(best_iter, it), best_iter)
            best_pose = torch.where(better.expand(B)[:, None, None], pose, best_pose)
        if it + 1 < iters:                                          # (the last iterate has been scored: no step leads anywhere)
            (-mi.sum()).backward()
            opt.step()
    return Refined(pose=best_pose, mi=best_mi, start_mi=trace[0].clone(), trace=trace, best_iter=best_iter)
