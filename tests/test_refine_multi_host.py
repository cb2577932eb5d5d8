"""tests/refine_contract.py held to things that are not taken from it (no GPU): its chain rule against central differences in
numpy.longdouble, its step against torch.optim.Adam + score._rigid + autograd (the arithmetic `refine` runs), frozen axes and zero
gradients, the selection's tie and NaN rules, the multi-start property on the peak scene; and the argument refusals of
`refine_multi` and `search`, which need no device."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_contract as RC  # noqa: E402
import score_soft_contract as SS  # noqa: E402
from test_score_host import PEAK, peak_case  # noqa: E402
from test_score_soft_host import STARTS, reprojection_offset, start_pose  # noqa: E402
from efgh_amd.common import MultiRefined, Searched, refine_multi, search  # noqa: E402  (the feature under test: no CPU path, but it imports and checks)
from efgh_amd.common.score import _rigid  # noqa: E402

SCALE = [math.radians(0.2)] * 3 + [0.02] * 3     # `refine`'s default steps
# a start outside the basin of the peak scene, found here on the CPU: 2.5 x STARTS[1] (test_the_best_of_many_starts has the figures)
FAR = [2.5 * x for x in STARTS[1]]
W12 = np.arange(1.0, 13.0).reshape(3, 4)         # the smooth `linear` scorer of test_score_soft_host.py: mi = sum(P * W12)


def poses(B, S, seed):
    """(B,S,3,4) pinhole-like matrices of mixed magnitudes"""
    rs = np.random.RandomState(seed)
    base = np.array([[40.0, 0, 32, 0.3], [0, 40.0, 24, -0.2], [0, 0, 1.0, 0.1]])
    return base + rs.randn(B, S, 3, 4) * np.array([5.0, 5.0, 5.0, 1.0])


def objective_ld(G, Pstart, p):
    """sum_b sum_ij G (Pstart D(p)) in numpy.longdouble, D from its definition (three elementary rotations multiplied out)"""
    ld = np.longdouble
    p = [ld(x) for x in p]
    c, s = [np.cos(x) for x in p[:3]], [np.sin(x) for x in p[:3]]
    o, l = ld(0), ld(1)
    Rx = np.array([[l, o, o], [o, c[0], -s[0]], [o, s[0], c[0]]], dtype=ld)
    Ry = np.array([[c[1], o, s[1]], [o, l, o], [-s[1], o, c[1]]], dtype=ld)
    Rz = np.array([[c[2], -s[2], o], [s[2], c[2], o], [o, o, l]], dtype=ld)
    D = np.zeros((4, 4), dtype=ld)
    D[:3, :3] = Rz.dot(Ry).dot(Rx)
    D[:3, 3] = p[3:]
    D[3, 3] = l
    return sum((G[b].astype(ld) * Pstart[b].astype(ld).dot(D)).sum() for b in range(G.shape[0]))


@pytest.mark.parametrize('pooled', [False, True])
def test_chain_rule_against_central_differences(pooled):
    """h = 2^-20.  A term of the objective is a product of at most three sines and cosines times G A, so its third derivative is at
    most 27 times the term and the central difference is off by h^2 / 6 * 27 * 2 = 9 h^2 of the magnitude sum |G_ij| sum_k |A_ik|;
    its own rounding is about 30 operations of longdouble eps, divided by h"""
    B, S = 3, 4
    rs = np.random.RandomState(11 + pooled)
    G, Pstart = rs.randn(B, S, 3, 4), poses(B, S, 5)
    G[0, 1] = 0.0
    ld_eps = float(np.finfo(np.longdouble).eps)
    h = 2.0 ** -20
    for case in ('zero', 'random', 'large'):
        z = np.zeros((1 if pooled else B, S, 6)) if case == 'zero' else rs.randn(1 if pooled else B, S, 6) * (3.0 if case == 'random' else 300.0)
        got, bound = RC.chain_rule(G, Pstart, z, SCALE)
        worst = 0.0
        for zb in range(z.shape[0]):
            for s in range(S):
                bs = range(B) if pooled else [zb]
                p = z[zb, s] * np.array(SCALE)
                mag = sum((np.abs(G[b, s]) * np.abs(Pstart[b, s, :, :3]).sum(1, keepdims=True)).sum() for b in bs)
                for a in range(6):
                    e = np.zeros(6)
                    e[a] = h
                    fd = (objective_ld(G[list(bs), s], Pstart[list(bs), s], p + e) - objective_ld(G[list(bs), s], Pstart[list(bs), s], p - e)) / (2 * np.longdouble(h))
                    err = abs(float(got[zb, s, a] - np.longdouble(SCALE[a]) * fd))
                    tol = bound[zb, s, a] + SCALE[a] * (9 * h * h + 30 * ld_eps / h) * mag
                    worst = max(worst, err / tol if tol > 0 else (0.0 if err == 0 else np.inf))
        print('%s, pooled %s: largest error / tolerance %.3f' % (case, pooled, worst))
        assert worst <= 1.0
    if not pooled:
        assert (got[0, 1] == 0).all() and (bound[0, 1] == 0).all()      # the all-zero G row


def torch_loop(start, W, scale, pool, iters):
    """`refine`'s own loop on the CPU with the linear scorer -> per iterate: z, m, v BEFORE its step, the pose, dmi, and z, m, v after"""
    start = torch.from_numpy(start)
    B = start.shape[0]
    sc = torch.tensor(scale, dtype=torch.float64)
    z = torch.zeros((1 if pool else B, 6), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([z], lr=1.0)
    out = []
    for it in range(iters):
        opt.zero_grad(set_to_none=True)
        p = z * sc
        P = torch.matmul(start, _rigid(p[:, :3], p[:, 3:]))
        mi = (P * torch.from_numpy(W)).sum((1, 2))
        stt = opt.state.get(z, {})
        rec = dict(z=z.detach().numpy().copy(), m=stt['exp_avg'].numpy().copy() if stt else np.zeros(z.shape),
                   v=stt['exp_avg_sq'].numpy().copy() if stt else np.zeros(z.shape), P=P.detach().numpy().copy())
        (-mi.sum()).backward()
        rec['dmi'] = -z.grad.numpy().copy()
        opt.step()
        stt = opt.state[z]
        rec.update(z1=z.detach().numpy().copy(), m1=stt['exp_avg'].numpy().copy(), v1=stt['exp_avg_sq'].numpy().copy())
        out.append(rec)
    return out


@pytest.mark.parametrize('pool', [False, True])
def test_the_step_against_torch_adam_and_autograd(pool):
    """the contract's first iterates from a fresh state against torch.optim.Adam + _rigid + autograd, each step from torch's own state
    before it: the gradient, m, v, z and the next pose inside the contract's bounds"""
    B = 3
    start = poses(B, 1, 21)
    W = np.broadcast_to(W12, (B, 1, 3, 4)).copy()
    recs = torch_loop(start[:, 0], W12, SCALE, pool, 3)
    lead = (1, 1) if pool else (B, 1)
    for it in range(2):
        r, nxt = recs[it], recs[it + 1]
        st = RC.new_state(B, 1, pool, 3)
        st['z'], st['m'], st['v'] = r['z'].reshape(lead + (6,)), r['m'].reshape(lead + (6,)), r['v'].reshape(lead + (6,))
        mi = (r['P'] * W12).sum((1, 2))
        mi = np.array([[mi.sum()]]) if pool else mi.reshape(lead)
        out = RC.step(st, W, start, r['P'][:, None], mi, SCALE, it)
        for name, got, ref, bound in (('dMI/dz', out['dmi'], r['dmi'], out['ddmi']), ('m', st['m'], r['m1'], out['dm']), ('v', st['v'], r['v1'], out['dv']),
                                      ('z', st['z'], r['z1'], out['dz']), ('pose', out['P'], nxt['P'][:, None], out['dP'])):
            err = np.abs(got - ref.reshape(got.shape))
            print('step %d %s: largest error %.3e, its bound %.3e, smallest bound / error %.1f'
                  % (it + 1, name, err.max(), bound.flat[err.argmax()], (bound[err > 0] / err[err > 0]).min() if (err > 0).any() else np.inf))
            assert np.abs(ref).max() > 0 and (err <= bound).all(), (it, name)
        assert (np.abs(st['z']) > 0.5).all()                     # an Adam step of lr 1 moves every axis by about one
    # iterate 0 of the contract's own loop is the start, bit for bit, and its first step is the one above
    mine = RC.refine_multi(lambda P: ((P * W12).sum((2, 3)).sum(0) if pool else (P * W12).sum((2, 3)), W), start, 3, SCALE, pool=pool)
    assert (mine['best_iter'] == 2).all() and (np.diff(mine['trace'], axis=0) > 0).all()      # linear: every step climbs
    assert np.abs(mine['pose'][:, 0] - recs[2]['P']).max() <= 1e-9 * np.abs(start).max()


def test_frozen_axes_and_zero_gradients_move_nothing():
    B, S = 2, 3
    start = poses(B, S, 31)
    G = np.random.RandomState(32).randn(B, S, 3, 4)
    G[:, 1] = 0.0                                                # start 1: no gradient at all
    scale = [SCALE[0], 0.0, SCALE[2], 0.0, SCALE[4], 0.0]
    st = RC.new_state(B, S, False, 4)
    P = start.copy()
    for it in range(3):
        out = RC.step(st, G, start, P, np.full((B, S), float(it)), scale, it)
        P = out['P']
        assert (st['z'][..., [1, 3, 5]] == 0).all() and (st['m'][..., [1, 3, 5]] == 0).all() and (st['v'][..., [1, 3, 5]] == 0).all()
        assert (st['z'][:, [0, 2]][..., [0, 2, 4]] != 0).all()
        assert (st['z'][:, 1] == 0).all() and (P[:, 1].view(np.int64) == start[:, 1].view(np.int64)).all() and (out['dP'][:, 1] == 0).all()
        assert np.isfinite(P).all()
    # a start with a NaN entry and no gradient stays put: the zero terms are never multiplied with it
    start[0, 1, 2, 1] = np.nan
    st = RC.new_state(B, S, False, 2)
    out = RC.step(st, G, start, start.copy(), np.zeros((B, S)), SCALE, 0)
    assert np.isfinite(st['z']).all() and (st['z'][0, 1] == 0).all() and (out['P'][0, 1].view(np.int64) == start[0, 1].view(np.int64)).all()
    # bookkeeping: strict improvement, the first of equals stays, a NaN never wins
    st = RC.new_state(1, 1, False, 4)
    Ps = [poses(1, 1, 40 + i) for i in range(4)]
    for it, mi in enumerate([1.0, 1.0, float('nan'), 2.0]):
        o = RC.step(st, G[:1, :1], start[:1, :1], Ps[it], np.array([[mi]]), SCALE, it, last=it == 3)
        assert bool(o['better'][0, 0]) == (it in (0, 3))
    assert st['best_iter'][0, 0] == 3 and st['best_mi'][0, 0] == 2.0 and (st['best_pose'] == Ps[3]).all() and np.isnan(st['trace'][2, 0, 0])


def test_selection_rules():
    nan = float('nan')
    v = np.array([[1.0, 3.0, 3.0, nan, -0.0, 0.0, 3.0, -np.inf, np.inf, nan]])
    assert RC.select(v, 10).tolist() == [[8, 1, 2, 6, 0, 4, 5, 7, 3, 9]]      # ties by ascending index; -0.0 equals 0.0; NaNs last, by index
    assert RC.select(v, 1).tolist() == [[8]]
    assert RC.select(np.array([[nan, nan, 1.0]]), 2).tolist() == [[2, 0]]
    assert RC.select(np.array([[5.0]]), 1).tolist() == [[0]]                   # K = 1
    assert RC.select(np.full((2, 7), 4.0), 7).tolist() == [list(range(7))] * 2  # all equal, keep = K
    rs = np.random.RandomState(3)
    w = rs.randn(3, 200)
    got = RC.select(w, 64)
    assert got.dtype == np.int32 and (got == np.argsort(-w, axis=1, kind='stable')[:, :64]).all()
    assert (RC.best(np.array([[1.0, 2.0, 2.0], [3.0, 1.0, 3.0]])) == [1, 0]).all()


def peak_scorer():
    pc, img, P, value = peak_case()

    def scorer(Pb):
        ref = SS.score_soft(pc, img, Pb, value, 0.0, 256.0, PEAK['bins'])
        return ref['mi'], ref['grad']
    return scorer, pc, P[0, 0]


def test_the_best_of_many_starts():
    """The multi-start property on the peak scene, bins 8, 200 iterations of the contract's loop with SS.score_soft as scorer, from
    STARTS[0], STARTS[1], the true pose and the far start FAR = 2.5 x STARTS[1] = (-0.2, 0.15, 0.125 rad; -0.75, 0.5, 0.5 m), which
    lies 12.68 px from the truth.  Measured here: the far start's own climb ends 14.28 px from the truth (mi 0.081 -> 0.146), the
    other three end at 0.05 .. 0.08 px (mi 1.169), and best() picks one of them."""
    scorer, pc, P0 = peak_scorer()
    off = lambda P: reprojection_offset(pc[0], P, P0, PEAK['h'], PEAK['w'])
    starts = np.stack([start_pose(P0, STARTS[0]), start_pose(P0, STARTS[1]), P0, start_pose(P0, FAR)])[None]
    r = RC.refine_multi(scorer, starts, 200, SCALE)
    ends = [off(r['pose'][0, s]) for s in range(4)]
    best = int(RC.best(r['mi'])[0])
    print('starts %s px -> ends %s px, mi %s, best() = %d' % (['%.2f' % off(starts[0, s]) for s in range(4)], ['%.3f' % e for e in ends],
                                                              ['%.4f' % v for v in r['mi'][0]], best))
    assert off(starts[0, 3]) <= 20.0 and ends[3] > 2.0           # the far start on its own does not get there
    assert best != 3 and ends[best] <= 0.5                       # the best of the four does
    assert max(ends[:3]) <= 0.5
    assert (r['trace'][0] == r['start_mi']).all() and (r['mi'] == r['trace'].max(0)).all() and (r['best_iter'] == r['trace'].argmax(0)).all()
    # starts are independent: the far start alone gives the same bits as the far start in company
    alone = RC.refine_multi(scorer, starts[:, 3:], 200, SCALE)
    assert (alone['trace'][:, 0, 0] == r['trace'][:, 0, 3]).all() and (alone['pose'][0, 0] == r['pose'][0, 3]).all()


def test_one_set_of_constants():
    """Adam's constants and the selection's limits are written down in the kernel file, its header, the wrapper and the contract:
    the four agree"""
    import re
    mod = sys.modules['efgh_amd.common.refine_multi']
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'efgh_amd', 'csrc')
    hip, hdr = open(os.path.join(csrc, 'refine.hip')).read(), open(os.path.join(csrc, 'refine.h')).read()
    b1, b2, eps = (float(x) for x in re.search(r'BETA1 = ([\d.e-]+), BETA2 = ([\d.e-]+), ADAM_EPS = ([\d.e-]+);', hip).groups())
    assert (b1, b2, eps) == (RC.BETA1, RC.BETA2, RC.ADAM_EPS) and (b1, b2) == (mod.BETA1, mod.BETA2)
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1.0).defaults
    assert (b1, b2) == tuple(opt['betas']) and eps == opt['eps']
    keep, most = int(re.search(r'EFGH_REFINE_MAX_KEEP = (\d+);', hdr).group(1)), int(re.search(r'EFGH_REFINE_MAX_S = (\d+);', hdr).group(1))
    from efgh_amd.common.score import MAX_CANDIDATES
    assert keep == mod.MAX_KEEP == RC.MAX_KEEP and most == MAX_CANDIDATES == RC.MAX_K


def test_arguments_are_checked_before_any_launch():
    from efgh_amd import _C
    pc, img = torch.zeros(2, 4, 5), torch.zeros(2, 4, 6, 3, dtype=torch.uint8)
    starts = torch.zeros(2, 3, 3, 4)
    calls = []
    spy = lambda *a, **kw: calls.append(1)
    for name, kw in (('starts', dict(starts=starts[0, 0])), ('starts', dict(starts=starts.long())), ('starts', dict(starts=None)),
                     ('starts', dict(starts=torch.zeros(2, 3, 4, 3))), ('starts', dict(starts=torch.zeros(2, 4097, 3, 4))),
                     ('iters', dict(iters=0)), ('iters', dict(iters=2.5)), ('iters', dict(iters=True)), ('rot_step_deg', dict(rot_step_deg=0.0)),
                     ('rot_step_deg', dict(trans_step=float('nan'))), ('rot_step_deg', dict(dof=(1, 1, 1))), ('pool', dict(pool=1)),
                     ('scorer', dict(scorer=None))):
        a = dict(starts=starts, scorer=spy)
        a.update(kw)
        with pytest.raises(_C.EfghError, match=r'refine_multi: %s\b' % name):
            refine_multi(pc, img, **a)
    with pytest.raises(_C.EfghError, match='S = 4097'):
        refine_multi(pc, img, torch.zeros(2, 4097, 3, 4), scorer=spy)
    with pytest.raises(_C.EfghError, match='CPU tensor'):          # everything valid but on the CPU: there is no CPU path
        refine_multi(pc, img, starts, scorer=spy)
    P0 = torch.zeros(2, 3, 4)
    grid = dict(rot_deg=(0.5, 0, 0), trans=(0.1, 0, 0))            # 9 candidates
    for name, kw in (('keep', dict(keep=0)), ('keep', dict(keep=10)), ('keep', dict(keep=2.0)), ('iters', dict(iters=0)), ('scorer', dict(scorer=None)),
                     ('pool', dict(pool=0))):
        a = dict(scorer=spy)
        a.update(kw)
        with pytest.raises(_C.EfghError, match=r'search: %s\b' % name):
            search(pc, img, P0, **grid, **a)
    with pytest.raises(_C.EfghError, match=r'search: keep: 65 of K = 81'):
        search(pc, img, P0, rot_deg=(0.5, 0.5, 0), trans=(0.1, 0.1, 0), keep=65, scorer=spy)
    with pytest.raises(_C.EfghError, match='candidates_around: P'):
        search(pc, img, P0[0], **grid, scorer=spy)
    assert calls == []                                             # no scorer ran: every refusal came first
    with pytest.raises(_C.EfghError, match=r'score_soft: pc: a CPU tensor'):      # the default scorer checks the rest, in front of any launch
        search(pc, img, P0, **grid)
    assert MultiRefined.__slots__ == ('pose', 'mi', 'start_mi', 'trace', 'best_iter') and Searched.__slots__ == ('coarse', 'kept', 'refined', 'pose')
