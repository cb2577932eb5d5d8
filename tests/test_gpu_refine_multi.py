"""csrc/refine.hip against tests/refine_contract.py: one teacher-forced efgh_refine_step through the library - z, m, v and the next
pose inside the bounds the contract derives (never fitted to an output), every bookkeeping decision and copy EXACTLY -, the selection
EXACTLY, and `refine_multi` / `search` on the device: iterate 0, independent starts, the peak scene, a visible-points scorer, two
runs bit for bit, starts that see nothing, the refusals with guard buffers."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_contract as RC  # noqa: E402
from test_score_host import PEAK, peak_case  # noqa: E402
from test_score_soft_host import STARTS, reprojection_offset, start_pose  # noqa: E402
from test_refine_multi_host import FAR, SCALE, poses  # noqa: E402

pytestmark = pytest.mark.gpu
FROZEN = [SCALE[0], 0.0, SCALE[2], SCALE[3], 0.0, SCALE[5]]


def _api():
    import efgh_amd.common as C
    return C


def _bits(t):
    return t.contiguous().view(torch.int64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _launch_step(G, Pstart, P, mi, B, S, pool, st, scale, it, last):
    from efgh_amd import _C
    ss, bc2 = RC.bias_terms(it + 1)
    _C.check(_C.lib().efgh_refine_step(_C.ptr(G), _C.ptr(Pstart), _C.ptr(P), _C.ptr(mi), B, S, int(pool), _C.ptr(st['z']), _C.ptr(st['m']),
                                       _C.ptr(st['v']), _C.ptr(st['best_mi']), _C.ptr(st['best_iter']), _C.ptr(st['best_pose']), _C.ptr(st['trace']),
                                       *scale, it, ss, bc2, int(last), _C.stream_ptr()))


def _forced_case(B, S, pool, it, scale, seed):
    """a random state in the middle of a climb, as the contract's dict (numpy): rows that never moved and have no gradient, rows
    with an all-zero G, mi equal to best_mi, mi above and below it, a NaN mi"""
    rs = np.random.RandomState(seed)
    Z0 = 1 if pool else B
    st = RC.new_state(B, S, pool, it + 1)
    st['z'], st['m'], st['v'] = rs.randn(Z0, S, 6) * 3.0, rs.randn(Z0, S, 6) * 0.1, rs.rand(Z0, S, 6) * 0.01
    st['best_mi'] = rs.rand(Z0, S)
    st['best_iter'] = rs.randint(0, it, (Z0, S)).astype(np.int64)
    st['best_pose'] = rs.randn(B, S, 3, 4)
    st['trace'][:] = -7.0
    G, Pstart, P = rs.randn(B, S, 3, 4) * 0.01, poses(B, S, seed + 1), poses(B, S, seed + 2)
    mi = rs.rand(Z0, S)
    kind = rs.randint(0, 6, (Z0, S))
    if S == 1:
        kind[:] = seed % 6
    mi[kind == 0] = st['best_mi'][kind == 0]                      # equal: no update may happen
    mi[kind == 1] = np.nan
    quiet = kind == 2                                            # never moved, no gradient: stays on the start
    for k in ('z', 'm', 'v'):
        st[k][quiet] = 0.0
        st[k][..., [a for a in range(6) if scale[a] == 0.0]] = 0.0      # a frozen axis has never had a gradient
    G[np.broadcast_to(quiet | (kind == 3), (B, S))] = 0.0        # kind 3: an all-zero G row with momentum left
    G[:, :, 1, 2][np.broadcast_to(kind == 4, (B, S))] = 0.0       # single zero entries
    return st, G, Pstart, P, mi, quiet


def _forced(B, S, pool, it, scale, seed):
    st, G, Pstart, P, mi, quiet = _forced_case(B, S, pool, it, scale, seed)
    rows = S if pool else B * S
    for last in (False, True):
        dst = {k: _dev(v.reshape((rows, 6)) if k in 'zmv' else v) for k, v in st.items()}
        dG, dS, dP, dmi = _dev(G), _dev(Pstart), _dev(P), _dev(mi)
        keep = {k: v.clone() for k, v in dst.items()}
        _launch_step(dG, dS, dP, dmi, B, S, pool, dst, scale, it, last)
        ref = {k: v.copy() for k, v in st.items()}
        out = RC.step(ref, G, Pstart, P, mi, scale, it, last=last)
        # bookkeeping: exact
        got_iter = dst['best_iter'].cpu().numpy().reshape(ref['best_iter'].shape)
        assert (got_iter == ref['best_iter']).all() and ((got_iter == it) == out['better']).all()
        assert out['better'].any() or S == 1
        assert torch.equal(_bits(dst['best_mi']), _bits(_dev(ref['best_mi'])).reshape(dst['best_mi'].shape))
        assert torch.equal(_bits(dst['best_pose']), _bits(_dev(ref['best_pose'])))
        tr = dst['trace'].cpu().numpy()
        assert np.array_equal(tr[it], mi, equal_nan=True) and (tr[:it] == -7.0).all()
        assert torch.equal(dG, _dev(G)) and torch.equal(dS, _dev(Pstart)) and torch.equal(_bits(dmi), _bits(_dev(mi)))      # inputs unwritten
        if last:                                                 # the bookkeeping only
            assert all(torch.equal(dst[k], keep[k]) for k in 'zmv') and torch.equal(dP, _dev(P))
            continue
        worst = np.inf
        for k, bound in (('z', out['dz']), ('m', out['dm']), ('v', out['dv'])):
            got = dst[k].cpu().numpy().reshape(ref[k].shape)
            err = np.abs(got - ref[k])
            assert np.isfinite(got).all() and (err <= bound).all(), (k, err.max(), bound.flat[err.argmax()])
            if (err > 0).any():
                worst = min(worst, (bound[err > 0] / err[err > 0]).min())
        got = dP.cpu().numpy()
        err = np.abs(got - out['P'])
        assert np.isfinite(got).all() and (err <= out['dP']).all(), ('pose', err.max(), out['dP'].flat[err.argmax()])
        if (err > 0).any():
            worst = min(worst, (out['dP'][err > 0] / err[err > 0]).min())
        print('B %d S %d pool %d it %d: smallest bound / error %.1f' % (B, S, pool, it, worst))
        frozen = [a for a in range(6) if scale[a] == 0.0]
        assert all((dst[k].cpu().numpy()[:, frozen] == 0).all() for k in 'zmv')
        q = np.broadcast_to(quiet, (B, S))
        assert (got[q].view(np.int64) == Pstart[q].view(np.int64)).all() and (dst['z'].cpu().numpy().reshape(quiet.shape + (6,))[quiet] == 0).all()


@pytest.mark.parametrize('S', [1, 63, 64, 65, 257, 4096])
def test_one_step_teacher_forced(S):
    its = (1, 2, 1000)
    j = [1, 63, 64, 65, 257, 4096].index(S)
    _forced(1, S, False, its[j % 3], SCALE, 100 + j)
    _forced(3, S, False, its[(j + 1) % 3], FROZEN if j % 2 else SCALE, 200 + j)
    _forced(3, S, True, its[(j + 2) % 3], SCALE if j % 2 else FROZEN, 300 + j)


def test_a_frozen_axis_stays_zero_from_a_fresh_state():
    B, S = 2, 65
    G, Pstart = np.random.RandomState(5).randn(B, S, 3, 4), poses(B, S, 6)
    st = RC.new_state(B, S, False, 3)
    dst = {k: _dev(v.reshape((B * S, 6)) if k in 'zmv' else v) for k, v in st.items()}
    dP, dS = _dev(Pstart), _dev(Pstart)
    for it in range(2):
        _launch_step(_dev(G), dS, dP, _dev(np.full((B, S), float(it))), B, S, False, dst, FROZEN, it, False)
    z = dst['z'].cpu().numpy()
    assert (z[:, [1, 4]] == 0).all() and (z[:, [0, 2, 3, 5]] != 0).all() and dst['best_iter'].cpu().tolist() == [[1] * S] * B


@pytest.mark.parametrize('K', [1, 63, 64, 65, 729, 4096])
def test_select(K):
    _api()
    mod = sys.modules['efgh_amd.common.refine_multi']
    rs = np.random.RandomState(K)
    val = rs.randn(4, K)
    val[1] = 2.5                                                 # all equal
    val[2] = rs.randint(0, 5, K)                                 # planted ties
    val[3, rs.rand(K) < 0.3] = np.nan
    val[3, rs.rand(K) < 0.2] = val[3, 0]
    if K > 4:
        val[3, 3], val[3, 4] = 0.0, -0.0
    for keep in sorted({1, min(8, K), min(64, K)}):
        got = mod.select(_dev(val), keep)
        assert got.dtype == torch.int32 and tuple(got.shape) == (4, keep)
        ref = RC.select(val, keep)
        assert (got.cpu().numpy() == ref).all(), (K, keep)
    one = mod.select(_dev(val[0]), 1)
    assert tuple(one.shape) == (1,) and int(one[0]) == int(np.argmax(val[0]))


def _peak(B=1):
    pc, img, P, value = peak_case()
    t = dict(pc=_dev(np.concatenate([pc] * B)), img=_dev(np.concatenate([img] * B)), value=_dev(np.concatenate([value] * B)))
    return t, pc, P[0, 0]


def _kw(t, **more):
    kw = dict(value=t['value'], value_range=(0.0, 256.0), bins=PEAK['bins'])
    kw.update(more)
    return kw


def _same_result(a, b):
    return all(torch.equal(_bits(getattr(a, k)) if getattr(a, k).dtype == torch.float64 else getattr(a, k),
                           _bits(getattr(b, k)) if getattr(b, k).dtype == torch.float64 else getattr(b, k)) for k in a.__slots__)


def test_iterate_zero_is_the_start():
    C = _api()
    t, pc, P0 = _peak()
    starts = _dev(np.stack([start_pose(P0, STARTS[0]), start_pose(P0, STARTS[1]), P0])[None])
    for s in (starts, starts.float()):
        r = C.refine_multi(t['pc'], t['img'], s, iters=1, **_kw(t))
        assert isinstance(r, C.MultiRefined) and r.pose.dtype == torch.float64 and tuple(r.pose.shape) == (1, 3, 3, 4) and tuple(r.trace.shape) == (1, 1, 3)
        assert torch.equal(_bits(r.pose), _bits(s.to(torch.float64))) and r.best_iter.tolist() == [[0, 0, 0]] and torch.equal(r.mi, r.start_mi)
    one = C.refine_multi(t['pc'], t['img'], starts[:, 0], iters=1, **_kw(t))      # (B,3,4): S = 1
    old = C.refine(t['pc'], t['img'], starts[:, 0], iters=1, **_kw(t))
    assert tuple(one.mi.shape) == (1, 1) and torch.equal(_bits(one.mi[:, 0]), _bits(old.mi)) and torch.equal(_bits(one.pose[:, 0]), _bits(old.pose))


@pytest.mark.parametrize('pool', [False, True])
def test_starts_are_independent(pool):
    C = _api()
    t, pc, P0 = _peak(B=2)
    rs = np.random.RandomState(8)
    zs = rs.randn(2, 5, 6) * np.array([0.03, 0.03, 0.03, 0.15, 0.15, 0.15])
    starts = _dev(np.stack([np.stack([start_pose(P0, zs[b, s].tolist()) for s in range(5)]) for b in range(2)]))
    keep = starts.clone()
    r = C.refine_multi(t['pc'], t['img'], starts, iters=20, pool=pool, **_kw(t))
    assert tuple(r.trace.shape) == ((20, 5) if pool else (20, 2, 5)) and tuple(r.mi.shape) == ((5,) if pool else (2, 5))
    assert (r.trace[0] != r.trace[-1]).all() and (r.best_iter > 0).any()
    for s in range(5):
        one = C.refine_multi(t['pc'], t['img'], starts[:, s], iters=20, pool=pool, **_kw(t))
        for k in ('mi', 'start_mi', 'best_iter', 'trace'):
            a, b = getattr(r, k)[..., s], getattr(one, k)[..., 0]
            assert torch.equal(a, b) and not torch.isnan(a.double()).any(), (k, s)
        assert torch.equal(_bits(r.pose[:, s]), _bits(one.pose[:, 0])), s
    again = C.refine_multi(t['pc'], t['img'], starts, iters=20, pool=pool, **_kw(t))
    assert _same_result(r, again) and torch.equal(starts, keep)   # two runs give the same bits; the inputs are unwritten
    # best() and best_pose() stay on the device: a host read of the index raises here
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        i, bp = r.best(), r.best_pose()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert tuple(i.shape) == (() if pool else (2,)) and i.is_cuda and tuple(bp.shape) == (2, 3, 4)
    mi = r.mi.cpu().numpy()
    want = np.argmax(mi, -1)
    assert (i.cpu().numpy() == want).all()
    for b in range(2):                                            # (pooled: one z for the batch, both samples took the same start)
        assert torch.equal(_bits(bp[b]), _bits(r.pose[b, int(want) if pool else int(want[b])]))


def test_on_the_peak_scene():
    C = _api()
    t, pc, P0 = _peak()
    starts = _dev(np.stack([start_pose(P0, STARTS[0]), start_pose(P0, STARTS[1]), P0])[None])
    r = C.refine_multi(t['pc'], t['img'], starts, iters=200, rot_step_deg=0.2, trans_step=0.02, **_kw(t))
    off = lambda P: reprojection_offset(pc[0], P, P0, PEAK['h'], PEAK['w'])
    ends = [off(r.pose[0, s].cpu().numpy()) for s in range(3)]
    print('offsets %s px -> %s px, mi %s -> %s at %s' % (['%.2f' % off(starts[0, s].cpu().numpy()) for s in range(3)], ['%.3f' % e for e in ends],
                                                         r.start_mi[0].tolist(), r.mi[0].tolist(), r.best_iter[0].tolist()))
    assert max(ends) <= 0.5
    trace = r.trace.cpu().numpy()
    assert (r.mi.cpu().numpy() == trace.max(0)).all() and (r.best_iter.cpu().numpy() == trace.argmax(0)).all() and (r.start_mi.cpu().numpy() == trace[0]).all()
    assert r.best().tolist() == [int(np.argmax(r.mi.cpu().numpy()[0]))] and tuple(r.best_pose().shape) == (1, 3, 4)
    again = C.score_soft(t['pc'], t['img'], r.best_pose(), **_kw(t))
    assert torch.equal(_bits(again.mi[:, 0]), _bits(r.mi[0, r.best()]))
    all3 = C.score_soft(t['pc'], t['img'], r.pose, **_kw(t))      # every pose handed back is the iterate that scored best
    assert torch.equal(_bits(all3.mi), _bits(r.mi))
    # a depth test whose tolerance hides nothing: the same climb, bit for bit
    vis = functools.partial(C.score_soft_visible, occlusion=C.Occlusion(8, 0.0, 1e30))
    rv = C.refine_multi(t['pc'], t['img'], starts, iters=30, scorer=vis, **_kw(t))
    rp = C.refine_multi(t['pc'], t['img'], starts, iters=30, **_kw(t))
    assert _same_result(rv, rp) and (rp.best_iter > 0).all()


def test_starts_that_see_nothing_stay_put():
    C = _api()
    t, pc, P0 = _peak()
    away = P0.copy()
    away[2] = -away[2]                                            # every point behind the camera
    bad = start_pose(P0, STARTS[0])
    bad[1, 2] = np.nan
    starts = _dev(np.stack([away, bad, start_pose(P0, STARTS[0])])[None])
    r = C.refine_multi(t['pc'], t['img'], starts, iters=5, **_kw(t))
    assert torch.equal(_bits(r.pose[:, :2]), _bits(starts[:, :2])) and (r.mi[:, :2] == 0).all() and (r.trace[:, :, :2] == 0).all()
    assert r.best_iter[0].tolist()[:2] == [0, 0] and int(r.best_iter[0, 2]) > 0 and float(r.mi[0, 2]) > float(r.start_mi[0, 2])
    assert not any(torch.isnan(x).any() for x in (r.mi, r.start_mi, r.trace, r.pose[:, 0], r.pose[:, 2]))


def test_search_from_the_far_start():
    """the grid around the far start of the host file holds a pose inside the basin: one step back along each of FAR's six axes"""
    C = _api()
    t, pc, P0 = _peak()
    far = _dev(start_pose(P0, FAR)[None])
    f = C.search(t['pc'], t['img'], far, rot_deg=[math.degrees(abs(x)) for x in FAR[:3]], trans=[abs(x) for x in FAR[3:]], steps=1, keep=8,
                 iters=200, **_kw(t))
    off = lambda P: reprojection_offset(pc[0], P, P0, PEAK['h'], PEAK['w'])
    assert isinstance(f, C.Searched) and tuple(f.coarse.mi.shape) == (1, 729) and f.kept.dtype == torch.int32 and tuple(f.kept.shape) == (1, 8)
    assert (f.kept.cpu().numpy() == RC.select(f.coarse.mi.cpu().numpy(), 8)).all()
    end = off(f.pose[0].cpu().numpy())
    print('search: %.2f px -> %.3f px; kept %s, their ends %s px' % (off(far[0].cpu().numpy()), end, f.kept[0].tolist(),
                                                                   ['%.2f' % off(f.refined.pose[0, s].cpu().numpy()) for s in range(8)]))
    assert tuple(f.pose.shape) == (1, 3, 4) and torch.equal(_bits(f.pose), _bits(f.refined.best_pose()))
    assert end <= 0.5
    # pooled: one selection and one z for the batch
    t2, _, _ = _peak(B=2)
    g = C.search(t2['pc'], t2['img'], torch.cat([far, far]), rot_deg=(0.5, 0, 0), trans=(0.1, 0, 0), keep=3, iters=3, pool=True, **_kw(t2))
    assert tuple(g.kept.shape) == (3,) and tuple(g.coarse.mi.shape) == (9,) and tuple(g.pose.shape) == (2, 3, 4) and tuple(g.refined.mi.shape) == (3,)
    assert (g.kept.cpu().numpy() == RC.select(g.coarse.mi.cpu().numpy()[None], 3)[0]).all()


def test_refusals_launch_nothing():
    from efgh_amd import _C
    C = _api()
    mod = sys.modules['efgh_amd.common.refine_multi']
    t, pc, P0 = _peak()
    starts = _dev(np.stack([P0, P0])[None])
    with pytest.raises(_C.EfghError, match='S = 4097'):
        C.refine_multi(t['pc'], t['img'], torch.zeros(1, 4097, 3, 4, device='cuda'), **_kw(t))
    for name, kw in (('starts', dict(starts=starts[0, 0])), ('starts', dict(starts=starts.half())), ('iters', dict(iters=0)),
                     ('rot_step_deg', dict(dof=(1, 1))), ('rot_step_deg', dict(dof=7)), ('starts', dict(starts=starts.cpu()))):
        a = dict(starts=starts)
        a.update(kw)
        with pytest.raises(_C.EfghError, match=r'refine_multi: %s\b' % name):
            C.refine_multi(t['pc'], t['img'], **_kw(t, **a))
    with pytest.raises(_C.EfghError, match=r'score_soft: cam_T_velo'):     # a batch that is not the cloud's: the scorer's own check
        C.refine_multi(t['pc'], t['img'], torch.cat([starts, starts]), **_kw(t))
    with pytest.raises(_C.EfghError, match=r'search: keep: 65'):
        C.search(t['pc'], t['img'], starts[:, 0], rot_deg=(1, 1, 1), trans=(1, 1, 1), keep=65, **_kw(t))
    with pytest.raises(_C.EfghError, match=r'search: keep: 4 of K = 3'):
        C.search(t['pc'], t['img'], starts[:, 0], rot_deg=(1, 0, 0), trans=(0, 0, 0), keep=4, **_kw(t))
    with pytest.raises(_C.EfghError, match=r'select: keep: 65'):
        mod.select(torch.zeros(2, 100, dtype=torch.float64, device='cuda'), 65)
    with pytest.raises(_C.EfghError, match=r'select: val'):
        mod.select(torch.zeros(2, 100, device='cuda'), 8)
    # the entry points themselves, with guard buffers
    L, sp = _C.lib(), _C.stream_ptr
    B, S = 2, 3
    f = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device='cuda')
    G, Ps, P, mi, z, m, v, bm, bp, tr = f(B, S, 12), f(B, S, 12), f(B, S, 12), f(B, S), f(B * S, 6), f(B * S, 6), f(B * S, 6), f(B, S), f(B, S, 12), f(4, B, S)
    bi = torch.full((B, S), -7, dtype=torch.int64, device='cuda')
    idx = torch.full((2, 64), -7, dtype=torch.int32, device='cuda')

    def step(B=B, S=S, pool=0, it=1, ss=1.0, bc2=0.5, last=0, scale=SCALE, G=G, z=z):
        return L.efgh_refine_step(_C.ptr(G), _C.ptr(Ps), _C.ptr(P), _C.ptr(mi), B, S, pool, _C.ptr(z), _C.ptr(m), _C.ptr(v), _C.ptr(bm), _C.ptr(bi),
                                  _C.ptr(bp), _C.ptr(tr), *scale, it, ss, bc2, last, sp())
    for kw, word in ((dict(S=4097), b'S = 4097'), (dict(S=0), b'S = 0'), (dict(B=0), b'B = 0'), (dict(pool=2), b'pool = 2'), (dict(it=-1), b'it = -1'),
                     (dict(last=2), b'last = 2'), (dict(ss=float('nan')), b'step_size = nan'), (dict(bc2=0.0), b'bc2_sqrt = 0'),
                     (dict(scale=[1.0, -1.0, 1, 1, 1, 1]), b'scale1 = -1'), (dict(scale=[1.0, 1, 1, 1, 1, float('inf')]), b'scale5 = inf'),
                     (dict(G=None), b'null pointer'), (dict(z=None), b'null pointer')):
        assert step(**kw) != 0
        assert b'efgh_refine_step' in L.efgh_last_error() and word in L.efgh_last_error(), (kw, L.efgh_last_error())
    for a, word in (((_C.ptr(G), 2, 4097, 8), b'K = 4097'), ((_C.ptr(G), 2, 100, 65), b'keep = 65'), ((_C.ptr(G), 2, 6, 7), b'keep = 7'),
                    ((_C.ptr(G), 2, 6, 0), b'keep = 0'), ((_C.ptr(G), 0, 6, 2), b'rows = 0'), ((None, 2, 6, 2), b'null pointer')):
        assert L.efgh_refine_select(*a, _C.ptr(idx), sp()) != 0
        assert b'efgh_refine_select' in L.efgh_last_error() and word in L.efgh_last_error(), (a, L.efgh_last_error())
    torch.cuda.synchronize()
    assert all((x == -7).all() for x in (G, Ps, P, mi, z, m, v, bm, bp, tr, bi, idx))
    r = C.refine_multi(t['pc'], t['img'], starts, iters=2, **_kw(t))     # and the library goes on working
    assert torch.equal(_bits(r.pose[:, 0]), _bits(r.pose[:, 1]))
