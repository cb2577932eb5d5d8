"""csrc/score_soft.hip through efgh_amd.common.score_soft / refine against tests/score_soft_contract.py: `hist` and `count` EXACTLY, mi,
nmi and the entropies inside score_contract.bounds, the pose gradient inside the bound the contract derives (never fitted to an
output).  Small shapes: the wave and block boundaries, one point either side of the kernel's chunk, several candidates and samples,
both ends of the bin range, pooled batches, the directed edge cases of the host file, 4096 points on one pixel, empty histograms, NaN /
inf in poses, clouds and values, real strides, a float32 leaf, a non-uniform upstream gradient, two runs bit for bit, and `refine`
on the device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_contract as SC  # noqa: E402
import score_soft_contract as SS  # noqa: E402
from test_gpu_score import BIG, COMBOS, _case  # noqa: E402
from test_score_host import PEAK, image, peak_case  # noqa: E402
from test_score_soft_host import STARTS, edge_case, reprojection_offset, start_pose  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ('mi', 'nmi', 'hx', 'hy', 'hxy')


def _soft(*a, **kw):
    from efgh_amd.common import score_soft
    return score_soft(*a, **kw)


def _chunk():
    from efgh_amd import _C
    return int(_C.lib().efgh_score_chunk())


def _same(got, ref, grad=None):
    """Score against the contract's dict: hist and count exactly, the five numbers inside their bounds; grad (B,K,3,4), if given,
    inside its own"""
    hist, count = got.hist.cpu().numpy(), got.count.cpu().numpy()
    assert hist.dtype == np.int32 and hist.shape == ref['hist'].shape and count.dtype == np.int32 and count.shape == ref['count'].shape
    bad = np.argwhere(hist != ref['hist'])
    assert bad.shape[0] == 0, ('hist', bad.shape[0], bad[:4].tolist())
    assert (count == ref['count']).all(), ('count', count.tolist(), ref['count'].tolist())
    for k in KEYS:
        a = getattr(got, k).detach().cpu().numpy()
        assert a.dtype == np.float64 and a.shape == ref[k].shape and np.isfinite(a).all(), (k, a)
        err, bound = np.abs(a - ref[k]), ref['bound'][k]
        print('%s: largest error %.3e, its bound %.3e' % (k, err.max(), bound.flat[err.argmax()]))
        assert (err <= bound).all(), (k, err.max(), bound.flat[err.argmax()])
        assert (a[ref['count'] == 0] == 0).all(), k
    if grad is not None:
        g = grad.cpu().numpy()
        assert g.dtype == np.float64 and g.shape == ref['grad'].shape and np.isfinite(g).all()
        err, bound = np.abs(g - ref['grad']), ref['grad_bound']
        print('grad: largest |G| %.3e, largest error %.3e, its bound %.3e, smallest bound / error %.1f'
              % (np.abs(ref['grad']).max(), err.max(), bound.flat[err.argmax()], (bound[err > 0] / err[err > 0]).min() if (err > 0).any() else np.inf))
        assert (err <= bound).all(), ('grad', err.max(), bound.flat[err.argmax()])
        zero = ref['count'] == 0
        assert (g[:, zero] == 0).all() if zero.ndim == 1 else (g[zero] == 0).all()


def _check(pc, img, P, value, lo=0.0, hi=1.0, bins=32, min_depth=0.0, pool=False):
    """numpy pc (B,C,N) float32, img uint8 (B,H,W,3), P (B,K,3,4) float64, value (B,N) float32 -> (Score, grad, the contract's dict)"""
    T = torch.from_numpy(P).cuda().requires_grad_()
    got = _soft(torch.from_numpy(pc).cuda(), torch.from_numpy(img).cuda(), T, value=torch.from_numpy(value).cuda(), value_range=(lo, hi),
                bins=bins, min_depth=min_depth, pool=pool, want_hist=True)
    assert got.mi.requires_grad and not any(getattr(got, k).requires_grad for k in KEYS[1:])
    got.mi.sum().backward()
    assert T.grad.dtype == torch.float64 and tuple(T.grad.shape) == tuple(P.shape)
    ref = SS.score_soft(pc, img, P, value, lo, hi, bins, min_depth, pool=pool, chunk=_chunk())
    _same(got, ref, T.grad)
    return got, T.grad, ref


@pytest.mark.parametrize('N', [1, 63, 64, 65, 255, 256, 257, 1000, 'chunk-1', 'chunk+0', 'chunk+1'])
def test_sizes(N):
    n = _chunk() + int(N[5:]) if isinstance(N, str) else N
    seen = 0
    for j, (K, B, bins, hw) in enumerate(COMBOS):
        pc, img, P = _case(n, hw, 10 * j + n % 97, B=B, K=K)
        got, grad, ref = _check(pc, img, P, pc[:, 3], 0.0, 1.0, bins)
        seen += int(ref['count'].sum())
    assert seen >= (n if n > 1 else 0)


def test_pooled_batch_is_the_sum_of_the_samples():
    pc, img, P = _case(1500, BIG, 15, B=3, K=2)
    for bins in (8, 64):
        got, grad, ref = _check(pc, img, P, pc[:, 3], bins=bins, pool=True)
        each = SS.score_soft(pc, img, P, pc[:, 3], 0.0, 1.0, bins, want_grad=False)
        assert tuple(got.hist.shape) == (2, bins, bins) and tuple(got.mi.shape) == (2,) and tuple(got.count.shape) == (2,)
        assert (got.hist.cpu().numpy() == each['hist'].sum(0)).all() and (got.count.cpu().numpy() == each['count'].sum(0)).all()
        assert np.abs(ref['grad']).max() > 0


def test_directed_edge_cases():
    """pixel centres, t - j exactly 0 and 1, L = 0 and 255, neighbours clipped at all four borders (test_score_soft_host.edge_case)"""
    pc, img, P, value = edge_case()
    for bins in (8, 64):
        got, grad, ref = _check(pc, img, P, value, bins=bins)
        assert ref['count'].tolist() == [[pc.shape[2]]] and np.abs(ref['grad']).max() > 0
    # the directed points alone: every gate is shut or every slope is 0 or the neighbour cell is empty where it matters
    got, grad, ref = _check(pc[:, :, :4], img, P, value[:, :4], bins=8)
    assert (grad == 0).all() and ref['hist'][0, 0, 2].tolist() == [256, 256, 0, 0, 0, 0, 0, 512]


def test_4096_points_on_one_pixel():
    img = image(*BIG, 30)[None]
    P = np.array([[[[0, 0, 5.5, 0], [0, 0, 7.5, 0], [0, 0, 1., 0]]]])
    pc = np.zeros((1, 3, 4096), np.float32)
    pc[0, 2] = (4096 - np.arange(4096)) / 16.0
    value = np.full((1, 4096), 0.3, np.float32)
    for bins in (8, 64):
        got, grad, ref = _check(pc, img, P, value, bins=bins)
        assert ref['hist'].sum() == 4096 * 256 and ref['count'].tolist() == [[4096]] and (ref['hist'][0, 0] > 0).sum() <= 2
        assert np.isfinite(grad.cpu().numpy()).all()


def test_empty_histograms_and_non_finite_poses():
    pc, img, P = _case(600, BIG, 40, B=1, K=6)
    P[0, 1, 0] += 1e4 * P[0, 1, 2]                                 # every u 10^4 pixels to the right: nothing in frame
    P[0, 2, 2] = 0.0                                               # w = 0 for every point: none in front
    P[0, 3, 1, 1] = np.nan
    P[0, 4, 0, 3] = np.inf
    P[0, 5, 2, 3] = -np.inf
    got, grad, ref = _check(pc, img, P, pc[:, 3])
    assert ref['count'][0, 0] > 100 and ref['count'][0, 1:].tolist() == [0] * 5
    for k in KEYS:
        assert (getattr(got, k)[0, 1:] == 0).all() and not torch.isnan(getattr(got, k)).any()     # five zeros a candidate
    assert (grad[0, 1:] == 0).all() and not torch.isnan(grad).any() and grad[0, 0].abs().max() > 0
    # NaN and inf coordinates in the cloud: those points drop out, the rest count
    pc[0, 0, ::7] = np.nan
    pc[0, 2, 1::7] = np.inf
    pc[0, 1, 2::7] = -np.inf
    got, grad, ref = _check(pc, img, P[:, :1], pc[:, 3])
    assert 50 < ref['count'][0, 0] < 600 * 4 // 7


def test_nan_and_infinite_values_and_min_depth():
    pc, img, P = _case(1000, BIG, 50, B=2, K=2)
    value = pc[:, 3].copy()
    value[:, ::3] = np.nan
    value[:, 1::9] = np.inf
    value[:, 2::9] = -np.inf
    got, grad, ref = _check(pc, img, P, value, bins=8)
    full = SS.score_soft(pc, img, P, pc[:, 3], 0.0, 1.0, 8, want_grad=False)
    assert (ref['count'] < full['count']).all() and (ref['count'] > full['count'] // 2).all()
    _check(pc, img, P, value, lo=0.25, hi=0.5, bins=64, min_depth=12.0)
    _check(pc, img, P, value * 200 - 100, lo=-37.5, hi=61.0, bins=16)


def test_strided_cloud_and_value():
    """the cloud is rows 1..4 of a 6-row tensor and every second point of it, the value a column of a (B,N,3) tensor"""
    N, B, K = 1031, 3, 2
    pc, img, P = _case(N, BIG, 20, B=B, K=K)
    big = torch.zeros(B, 6, 2 * N, device='cuda')
    big[:, 1:5, ::2] = torch.from_numpy(pc).cuda()
    val3 = torch.rand(B, N, 3, device='cuda') * 1.5 - 0.25           # beyond both ends of the range
    view, val = big[:, 1:5, ::2], val3[:, :, 1]
    assert view.stride(2) == 2 and val.stride(1) == 3
    keep = big.clone(), val3.clone()
    T = torch.from_numpy(P).cuda().requires_grad_()
    got = _soft(view, torch.from_numpy(img).cuda(), T, value=val, bins=16, want_hist=True)
    got.mi.sum().backward()
    _same(got, SS.score_soft(pc, img, P, val.cpu().numpy(), 0.0, 1.0, 16, chunk=_chunk()), T.grad)
    # value=None is row 3 of the view; a view with a batch stride of its own
    T.grad = None
    got = _soft(view, torch.from_numpy(img).cuda(), T, want_hist=True)
    got.mi.sum().backward()
    _same(got, SS.score_soft(pc, img, P, pc[:, 3], 0.0, 1.0, 32, chunk=_chunk()), T.grad)
    assert torch.equal(keep[0], big) and torch.equal(keep[1], val3)


def test_float32_leaf_non_uniform_upstream_and_no_grad():
    pc, img, P = _case(2000, BIG, 60, B=3, K=5)
    t = torch.from_numpy(pc).cuda(), torch.from_numpy(img).cuda()
    P32 = P.astype(np.float32)
    ref = SS.score_soft(pc, img, P32.astype(np.float64), pc[:, 3], 0.0, 1.0, 32, chunk=_chunk())
    T = torch.from_numpy(P32).cuda().requires_grad_()
    got = _soft(*t, T, want_hist=True)
    up = torch.tensor(np.random.RandomState(61).randn(3, 5), device='cuda')
    (got.mi * up).sum().backward()
    assert T.grad.dtype == torch.float32 and tuple(T.grad.shape) == (3, 5, 3, 4)
    want = ref['grad'] * up.cpu().numpy()[:, :, None, None]
    # the product and the conversion to float32 round once each on top of the gradient's own bound
    tol = ref['grad_bound'] * np.abs(up.cpu().numpy())[:, :, None, None] + np.abs(want) * (2.0 ** -24 + 2.0 ** -52)
    err = np.abs(T.grad.cpu().numpy().astype(np.float64) - want)
    assert (err <= tol).all(), (err.max(), tol.flat[err.argmax()])
    _same(got, ref)
    # (B,3,4) is K = 1, and its gradient has that shape; pooled, the upstream gradient is (K,)
    T1 = torch.from_numpy(P[:, 0]).cuda().requires_grad_()
    got = _soft(*t, T1, pool=True, want_hist=True)
    (got.mi * 3.0).sum().backward()
    one = SS.score_soft(pc, img, P[:, :1], pc[:, 3], 0.0, 1.0, 32, pool=True, chunk=_chunk())
    assert tuple(T1.grad.shape) == (3, 3, 4)
    assert (np.abs(T1.grad.cpu().numpy() - 3.0 * one['grad'][:, 0]) <= 3.0 * one['grad_bound'][:, 0] + np.abs(3.0 * one['grad'][:, 0]) * 2.0 ** -52).all()
    # without requires_grad, and under no_grad, mi is a plain tensor
    plain = _soft(*t, torch.from_numpy(P).cuda(), want_hist=True)
    assert not plain.mi.requires_grad and plain.mi.grad_fn is None
    _same(plain, SS.score_soft(pc, img, P, pc[:, 3], 0.0, 1.0, 32, want_grad=False))
    with torch.no_grad():
        assert not _soft(*t, T).mi.requires_grad


def test_two_runs_same_bits_inputs_untouched():
    pc, img, P, value = peak_case()
    pc2, img2, P2 = _case(3 * _chunk() + 17, BIG, 70, B=2, K=5)
    for arrs, kw in (((pc, img, P, value), dict(value_range=(0.0, 256.0), bins=8)), ((pc2, img2, P2, pc2[:, 3].copy()), dict(bins=64)),
                     ((pc2, img2, P2, pc2[:, 3].copy()), dict(bins=32, pool=True))):
        t = [torch.from_numpy(a).cuda() for a in arrs]
        runs = []
        for _ in range(2):
            T = t[2].clone().requires_grad_()
            s = _soft(t[0], t[1], T, value=t[3], want_hist=True, **kw)
            s.mi.sum().backward()
            runs.append([getattr(s, k).detach() for k in KEYS + ('count', 'hist')] + [T.grad])
        for a, b in zip(*runs):
            assert a.data_ptr() != b.data_ptr()
            assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
        assert runs[0][-1].abs().max() > 0
        for a, b in zip(t, arrs):
            assert (a.cpu().numpy().view(np.uint8) == b.view(np.uint8)).all()


def test_count_is_scores_count():
    from efgh_amd.common import score
    pc, img, P = _case(3000, BIG, 80, B=2, K=3)
    t = torch.from_numpy(pc).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(P).cuda()
    value = t[0][:, 3].clone()
    value[:, ::5] = float('nan')
    hard, soft = score(*t, value=value, bins=16, min_depth=2.0), _soft(*t, value=value, bins=16, min_depth=2.0)
    assert torch.equal(hard.count, soft.count) and hard.count.min() > 100 and soft.count.dtype == torch.int32


def test_errors_name_the_value_and_launch_nothing():
    from efgh_amd import _C
    pc, img, P = _case(64, BIG, 90, B=2, K=2)
    t = dict(pc=torch.from_numpy(pc).cuda(), img=torch.from_numpy(img).cuda(), T=torch.from_numpy(P).cuda())
    for name, kw in (('bins', dict(bins=24)), ('pc', dict(pc=t['pc'].cpu())), ('cam_T_velo', dict(T=t['T'].cpu())), ('pool', dict(pool=1)),
                     ('value_range', dict(value_range=(1.0, 0.0))), ('min_depth', dict(min_depth=-1.0))):
        a = dict(t)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        with pytest.raises(_C.EfghError, match=r'score_soft: %s\b' % name):
            _soft(a['pc'], a['img'], a['T'], **kw)
    # a point adds 256 to a 32-bit cell: 2^23 points a histogram are refused, by the wrapper and by the entry point
    wide, wval = torch.zeros(1, 3, 1 << 23, device='cuda').expand(2, 3, 1 << 23), torch.zeros(1, 1 << 23, device='cuda').expand(2, 1 << 23)
    with pytest.raises(_C.EfghError, match=r'score_soft: pc: 8388608 points'):
        _soft(wide, t['img'], t['T'], value=wval)
    with pytest.raises(_C.EfghError, match=r'score_soft: pc: 8388608 points'):
        _soft(wide[:, :, :1 << 22], t['img'], t['T'], value=wval[:, :1 << 22], pool=True)
    L, st = _C.lib(), _C.stream_ptr
    h, w = BIG
    p, v, P0, im = t['pc'], t['pc'][:, 3], t['T'].contiguous(), t['img']
    hist = torch.full((2, 2, 64, 64), -7, dtype=torch.int32, device='cuda')
    table, flag = torch.full((4, 64, 64), -7.0, dtype=torch.float64, device='cuda'), torch.full((4, 64, 64), 7, dtype=torch.uint8, device='cuda')
    tot, part = torch.full((4,), -7, dtype=torch.int32, device='cuda'), torch.full((2, 2, 1, 12), -7.0, dtype=torch.float64, device='cuda')
    G = torch.full((2, 2, 12), -7.0, dtype=torch.float64, device='cuda')

    def points(B=2, N=64, K=2, bins=8, lo=0.0, hi=1.0, min_depth=0.0, pool=0):
        return (_C.ptr(p), p.stride(0), p.stride(1), B, N, _C.ptr(v), v.stride(0), _C.ptr(P0), K, _C.ptr(im), h, w, bins, lo, hi, min_depth, pool)
    for kw, word in ((dict(bins=256), b'bins = 256'), (dict(K=4097), b'K = 4097'), (dict(B=0), b'B = 0'), (dict(N=0), b'N = 0'),
                     (dict(N=1 << 23), b'N = 8388608'), (dict(N=1 << 22, pool=1), b'B * N = 8388608'), (dict(pool=2), b'pool = 2'),
                     (dict(lo=1.0, hi=1.0), b'lo = 1'), (dict(min_depth=float('nan')), b'min_depth')):
        assert L.efgh_score_soft_hist(*points(**kw), _C.ptr(hist), st()) != 0
        assert b'efgh_score_soft_hist' in L.efgh_last_error() and word in L.efgh_last_error(), (kw, L.efgh_last_error())
        assert L.efgh_score_soft_grad(*points(**kw), _C.ptr(table), _C.ptr(flag), _C.ptr(tot), _C.ptr(part), st()) != 0
        assert b'efgh_score_soft_grad' in L.efgh_last_error() and word in L.efgh_last_error(), (kw, L.efgh_last_error())
    assert L.efgh_score_soft_hist(*points(), None, st()) != 0 and b'null pointer' in L.efgh_last_error()
    assert L.efgh_score_soft_grad(*points(), _C.ptr(table), None, _C.ptr(tot), _C.ptr(part), st()) != 0 and b'null pointer' in L.efgh_last_error()
    for a, word in (((_C.ptr(hist), 0, 8), b'n_hist = 0'), ((_C.ptr(hist), 4, 12), b'bins = 12'), ((None, 4, 8), b'null pointer')):
        assert L.efgh_score_soft_table(*a, _C.ptr(table), _C.ptr(flag), _C.ptr(tot), st()) != 0
        assert b'efgh_score_soft_table' in L.efgh_last_error() and word in L.efgh_last_error()
    for a, word in (((_C.ptr(part), 2, 2, 0), b'n_chunk = 0'), ((_C.ptr(part), 2, 2, 2049), b'n_chunk = 2049'), ((_C.ptr(part), 2, 4097, 1), b'K = 4097'),
                    ((None, 2, 2, 1), b'null pointer')):
        assert L.efgh_score_soft_fold(*a, _C.ptr(G), st()) != 0
        assert b'efgh_score_soft_fold' in L.efgh_last_error() and word in L.efgh_last_error()
    torch.cuda.synchronize()
    assert (hist == -7).all() and (table == -7).all() and (flag == 7).all() and (tot == -7).all() and (part == -7).all() and (G == -7).all()
    _check(pc, img, P, pc[:, 3])                                   # and the library goes on working


def test_refine_on_the_device():
    from efgh_amd.common import refine
    pc, img, P, value = peak_case()
    P0 = P[0, 0]
    Pst = start_pose(P0, STARTS[0])
    t = torch.from_numpy(pc).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(Pst)[None].cuda()
    r = refine(*t, value=torch.from_numpy(value).cuda(), value_range=(0.0, 256.0), bins=PEAK['bins'], iters=200, rot_step_deg=0.2, trans_step=0.02)
    assert r.pose.is_cuda and r.pose.dtype == torch.float64 and tuple(r.pose.shape) == (1, 3, 4) and tuple(r.trace.shape) == (200, 1)
    trace, best = r.trace.cpu().numpy()[:, 0], int(r.best_iter)
    after = reprojection_offset(pc[0], r.pose[0].cpu().numpy(), P0, PEAK['h'], PEAK['w'])
    print('offset %.2f px -> %.3f px, mi %.4f -> %.4f at iterate %d'
          % (reprojection_offset(pc[0], Pst, P0, PEAK['h'], PEAK['w']), after, float(r.start_mi), float(r.mi), best))
    assert best == int(trace.argmax()) and float(r.mi) == trace.max() and float(r.start_mi) == trace[0]
    # the pose handed back is the iterate that scored best: scoring it again gives the same number, bit for bit
    again = _soft(t[0], t[1], r.pose, value=torch.from_numpy(value).cuda(), value_range=(0.0, 256.0), bins=PEAK['bins'])
    assert torch.equal(again.mi[:, 0], r.mi)
    assert float(r.mi) >= float(r.start_mi)
    assert after <= 0.5
    # iterate 0 is P0 bit for bit
    r1 = refine(*t, value=torch.from_numpy(value).cuda(), value_range=(0.0, 256.0), bins=PEAK['bins'], iters=1)
    assert torch.equal(r1.pose.view(torch.int64), t[2].view(torch.int64)) and r1.best_iter.tolist() == [0] and torch.equal(r1.mi, r.start_mi)
