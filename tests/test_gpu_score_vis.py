"""csrc/score_vis.hip and the masked instances of score.hip's / score_soft.hip's kernels through efgh_amd.common.score_vis against
tests/score_vis_contract.py: `zmin` bits, mask words, `hist`, `count` and occupancy EXACTLY; mi / nmi / the entropies inside
score_contract.bounds, the pose gradient inside score_soft_contract's bound, mi_mm inside score_vis_contract.mm_bound (none fitted to
an output).  Small shapes: the mask word, wave, block and chunk boundaries; cells 1, 8, (6, 2) and 64; three tolerances; directed
cases; the link to the unmasked path bit for bit; pooled batches, real strides, a float32 leaf, two runs bit for bit, the refusals, and
`refine` through a functools.partial of the new scorer."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_contract as FC  # noqa: E402
import score_vis_contract as SV  # noqa: E402
from test_gpu_score import BIG, COMBOS, SMALL, _case  # noqa: E402
from test_score_host import PEAK, image, peak_case  # noqa: E402
from test_score_soft_host import STARTS, start_pose  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ('mi', 'nmi', 'hx', 'hy', 'hxy', 'mi_mm')
CELLS = (1, 8, (6, 2), 64)
TOLS = ((0.0, 0.0), (0.25, 0.0), (0.0, 0.5))
assert SMALL == (5, 7) and BIG == (48, 64)                        # cell 64 is one cell on SMALL; 8 and (6, 2) clip at BIG's edges


def _api():
    from efgh_amd import common
    return common


def _chunk():
    from efgh_amd import _C
    return int(_C.lib().efgh_score_chunk())


def _occ(cell, tol=(0.0, 0.0)):
    return _api().Occlusion(cell, tol[0], tol[1])


def _cuda(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _same(got, ref, grad=None, mask=True):
    """VisibleScore against the contract's dict: zmin bits, mask words, hist, count and occupancy exactly; the six numbers inside
    their bounds; grad (B,K,3,4), if given, inside its own"""
    if mask:
        m, z = got.mask.cpu().numpy(), got.zmin.cpu().numpy()
        assert m.dtype == np.int32 and m.shape == ref['mask'].shape and z.dtype == np.float32 and z.shape == ref['zmin'].shape
        bad = np.argwhere(z.view(np.uint32) != ref['zmin'].view(np.uint32))
        assert bad.shape[0] == 0, ('zmin', bad.shape[0], bad[:4].tolist())
        bad = np.argwhere(m != ref['mask'])
        assert bad.shape[0] == 0, ('mask', bad.shape[0], bad[:4].tolist())
    hist, count, ocp = got.hist.cpu().numpy(), got.count.cpu().numpy(), got.occupancy.cpu().numpy()
    assert hist.dtype == np.int32 and hist.shape == ref['hist'].shape and count.dtype == np.int32 and count.shape == ref['count'].shape
    bad = np.argwhere(hist != ref['hist'])
    assert bad.shape[0] == 0, ('hist', bad.shape[0], bad[:4].tolist())
    assert (count == ref['count']).all(), ('count', count.tolist(), ref['count'].tolist())
    assert ocp.dtype == np.int32 and ocp.shape == ref['occupancy'].shape and (ocp == ref['occupancy']).all(), ('occupancy', ocp.tolist())
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
        print('grad: largest |G| %.3e, largest error %.3e, its bound %.3e' % (np.abs(ref['grad']).max(), err.max(), bound.flat[err.argmax()]))
        assert (err <= bound).all(), ('grad', err.max(), bound.flat[err.argmax()])
        zero = ref['count'] == 0
        assert (g[:, zero] == 0).all() if zero.ndim == 1 else (g[zero] == 0).all()


def _hard(pc, img, P, value, cell, tol=(0.0, 0.0), lo=0.0, hi=1.0, bins=32, min_depth=0.0):
    t = _cuda(pc, img, P, value)
    got = _api().score_visible(t[0], t[1], t[2], occlusion=_occ(cell, tol), value=t[3], value_range=(lo, hi), bins=bins, min_depth=min_depth,
                               want_hist=True, want_mask=True)
    ref = SV.score_visible(pc, img, P, value, lo, hi, bins, cell, tol[0], tol[1], min_depth)
    _same(got, ref)
    return got, ref


def _soft(pc, img, P, value, cell, tol=(0.0, 0.0), lo=0.0, hi=1.0, bins=32, min_depth=0.0, pool=False):
    t = _cuda(pc, img, P, value)
    T = t[2].requires_grad_()
    got = _api().score_soft_visible(t[0], t[1], T, occlusion=_occ(cell, tol), value=t[3], value_range=(lo, hi), bins=bins, min_depth=min_depth,
                                    pool=pool, want_hist=True, want_mask=True)
    assert got.mi.requires_grad and got.mi_mm.requires_grad and not any(getattr(got, k).requires_grad for k in KEYS[1:5])
    got.mi.sum().backward()
    assert T.grad.dtype == torch.float64 and tuple(T.grad.shape) == tuple(P.shape)
    ref = SV.score_soft_visible(pc, img, P, value, lo, hi, bins, cell, tol[0], tol[1], min_depth, pool=pool, chunk=_chunk())
    _same(got, ref, T.grad)
    return got, T.grad, ref


SIZES = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 'chunk-1', 'chunk+0', 'chunk+1', '2chunk+1']


@pytest.mark.parametrize('cell', CELLS, ids=str)
@pytest.mark.parametrize('N', SIZES)
def test_sizes(N, cell):
    """every size at every cell setting: the hard score at all three tolerances and the soft score with its gradient at one of them a
    combination (all three over the six), each with zmin, mask, hist, count and occupancy exact"""
    n = (2 * _chunk() + 1 if N[0] == '2' else _chunk() + int(N[5:])) if isinstance(N, str) else N
    hidden = visible = 0
    for j, (K, B, bins, hw) in enumerate(COMBOS):
        pc, img, P = _case(n, hw, 10 * j + n % 97, B=B, K=K)
        for tol in TOLS:
            got, ref = _hard(pc, img, P, pc[:, 3], cell, tol, bins=bins)
            if tol == TOLS[0]:
                hidden += int((ref['frame'] & ~ref['vis']).sum())
                visible += int(ref['vis'].sum())
            v = _api().Visibility(got.mask, got.zmin, n)
            assert (v.unpack().cpu().numpy() == ref['vis']).all() and (v.count().cpu().numpy() == ref['vis'].sum(-1)).all()
        _soft(pc, img, P, pc[:, 3], cell, TOLS[j % 3], bins=bins)
    print('N %d, cell %r: %d visible and %d hidden in-frame points over the six combinations at zero tolerance' % (n, cell, visible, hidden))
    if n >= 63:                                                    # the comparison is not vacuous: the mask hides and keeps
        assert hidden >= 1 and visible >= 1, (hidden, visible)


def test_visible_mask_alone_and_its_input_forms():
    pc, img, P = _case(1000, BIG, 5, B=3, K=2)
    t = _cuda(pc, img, P)
    ref = SV.visible(pc, P, 48, 64, (6, 2), 0.02, 0.1, 2.0)
    for im, T in ((t[1], t[2]), ((48, 64), t[2]), (t[1].permute(0, 3, 1, 2).float(), t[2].float().double())):
        v = _api().visible_mask(t[0], im, T, _occ((6, 2), (0.02, 0.1)), min_depth=2.0)
        r = ref if T is t[2] else SV.visible(pc, P.astype(np.float32).astype(np.float64), 48, 64, (6, 2), 0.02, 0.1, 2.0)
        assert v.mask.dtype == torch.int32 and v.zmin.dtype == torch.float32 and tuple(v.zmin.shape) == (3, 2, 8, 32) and v.n == 1000
        assert (v.mask.cpu().numpy() == r['mask']).all() and (v.zmin.cpu().numpy().view(np.uint32) == r['zmin'].view(np.uint32)).all()
        assert v.unpack().dtype == torch.bool and (v.unpack().cpu().numpy() == r['vis']).all()
        assert v.count().dtype == torch.int32 and (v.count().cpu().numpy() == r['vis'].sum(-1)).all()
    # (B,3,4) is K = 1; the default Occlusion is cell 8 without tolerance
    v = _api().visible_mask(t[0], t[1], t[2][:, 0])
    assert (v.mask.cpu().numpy() == SV.visible(pc, P[:, :1], 48, 64, 8)['mask']).all() and tuple(v.mask.shape) == (3, 1, 32)


def test_4096_points_on_one_pixel_at_one_depth_are_all_visible():
    img = image(*BIG, 30)[None]
    P = np.array([[[[0, 0, 5.5, 0], [0, 0, 7.5, 0], [0, 0, 1., 0]]]])
    pc = np.zeros((1, 3, 4096), np.float32)
    pc[0, 2] = 3.25
    value = np.full((1, 4096), 0.3, np.float32)
    for cell in (1, 8):
        got, ref = _hard(pc, img, P, value, cell, bins=8)
        assert ref['vis'].all() and ref['count'].tolist() == [[4096]] and (got.mask == -1).all()
        assert np.isfinite(ref['zmin']).sum() == 1 and ref['zmin'].min() == 3.25 and ref['occupancy'].tolist() == [[[1, 1, 1]]]
        assert got.mi_mm.cpu().tolist() == [[0.0]]                # Rxy - Rx - Ry + 1 = 0
    _soft(pc, img, P, value, 8, bins=8)


def test_4096_points_in_one_cell_at_distinct_depths_leave_one():
    img = image(*BIG, 30)[None]
    P = np.array([[[[0, 0, 5.5, 0], [0, 0, 7.5, 0], [0, 0, 1., 0]]]])
    pc = np.zeros((1, 3, 4096), np.float32)
    order = np.random.RandomState(31).permutation(4096)
    pc[0, 2] = (1 + order) / 16.0
    value = np.full((1, 4096), 0.3, np.float32)
    for cell in (1, 8, 64):
        got, ref = _hard(pc, img, P, value, cell, bins=8)
        assert ref['vis'].sum() == 1 and ref['vis'][0, 0, int(np.argmin(order))] and ref['count'].tolist() == [[1]]
        assert ref['zmin'].min() == 1 / 16.0
    got, ref = _hard(pc, img, P, value, 8, (0.0, 1.0), bins=8)         # depths 1/16 .. 17/16
    assert ref['count'].tolist() == [[17]]
    _soft(pc, img, P, value, 8, (0.0, 1.0), bins=8)


def test_float32_depth_ties_are_all_visible():
    """two points whose float64 depths differ but whose float32 depths tie are both visible at zero tolerance; one float32 step
    farther is hidden"""
    img = image(*BIG, 32)[None]
    P = np.array([[[[0, 0, 5.5, 0], [0, 0, 7.5, 0], [1e-5, 0, 1.0 + 1e-9, 0]]]])      # w = 1e-5 x + (1 + 1e-9) z
    pc = np.zeros((1, 3, 3), np.float32)
    pc[0, 0] = [0.0, 1e-3, 0.0]
    pc[0, 2] = [2.0, 2.0, np.nextafter(np.float32(2.0), np.float32(3.0))]
    value = np.full((1, 3), 0.5, np.float32)
    T = P[0, 0, 2]
    w = ((T[0] * pc[0, 0].astype(np.float64) + T[1] * 0.0) + T[2] * pc[0, 2].astype(np.float64)) + T[3]
    p = FC.project(pc[0], P[0, 0], *BIG)
    assert w[0] != w[1] and p['d'][0] == p['d'][1] < p['d'][2] and p['frame'].all() and len(set(zip(p['r'], p['c']))) == 1
    for cell in (1, 8):
        got, ref = _hard(pc, img, P, value, cell, bins=8)
        assert ref['vis'][0, 0].tolist() == [True, True, False] and ref['count'].tolist() == [[2]]


def test_nan_valued_points_occlude_but_do_not_count():
    pc, img, P = _case(1000, BIG, 50, B=2, K=2)
    value = pc[:, 3].copy()
    value[:, ::3] = np.nan
    value[:, 1::9] = np.inf
    for cell in (1, 8):
        got, ref = _hard(pc, img, P, value, cell, bins=8)
        clean = SV.score_visible(pc, img, P, pc[:, 3], 0.0, 1.0, 8, cell)
        assert (ref['mask'] == clean['mask']).all() and (ref['zmin'].view(np.uint32) == clean['zmin'].view(np.uint32)).all()   # the value plays no part
        nan_vis = ref['vis'] & np.isnan(value)[:, None, :]
        assert nan_vis.sum() > 10 and (ref['count'] == (ref['vis'] & ~np.isnan(value)[:, None, :]).sum(-1)).all()
        # and a NaN-valued nearest point hides the others of its cell although it does not count itself
        keep = np.arange(1000) % 3 != 0                          # the cloud without its NaN-valued points: fewer occluders
        sub = SV.score_visible(np.ascontiguousarray(pc[:, :, keep]), img, P, np.ascontiguousarray(value[:, keep]), 0.0, 1.0, 8, cell)
        assert (ref['count'] <= sub['count']).all() and (ref['count'] < sub['count']).any()
    _soft(pc, img, P, value, 8, (0.25, 0.0), bins=8)
    _hard(pc, img, P, value, (6, 2), (0.0, 0.5), lo=0.25, hi=0.5, bins=64, min_depth=12.0)
    _soft(pc, img, P, value, (6, 2), (0.0, 0.5), lo=0.25, hi=0.5, bins=64, min_depth=12.0)


def test_non_finite_points_and_poses_and_nothing_in_frame():
    pc, img, P = _case(600, BIG, 40, B=1, K=6)
    P[0, 1, 0] += 1e4 * P[0, 1, 2]                                 # every u 10^4 pixels to the right: nothing in frame
    P[0, 2, 2] = 0.0                                               # w = 0 for every point: none in front
    P[0, 3, 1, 1] = np.nan
    P[0, 4, 0, 3] = np.inf
    P[0, 5, 2, 3] = -np.inf
    for cell in (8, (6, 2)):
        got, ref = _hard(pc, img, P, pc[:, 3], cell, (0.25, 0.0))
        assert ref['count'][0, 0] > 30 and ref['count'][0, 1:].tolist() == [0] * 5
        assert (got.mask[0, 1:] == 0).all() and torch.isinf(got.zmin[0, 1:]).all() and (got.zmin[0, 1:] > 0).all()
        assert (got.occupancy[0, 1:] == 0).all()
        for k in KEYS:
            assert (getattr(got, k)[0, 1:] == 0).all() and not torch.isnan(getattr(got, k)).any()
    got, grad, ref = _soft(pc, img, P, pc[:, 3], 8, (0.25, 0.0))
    assert (grad[0, 1:] == 0).all() and not torch.isnan(grad).any() and grad[0, 0].abs().max() > 0
    # NaN and inf coordinates in the cloud: those points are in no frame, so they neither count nor occlude
    pc[0, 0, ::7] = np.nan
    pc[0, 2, 1::7] = np.inf
    pc[0, 1, 2::7] = -np.inf
    got, ref = _hard(pc, img, P[:, :1], pc[:, 3], 8, (0.0, 0.5))
    assert 10 < ref['count'][0, 0] < 600 * 4 // 7
    _soft(pc, img, P[:, :1], pc[:, 3], 8, (0.0, 0.5))


def test_a_tolerance_that_hides_nothing_is_the_unmasked_path_bit_for_bit():
    pc, img, P = _case(2 * _chunk() + 77, BIG, 70, B=2, K=3)
    value = pc[:, 3].copy()
    value[:, ::5] = np.nan
    t = _cuda(pc, img, P, value)
    A = _api()
    for cell in (1, (6, 2)):
        occ = _occ(cell, (0.0, 1e30))
        for bins in (8, 64):
            a = A.score_visible(t[0], t[1], t[2], occlusion=occ, value=t[3], bins=bins, want_hist=True, want_mask=True)
            b = A.score(t[0], t[1], t[2], value=t[3], bins=bins, want_hist=True)
            assert torch.equal(a.hist, b.hist) and torch.equal(a.count, b.count) and b.count.min() > 100
            for k in KEYS[:5]:
                assert torch.equal(getattr(a, k).view(torch.int64), getattr(b, k).view(torch.int64)), k
            assert (A.Visibility(a.mask, a.zmin, pc.shape[2]).unpack().cpu().numpy() == SV.visible(pc, P, 48, 64, cell, 0.0, 1e30)['frame']).all()
            assert torch.equal(A.miller_madow(b).view(torch.int64), a.mi_mm.view(torch.int64)) and torch.equal(A.occupancy(b.hist), a.occupancy)
            for pool in (False, True):
                Ta, Tb = t[2].clone().requires_grad_(), t[2].clone().requires_grad_()
                a = A.score_soft_visible(t[0], t[1], Ta, occlusion=occ, value=t[3], bins=bins, pool=pool, want_hist=True)
                b = A.score_soft(t[0], t[1], Tb, value=t[3], bins=bins, pool=pool, want_hist=True)
                a.mi.sum().backward()
                b.mi.sum().backward()
                assert torch.equal(a.hist, b.hist) and torch.equal(a.count, b.count)
                assert torch.equal(a.mi.detach().view(torch.int64), b.mi.detach().view(torch.int64))
                assert torch.equal(Ta.grad.view(torch.int64), Tb.grad.view(torch.int64)) and Tb.grad.abs().max() > 0
                assert torch.equal(A.miller_madow(b).detach().view(torch.int64), a.mi_mm.detach().view(torch.int64))


def test_pooled_batch_is_the_sum_of_the_samples():
    pc, img, P = _case(1500, BIG, 15, B=3, K=2)
    for bins, cell, tol in ((8, 8, TOLS[1]), (64, (6, 2), TOLS[2])):
        got, grad, ref = _soft(pc, img, P, pc[:, 3], cell, tol, bins=bins, pool=True)
        each = SV.score_soft_visible(pc, img, P, pc[:, 3], 0.0, 1.0, bins, cell, tol[0], tol[1], want_grad=False)
        assert tuple(got.hist.shape) == (2, bins, bins) and tuple(got.mi.shape) == (2,) and tuple(got.occupancy.shape) == (2, 3)
        assert tuple(got.mask.shape) == (3, 2, 47) and tuple(got.zmin.shape)[:2] == (3, 2)       # the mask stays per (b, k)
        assert (got.hist.cpu().numpy() == each['hist'].sum(0)).all() and (got.count.cpu().numpy() == each['count'].sum(0)).all()
        assert np.abs(ref['grad']).max() > 0 and 0 < ref['count'].min() < ref['frame'].sum((0, 2)).min()


def test_strided_cloud_and_value():
    """the cloud is rows 1..4 of a 6-row tensor and every second point of it, the value a column of a (B,N,3) tensor"""
    N, B, K = 1031, 3, 2
    pc, img, P = _case(N, BIG, 20, B=B, K=K)
    big = torch.zeros(B, 6, 2 * N, device='cuda')
    big[:, 1:5, ::2] = torch.from_numpy(pc).cuda()
    val3 = torch.rand(B, N, 3, device='cuda') * 1.5 - 0.25
    view, val = big[:, 1:5, ::2], val3[:, :, 1]
    assert view.stride(2) == 2 and val.stride(1) == 3
    keep = big.clone(), val3.clone()
    occ = _occ((6, 2), (0.25, 0.0))
    im, T = _cuda(img, P)
    got = _api().score_visible(view, im, T, occlusion=occ, value=val, bins=16, want_hist=True, want_mask=True)
    _same(got, SV.score_visible(pc, img, P, val.cpu().numpy(), 0.0, 1.0, 16, (6, 2), 0.25))
    T.requires_grad_()
    got = _api().score_soft_visible(view, im, T, occlusion=occ, want_hist=True, want_mask=True)           # value=None is row 3 of the view
    got.mi.sum().backward()
    _same(got, SV.score_soft_visible(pc, img, P, pc[:, 3], 0.0, 1.0, 32, (6, 2), 0.25, chunk=_chunk()), T.grad)
    v = _api().visible_mask(view, (48, 64), T.detach(), occ)
    assert torch.equal(v.mask, got.mask)
    assert torch.equal(keep[0], big) and torch.equal(keep[1], val3)


def test_float32_leaf_and_non_uniform_upstream():
    pc, img, P = _case(2000, BIG, 60, B=3, K=5)
    t = _cuda(pc, img)
    P32 = P.astype(np.float32)
    ref = SV.score_soft_visible(pc, img, P32.astype(np.float64), pc[:, 3], 0.0, 1.0, 32, 8, 0.25, chunk=_chunk())
    T = torch.from_numpy(P32).cuda().requires_grad_()
    got = _api().score_soft_visible(*t, T, occlusion=_occ(8, (0.25, 0.0)), want_hist=True, want_mask=True)
    up = torch.tensor(np.random.RandomState(61).randn(3, 5), device='cuda')
    (got.mi_mm * up).sum().backward()                                # mi_mm is mi minus a constant: the same gradient
    assert T.grad.dtype == torch.float32 and tuple(T.grad.shape) == (3, 5, 3, 4)
    want = ref['grad'] * up.cpu().numpy()[:, :, None, None]
    # the product and the conversion to float32 round once each on top of the gradient's own bound
    tol = ref['grad_bound'] * np.abs(up.cpu().numpy())[:, :, None, None] + np.abs(want) * (2.0 ** -24 + 2.0 ** -52)
    err = np.abs(T.grad.cpu().numpy().astype(np.float64) - want)
    assert (err <= tol).all() and np.abs(want).max() > 0, (err.max(), tol.flat[err.argmax()])
    _same(got, ref)
    plain = _api().score_soft_visible(*t, torch.from_numpy(P).cuda())
    assert not plain.mi.requires_grad and plain.mi.grad_fn is None and plain.hist is None and plain.mask is None and plain.zmin is None
    with torch.no_grad():
        assert not _api().score_soft_visible(*t, T).mi.requires_grad


def test_two_runs_same_bits_inputs_untouched():
    pc, img, P = _case(3 * _chunk() + 17, BIG, 70, B=2, K=5)
    value = pc[:, 3].copy()
    for kw in (dict(bins=64), dict(bins=32, pool=True)):
        arrs = (pc, img, P, value)
        t = _cuda(*arrs)
        runs = []
        for _ in range(2):
            T = t[2].clone().requires_grad_()
            s = _api().score_soft_visible(t[0], t[1], T, occlusion=_occ((6, 2), (0.02, 0.1)), value=t[3], want_hist=True, want_mask=True, **kw)
            s.mi.sum().backward()
            h = _api().score_visible(t[0], t[1], t[2], occlusion=_occ((6, 2), (0.02, 0.1)), value=t[3], want_hist=True, want_mask=True, bins=kw['bins'])
            runs.append([getattr(x, k).detach() for x in (s, h) for k in KEYS + ('count', 'hist', 'occupancy', 'mask', 'zmin')] + [T.grad])
        for a, b in zip(*runs):
            assert a.data_ptr() != b.data_ptr()
            assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a.view(torch.int32), b.view(torch.int64) if b.dtype == torch.float64 else b.view(torch.int32))
        assert runs[0][-1].abs().max() > 0
        for a, b in zip(t, arrs):
            assert (a.cpu().numpy().view(np.uint8) == b.view(np.uint8)).all()


def test_errors_name_the_value_and_launch_nothing():
    from efgh_amd import _C
    A = _api()
    pc, img, P = _case(64, BIG, 90, B=2, K=2)
    t = dict(pc=torch.from_numpy(pc).cuda(), img=torch.from_numpy(img).cuda(), T=torch.from_numpy(P).cuda())
    for who, fn in (('score_visible', A.score_visible), ('score_soft_visible', A.score_soft_visible)):
        for name, kw in (('bins', dict(bins=24)), ('pc', dict(pc=t['pc'].cpu())), ('cam_T_velo', dict(T=t['T'].cpu())), ('occlusion', dict(occlusion=8)),
                         ('value_range', dict(value_range=(1.0, 0.0))), ('min_depth', dict(min_depth=-1.0))):
            a, kw = dict(t), dict(kw)
            a.update({k: kw.pop(k) for k in list(kw) if k in a})
            with pytest.raises(_C.EfghError, match=r'%s: %s\b' % (who, name)):
                fn(a['pc'], a['img'], a['T'], **kw)
    with pytest.raises(_C.EfghError, match=r'occupancy: hist: .*CPU tensor'):
        A.occupancy(torch.zeros(2, 8, 8, dtype=torch.int32))
    with pytest.raises(_C.EfghError, match=r'visible_mask: cam_T_velo\b'):
        A.visible_mask(t['pc'], (48, 64), t['T'].cpu())
    # the C entry points check for themselves, in front of the first launch
    L, st = _C.lib(), _C.stream_ptr
    p, v, P0, im = t['pc'], t['pc'][:, 3], t['T'].contiguous(), t['img']
    zmin = torch.full((2, 2, 6, 8), -7, dtype=torch.int32, device='cuda')
    mask = torch.full((2, 2, 2), -7, dtype=torch.int32, device='cuda')
    hist = torch.full((2, 2, 8, 8), -7, dtype=torch.int32, device='cuda')
    occ = torch.full((4, 3), -7, dtype=torch.int32, device='cuda')

    def head(K=2, ch=8, cw=8, min_depth=0.0):
        return (_C.ptr(p), p.stride(0), p.stride(1), 2, 64, _C.ptr(P0), K, 48, 64, ch, cw, min_depth)
    for kw, word in ((dict(ch=0), b'cell_h = 0'), (dict(cw=65), b'cell_w = 65'), (dict(K=4097), b'K = 4097'), (dict(min_depth=-1.0), b'min_depth')):
        assert L.efgh_score_zmin(*head(**kw), _C.ptr(zmin), st()) != 0 and word in L.efgh_last_error(), L.efgh_last_error()
        assert L.efgh_score_visible(*head(**kw), 0.0, 0.0, _C.ptr(zmin), _C.ptr(mask), st()) != 0 and word in L.efgh_last_error()
    assert L.efgh_score_visible(*head(), -1.0, 0.0, _C.ptr(zmin), _C.ptr(mask), st()) != 0 and b'rel_tol = -1' in L.efgh_last_error()
    assert L.efgh_score_hist_masked(_C.ptr(p), p.stride(0), p.stride(1), 2, 64, _C.ptr(v), v.stride(0), _C.ptr(P0), 2, _C.ptr(im), 48, 64, 8, 0.0, 1.0,
                                    0.0, None, _C.ptr(hist), st()) != 0 and b'mask' in L.efgh_last_error()
    assert L.efgh_score_occupancy(_C.ptr(hist), 4, 12, _C.ptr(occ), st()) != 0 and b'bins = 12' in L.efgh_last_error()
    torch.cuda.synchronize()
    assert (zmin == -7).all() and (mask == -7).all() and (hist == -7).all() and (occ == -7).all()
    _hard(pc, img, P, pc[:, 3], 8)                                 # and the library goes on working


def test_refine_through_a_partial_of_the_visible_scorer():
    A = _api()
    pc, img, P, value = peak_case()
    Pst = start_pose(P[0, 0], STARTS[0])
    t = _cuda(pc, img, Pst[None])
    val = torch.from_numpy(value).cuda()
    scorer = functools.partial(A.score_soft_visible, occlusion=_occ((8, 2), (0.02, 0.1)))
    kw = dict(value=val, value_range=(0.0, 256.0), bins=PEAK['bins'], scorer=scorer)
    r = A.refine(*t, iters=30, rot_step_deg=0.2, trans_step=0.02, **kw)
    assert r.pose.is_cuda and r.pose.dtype == torch.float64 and tuple(r.pose.shape) == (1, 3, 4) and tuple(r.trace.shape) == (30, 1)
    trace = r.trace.cpu().numpy()[:, 0]
    print('mi %.4f -> %.4f at iterate %d' % (float(r.start_mi), float(r.mi), int(r.best_iter)))
    assert int(r.best_iter) == int(trace.argmax()) and float(r.mi) == trace.max() and float(r.start_mi) == trace[0]
    assert float(r.mi) >= float(r.start_mi)
    # the first iterate is scored as the scorer scores P0, and the pose handed back scores what `refine` says
    first = scorer(t[0], t[1], t[2], value=val, value_range=(0.0, 256.0), bins=PEAK['bins'])
    assert torch.equal(first.mi[:, 0], r.start_mi) and 0 < int(first.count) < PEAK['N']
    again = scorer(t[0], t[1], r.pose, value=val, value_range=(0.0, 256.0), bins=PEAK['bins'])
    assert torch.equal(again.mi[:, 0], r.mi)
    # iterate 0 is P0 bit for bit; pooled, one parameter set
    r1 = A.refine(*t, iters=1, **kw)
    assert torch.equal(r1.pose.view(torch.int64), t[2].view(torch.int64)) and r1.best_iter.tolist() == [0] and torch.equal(r1.mi, r.start_mi)
    r2 = A.refine(*t, iters=2, pool=True, **kw)
    assert tuple(r2.mi.shape) == (1,) and float(r2.mi) >= float(r2.start_mi)
