"""csrc/score.hip through efgh_amd.common.score against tests/score_contract.py: `hist` and `count` EXACTLY, mi / nmi / the entropies
inside the bound the contract derives (score_contract.bounds; never fitted to an output).  Small shapes: the wave and block
boundaries, one point either side of the kernel's chunk, several candidates and samples, both ends of the bin range, real strides,
4096 points in one cell, empty histograms, NaN / inf in poses and values, every accepted input form."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_contract as FC  # noqa: E402
import score_contract as SC  # noqa: E402
from test_score_host import PEAK, cloud, image, peak_case  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ('mi', 'nmi', 'hx', 'hy', 'hxy')
SMALL, BIG = (5, 7), (48, 64)
# every K of {1, 2, 5}, B of {1, 3}, bins of {8, 64} and both image sizes, at every N
COMBOS = [(1, 1, 8, SMALL), (2, 3, 64, BIG), (5, 1, 64, SMALL), (5, 3, 8, BIG), (1, 3, 64, BIG), (2, 1, 8, BIG)]


def _score(*a, **kw):
    from efgh_amd.common import score
    return score(*a, **kw)


def _chunk():
    from efgh_amd import _C
    return int(_C.lib().efgh_score_chunk())


def _same(got, ref, bins):
    hist, count = got.hist.cpu().numpy(), got.count.cpu().numpy()
    assert hist.dtype == np.int32 and hist.shape == ref['hist'].shape and count.dtype == np.int32 and count.shape == ref['count'].shape
    bad = np.argwhere(hist != ref['hist'])
    assert bad.shape[0] == 0, ('hist', bad.shape[0], bad[:4].tolist())
    assert (count == ref['count']).all(), ('count', count.tolist(), ref['count'].tolist())
    for k in KEYS:
        a = getattr(got, k).cpu().numpy()
        assert a.dtype == np.float64 and a.shape == ref[k].shape and np.isfinite(a).all(), (k, a)
        err, bound = np.abs(a - ref[k]), ref['bound'][k]
        print('%s: largest error %.3e, its bound %.3e, smallest bound / error %.1f'
              % (k, err.max(), bound.flat[err.argmax()], (bound[err > 0] / err[err > 0]).min() if (err > 0).any() else np.inf))
        assert (err <= bound).all(), (k, err.max(), bound.flat[err.argmax()])
        assert (a[ref['count'] == 0] == 0).all(), k


def _check(pc, img, P, value, lo=0.0, hi=1.0, bins=32, min_depth=0.0):
    """numpy pc (B,C,N) float32, img uint8 (B,H,W,3), P (B,K,3,4) float64, value (B,N) float32 -> (Score, the contract's dict)"""
    got = _score(torch.from_numpy(pc).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(P).cuda(), value=torch.from_numpy(value).cuda(),
                 value_range=(lo, hi), bins=bins, min_depth=min_depth, want_hist=True)
    ref = SC.score(pc, img, P, value, lo, hi, bins, min_depth)
    _same(got, ref, bins)
    return got, ref


def _case(N, hw, seed, B=1, K=1, C=4):
    """a cloud and a pinhole matrix per sample; candidate 0 is that matrix, the others move it by a few pixels and a little noise"""
    h, w = hw
    rs = np.random.RandomState(seed + 1000)
    pcs, Ps = [], []
    for b in range(B):
        pc, P0 = cloud(N, h, w, seed + b, C=C)
        cand = [P0]
        for k in range(1, K):
            Q = P0 + 0.01 * rs.randn(3, 4)
            Q[0] += rs.randint(-3, 4) * P0[2]
            Q[1] += rs.randint(-2, 3) * P0[2]
            cand.append(Q)
        pcs.append(pc)
        Ps.append(np.stack(cand))
    imgs = np.stack([image(h, w, seed + 50 + b) for b in range(B)])
    return np.stack(pcs), imgs, np.stack(Ps)


@pytest.mark.parametrize('N', [1, 63, 64, 65, 255, 256, 257, 1000, 'chunk-1', 'chunk+0', 'chunk+1'])
def test_sizes(N):
    n = _chunk() + int(N[5:]) if isinstance(N, str) else N
    seen = 0
    for j, (K, B, bins, hw) in enumerate(COMBOS):
        pc, img, P = _case(n, hw, 10 * j + n % 97, B=B, K=K)
        got, ref = _check(pc, img, P, pc[:, 3], 0.0, 1.0, bins)
        seen += int(ref['count'].sum())
    assert seen >= (n if n > 1 else 0)


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
    got = _score(view, torch.from_numpy(img).cuda(), torch.from_numpy(P).cuda(), value=val, bins=16, want_hist=True)
    ref = SC.score(pc, img, P, val.cpu().numpy(), 0.0, 1.0, 16)
    _same(got, ref, 16)
    assert ref['hist'][:, :, 0].sum() > 100 and ref['hist'][:, :, 15].sum() > 100
    # value=None is row 3 of the view; a view with a batch stride of its own
    got = _score(view, torch.from_numpy(img).cuda(), torch.from_numpy(P).cuda(), want_hist=True)
    _same(got, SC.score(pc, img, P, pc[:, 3], 0.0, 1.0, 32), 32)
    wide = torch.zeros(B, 2 * N, device='cuda')
    wide[:, :N] = torch.from_numpy(pc[:, 3]).cuda()
    got = _score(view, torch.from_numpy(img).cuda(), torch.from_numpy(P).cuda(), value=wide[:, :N], want_hist=True)
    _same(got, SC.score(pc, img, P, pc[:, 3], 0.0, 1.0, 32), 32)
    assert torch.equal(keep[0], big) and torch.equal(keep[1], val3)


def test_4096_points_in_one_cell():
    img = image(*BIG, 30)[None]
    P = np.array([[[[0, 0, 5.5, 0], [0, 0, 7.5, 0], [0, 0, 1., 0]]]])
    pc = np.zeros((1, 3, 4096), np.float32)
    pc[0, 2] = (4096 - np.arange(4096)) / 16.0
    value = np.full((1, 4096), 0.3, np.float32)
    for bins in (8, 64):
        got, ref = _check(pc, img, P, value, bins=bins)
        x, y = int(0.3 * bins), (int(SC.luma(img[0, 7, 5])) * bins) >> 8
        assert ref['hist'][0, 0, x, y] == 4096 and ref['hist'].sum() == 4096 and ref['count'].tolist() == [[4096]]
        for k in KEYS:
            assert getattr(got, k).cpu().tolist() == [[0.0]], k


def test_empty_histograms_and_non_finite_poses():
    pc, img, P = _case(600, BIG, 40, B=1, K=6)
    P[0, 1, 0] += 1e4 * P[0, 1, 2]                                 # every u 10^4 pixels to the right: nothing in frame
    P[0, 2, 2] = 0.0                                               # w = 0 for every point: none in front
    P[0, 3, 1, 1] = np.nan
    P[0, 4, 0, 3] = np.inf
    P[0, 5, 2, 3] = -np.inf
    got, ref = _check(pc, img, P, pc[:, 3])
    assert ref['count'][0, 0] > 100 and ref['count'][0, 1:].tolist() == [0] * 5
    for k in KEYS:
        assert (getattr(got, k)[0, 1:] == 0).all() and not torch.isnan(getattr(got, k)).any()
    # NaN and inf coordinates in the cloud: those points drop out, the rest count
    pc[0, 0, ::7] = np.nan
    pc[0, 2, 1::7] = np.inf
    pc[0, 1, 2::7] = -np.inf
    got, ref = _check(pc, img, P[:, :1], pc[:, 3])
    assert 50 < ref['count'][0, 0] < 600 * 4 // 7


def test_nan_and_infinite_values_and_min_depth():
    pc, img, P = _case(1000, BIG, 50, B=2, K=2)
    value = pc[:, 3].copy()
    value[:, ::3] = np.nan
    value[:, 1::9] = np.inf
    value[:, 2::9] = -np.inf
    value[0, 4] = 0.0                                              # v == lo
    value[0, 5] = 1.0                                              # v == hi
    value[0, 7] = np.nextafter(np.float32(1), np.float32(0))
    got, ref = _check(pc, img, P, value, bins=8)
    full = SC.score(pc, img, P, pc[:, 3], 0.0, 1.0, 8)
    assert (ref['count'] < full['count']).all() and (ref['count'] > full['count'] // 2).all()
    _check(pc, img, P, value, lo=0.25, hi=0.5, bins=64, min_depth=12.0)
    _check(pc, img, P, value * 200 - 100, lo=-37.5, hi=61.0, bins=16)


def test_input_forms_float32_poses_uint8_values_float_image():
    pc, img, P = _case(1000, BIG, 60, B=3, K=5)
    t = torch.from_numpy(pc).cuda()
    P32 = P.astype(np.float32)
    v8 = np.random.RandomState(61).randint(0, 256, (3, 1000)).astype(np.uint8)
    imf = torch.from_numpy(img).cuda().permute(0, 3, 1, 2).float() + 0.75
    got = _score(t, imf, torch.from_numpy(P32).cuda(), value=torch.from_numpy(v8).cuda(), value_range=(5.0, 6.0), bins=64, want_hist=True)
    ref = SC.score(pc, FC.u8_hwc(imf.cpu().numpy()), P32.astype(np.float64), v8.astype(np.float32), 0.0, 256.0, 64)
    _same(got, ref, 64)
    assert (ref['hist'].sum((0, 1, 3)) > 0).sum() > 50               # the uint8 values spread over the 64 value bins
    # (B,3,4) is K = 1; want_hist=False hands back no histogram
    got = _score(t, torch.from_numpy(img).cuda(), torch.from_numpy(P[:, 0]).cuda())
    one = SC.score(pc, img, P[:, :1], pc[:, 3], 0.0, 1.0, 32)
    assert got.hist is None and tuple(got.mi.shape) == (3, 1) and (got.count.cpu().numpy() == one['count']).all()
    assert (np.abs(got.mi.cpu().numpy() - one['mi']) <= one['bound']['mi']).all()
    # (H,W,3) with one sample
    got = _score(t[:1], torch.from_numpy(img[0]).cuda(), torch.from_numpy(P[:1]).cuda(), want_hist=True)
    _same(got, SC.score(pc[:1], img[:1], P[:1], pc[:1, 3], 0.0, 1.0, 32), 32)


@pytest.fixture(scope='module')
def peak():
    pc, img, P, value = peak_case()
    return pc, img, P, value, SC.score(pc, img, P, value, 0.0, 256.0, PEAK['bins'])


def test_peak_property_and_best(peak):
    pc, img, P, value, ref = peak
    got = _score(torch.from_numpy(pc).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(P).cuda(), value=torch.from_numpy(value).cuda(),
                 value_range=(0.0, 256.0), bins=PEAK['bins'], want_hist=True)
    _same(got, ref, PEAK['bins'])
    mi = got.mi.cpu().numpy()[0]
    assert (mi[0] > mi[1:]).all()                                  # the true pose, strictly, over every candidate >= 4 px away
    for by in ('mi', 'nmi'):
        best = got.best(by)
        assert best.is_cuda and best.dtype == torch.int64 and best.tolist() == [int(np.argmax(ref[by][0]))], by
    assert got.best().tolist() == [0]
    # uint8 values are the same levels
    got8 = _score(torch.from_numpy(pc).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(P).cuda(),
                  value=torch.from_numpy(value.astype(np.uint8)).cuda(), bins=PEAK['bins'], want_hist=True)
    assert torch.equal(got8.hist, got.hist) and torch.equal(got8.mi, got.mi)


def test_two_runs_same_bits_inputs_untouched(peak):
    pc, img, P, value, ref = peak
    pc2, img2, P2 = _case(3000, BIG, 70, B=2, K=5)
    for arrs, kw in (((pc, img, P, value), dict(value_range=(0.0, 256.0), bins=8)), ((pc2, img2, P2, pc2[:, 3].copy()), dict(bins=64))):
        t = [torch.from_numpy(a).cuda() for a in arrs]
        one = _score(t[0], t[1], t[2], value=t[3], want_hist=True, **kw)
        two = _score(t[0], t[1], t[2], value=t[3], want_hist=True, **kw)
        for k in KEYS + ('count', 'hist'):
            a, b = getattr(one, k), getattr(two, k)
            assert a.data_ptr() != b.data_ptr()
            assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b), k
        for a, b in zip(t, arrs):
            assert (a.cpu().numpy().view(np.uint8) == b.view(np.uint8)).all()


def test_stage_poses_behind_the_model(manifest):
    """the synthetic sample through an eval forward (the small configuration of tests/test_gpu_fuse_model.py): the initial pose and
    the three stages as four candidates, against the contract with the matrices copied to the host"""
    from efgh_amd import synthetic as syn
    from efgh_amd.common import stage_poses
    from efgh_amd.nets import EFGHBackbone
    raw, npts = (128, 256), 2048
    m = EFGHBackbone(syn.default_args(raw, 'cuda'))
    m.load_state_dict(syn.synthetic_state_dict(manifest['state_dict'], 1), strict=True)
    m = m.cuda().eval()
    b = syn.make_batch(raw, npts, 2)
    pcd, img, calib, A = (torch.from_numpy(b[k]).cuda() for k in ('pc', 'img', 'calib', 'A'))
    with torch.no_grad():
        pred = m(pcd, img, calib, A)
    poses, names = stage_poses(pred, calib)
    assert names == ('calib', 'eh_cam_T_velo', 'efh_cam_T_velo', 'efgh_cam_T_velo') and tuple(poses.shape) == (2, 4, 3, 4)
    assert torch.equal(poses[:, 3], pred['cam_T_velo'].to(poses.dtype)) and torch.equal(poses[:, 0], calib.to(poses.dtype))
    cam = img.repeat_interleave(2, 2).repeat_interleave(2, 3)      # the half-size input stands in for the raw-size frame, tiled
    value = torch.sqrt((pcd * pcd).sum(1))                         # the range: the synthetic sweep has no reflectance
    got = _score(pcd, cam, poses, value=value, value_range=(0.0, 32.0), bins=8, want_hist=True)
    ref = SC.score(b['pc'], FC.u8_hwc(cam.cpu().numpy()), poses.cpu().numpy().astype(np.float64), value.cpu().numpy(), 0.0, 32.0, 8)
    _same(got, ref, 8)
    assert (got.count > 0).all() and all(torch.isfinite(getattr(got, k)).all() for k in KEYS)


def test_errors_name_the_value_and_launch_nothing():
    from efgh_amd import _C
    pc, img, P = _case(64, BIG, 90, B=2, K=2)
    t = dict(pc=torch.from_numpy(pc).cuda(), img=torch.from_numpy(img).cuda(), T=torch.from_numpy(P).cuda())
    bad = [('bins', dict(bins=256)), ('bins', dict(bins=24)), ('pc', dict(pc=t['pc'].cpu())), ('img', dict(img=t['img'].cpu())),
           ('cam_T_velo', dict(T=t['T'].cpu())), ('value', dict(value=t['pc'][:, 3].cpu())), ('value', dict(pc=t['pc'][:, :3])),
           ('value_range', dict(value_range=(1.0, 0.0))), ('min_depth', dict(min_depth=-1.0))]
    for name, kw in bad:
        a = dict(t)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        with pytest.raises(_C.EfghError, match=r'score: %s\b' % name):
            _score(a['pc'], a['img'], a['T'], **kw)
        torch.cuda.synchronize()
    with pytest.raises(_C.EfghError, match='bins: 256'):
        _score(t['pc'], t['img'], t['T'], bins=256)
    # the C entry points check for themselves, in front of the first launch, and name the value
    L, st = _C.lib(), _C.stream_ptr
    h, w = BIG
    p, v, P0, im = t['pc'], t['pc'][:, 3], t['T'].contiguous(), t['img']
    hist = torch.full((2, 2, 64, 64), -7, dtype=torch.int32, device='cuda')
    out, cnt = torch.empty(2, 2, 5, dtype=torch.float64, device='cuda'), torch.empty(2, 2, dtype=torch.int32, device='cuda')

    def call(B=2, N=64, K=2, bins=8, lo=0.0, hi=1.0, min_depth=0.0, hist_=hist):
        return L.efgh_score_hist(_C.ptr(p), p.stride(0), p.stride(1), B, N, _C.ptr(v), v.stride(0), _C.ptr(P0), K, _C.ptr(im), h, w, bins,
                                 lo, hi, min_depth, _C.ptr(hist_), st())
    for kw, word in ((dict(bins=256), b'bins = 256'), (dict(bins=12), b'bins = 12'), (dict(K=4097), b'K = 4097'), (dict(K=0), b'K = 0'),
                     (dict(B=65536), b'B = 65536'), (dict(N=0), b'N = 0'), (dict(lo=1.0, hi=1.0), b'lo = 1'), (dict(hi=float('inf')), b'hi = inf'),
                     (dict(min_depth=float('nan')), b'min_depth'), (dict(hist_=None), b'null pointer')):
        assert call(**kw) != 0
        assert b'efgh_score_hist' in L.efgh_last_error() and word in L.efgh_last_error(), (kw, L.efgh_last_error())
    for kw, word in ((dict(bins=128), b'bins = 128'), (dict(K=4097), b'K = 4097'), (dict(B=0), b'B = 0')):
        a = dict(B=2, K=2, bins=8)
        a.update(kw)
        assert L.efgh_score_mi(_C.ptr(hist), a['B'], a['K'], a['bins'], _C.ptr(out), _C.ptr(cnt), st()) != 0
        assert b'efgh_score_mi' in L.efgh_last_error() and word in L.efgh_last_error()
    torch.cuda.synchronize()
    assert (hist == -7).all()                                      # nothing was launched, not even the zeroing
    assert _chunk() > 0 and _chunk() % 256 == 0
    _check(pc, img, P, pc[:, 3])                                   # and the library goes on working
