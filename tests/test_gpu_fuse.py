"""csrc/fuse.hip through efgh_amd.common.fuse against tests/fuse_contract.py, bit for bit: state, rgb and index as integers, depth and
uv as their float32 bit patterns (NaN compared as "is NaN").  Small shapes: the four-point store residues, the workgroup boundary,
real strides, collisions on one pixel, clipped windows, the frame and depth edges with exactly representable projections."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_contract as FC  # noqa: E402

pytestmark = pytest.mark.gpu
WANT = ('rgb', 'state', 'uv', 'depth', 'index')
H, W = 37, 53
IDENT = np.array([[[1., 0, 0, 0], [0, 1., 0, 0], [0, 0, 1., 0]]])


def _fuse(*a, **kw):
    from efgh_amd.common import fuse
    return fuse(*a, **kw)


def _same(got, ref, want=WANT):
    for k in WANT:
        t = getattr(got, k)
        if k not in want:
            assert t is None, k
            continue
        a, r = t.cpu().numpy(), ref[k]
        assert a.shape == r.shape and a.dtype == r.dtype, (k, a.shape, r.shape, a.dtype, r.dtype)
        if a.dtype == np.float32:
            assert (np.isnan(a) == np.isnan(r)).all(), k
            a, r = np.where(np.isnan(a), np.float32(0), a).view(np.int32), np.where(np.isnan(r), np.float32(0), r).view(np.int32)
        bad = np.argwhere(a != r)
        assert bad.shape[0] == 0, (k, bad.shape[0], bad[:4].tolist())


def _check(pc, img, P, want=WANT, **kw):
    """numpy pc (B,C,N) float32, img uint8 (B,H,W,3), P (B,3,4) float64 -> (Fused, the contract's dict), compared"""
    got = _fuse(torch.from_numpy(pc).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(P).cuda(), want=want, **kw)
    ref = FC.fuse(pc, img, P, **kw)
    _same(got, ref, want)
    return got, ref


def _image(B, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (B, h, w, 3)).astype(np.uint8)


def _case(N, h, w, seed, B=1, C=3):
    """a camera-like matrix per sample and points back-projected from drawn (u, v, depth): about a third out of frame, a
    twentieth behind the camera"""
    rs = np.random.RandomState(seed)
    P = np.zeros((B, 3, 4))
    pc = np.zeros((B, C, N), np.float32)
    for b in range(B):
        P[b] = np.array([[40., 0, w / 2, 0.3], [0, 40., h / 2, -0.2], [0, 0, 1., 0.1]]) + 0.05 * rs.randn(3, 4)
        d = 1.0 + 29.0 * rs.rand(N)
        d[rs.rand(N) < 0.05] *= -1
        u, v = (rs.rand(N) * 1.2 - 0.1) * w, (rs.rand(N) * 1.2 - 0.1) * h
        tgt = np.stack([u * d, v * d, d]) - P[b][:, 3:]
        pc[b, :3] = np.linalg.solve(P[b][:, :3], tgt).astype(np.float32)
        if C > 3:
            pc[b, 3:] = rs.rand(C - 3, N)
    return pc, _image(B, h, w, seed + 1), P


def _pts(uvw):
    """[(u, v, w)] with exactly representable products -> (1,3,N) cloud for IDENT"""
    a = np.array([[u * w, v * w, w] for u, v, w in uvw], dtype=np.float64).T
    assert (a.astype(np.float32).astype(np.float64) == a).all()
    return a.astype(np.float32)[None]


@pytest.mark.parametrize('N', [1, 2, 3, 4, 5, 255, 256, 257, 4099])
def test_sizes(N):
    pc, img, P = _case(N, H, W, 10 + N)
    got, ref = _check(pc, img, P)
    if N >= 255:
        assert len(np.unique(ref['state'])) == 4


def test_one_pixel_image():
    got, ref = _check(_pts([(0.5, 0.25, 2.0)]), np.array([[[[7, 8, 9]]]], np.uint8), IDENT)
    assert ref['state'].tolist() == [[3]] and ref['rgb'].tolist() == [[[7, 8, 9]]] and ref['index'].tolist() == [[[0]]]


def test_batch_and_strides():
    pc, img, P = _case(1031, H, W, 20, B=3, C=4)
    P[1, 0] += 1e4 * P[1, 2]                                     # sample 1: every u moves 10^4 pixels to the right
    got, ref = _check(pc, img, P, radius=1, rel_tol=0.01)
    assert (ref['state'][1] <= 1).all() and (ref['index'][1] == -1).all() and (ref['state'][0] >= 2).sum() > 300
    # a view with real strides (the cloud is rows 1..4 of a 6-row tensor), float32 matrices, the model's float image
    big = torch.zeros(3, 6, 1031, device='cuda')
    big[:, 1:5] = torch.from_numpy(pc).cuda()
    P32 = P.astype(np.float32)
    imf = torch.from_numpy(img).cuda().permute(0, 3, 1, 2).float() + 0.75
    got = _fuse(big[:, 1:5], imf, {'cam_T_velo': torch.from_numpy(P32).cuda()}, radius=1, rel_tol=0.01)
    _same(got, FC.fuse(pc, FC.u8_hwc(imf.cpu().numpy()), P32.astype(np.float64), radius=1, rel_tol=0.01))


def test_collisions_on_one_pixel():
    img = _image(1, H, W, 30)
    # the nearer point at the higher index
    got, ref = _check(_pts([(5.5, 7.5, 8.0), (5.25, 7.75, 2.0)]), img, IDENT)
    assert ref['state'].tolist() == [[2, 3]] and ref['index'][0, 7, 5] == 1 and ref['depth'][0, 7, 5] == 2.0
    # float64 depths 4 + 2^-40 and 4: one float32 depth, so the lower index wins the pixel and both are visible
    P = np.array([[[1., 0, 0, 0], [0, 0, 0, 10.], [0, 2.0 ** -40, 1., 0]]])
    pc = np.array([[[10., 10.], [1., 0.], [4., 4.]]], np.float32)
    got, ref = _check(pc, img, P)
    assert ref['state'].tolist() == [[3, 3]] and ref['index'][0, 2, 2] == 0 and (ref['index'] >= 0).sum() == 1
    # 4096 points on ONE pixel, the depths distinct and descending: the last one wins
    P = np.array([[[0, 0, 5.5, 0], [0, 0, 7.5, 0], [0, 0, 1., 0]]])
    pc = np.zeros((1, 3, 4096), np.float32)
    pc[0, 2] = (4096 - np.arange(4096)) / 16.0
    got, ref = _check(pc, img, P)
    assert ref['index'][0, 7, 5] == 4095 and (ref['index'] >= 0).sum() == 1
    assert (ref['state'][0, :4095] == 2).all() and ref['state'][0, 4095] == 3


def test_radius_and_tolerances():
    img = _image(1, H, W, 40)
    pc = _pts([(5.5, 5.5, 2.0), (6.5, 6.5, 10.0)])              # foreground on pixel (5,5), background on (6,6)
    assert _check(pc, img, IDENT, radius=0)[1]['state'].tolist() == [[3, 3]]
    assert _check(pc, img, IDENT, radius=1)[1]['state'].tolist() == [[3, 2]]
    # the bound 2 (1 + rel_tol) + abs_tol is the background's depth exactly: visible, by <=
    assert _check(pc, img, IDENT, radius=1, rel_tol=4.0)[1]['state'].tolist() == [[3, 3]]
    assert _check(pc, img, IDENT, radius=1, abs_tol=8.0)[1]['state'].tolist() == [[3, 3]]
    assert _check(pc, img, IDENT, radius=1, rel_tol=1.5, abs_tol=5.0)[1]['state'].tolist() == [[3, 3]]
    assert _check(pc, img, IDENT, radius=1, abs_tol=8.0 - 2.0 ** -40)[1]['state'].tolist() == [[3, 2]]
    # windows clipped at two corners
    pc = _pts([(0.5, 0.5, 3.0), (W - 0.5, H - 0.5, 4.0)])
    got, ref = _check(pc, img, IDENT, radius=8)
    assert (ref['index'] == 0).sum() == 81 and (ref['index'] == 1).sum() == 81 and (ref['index'] >= 0).sum() == 162
    assert (ref['index'][0, :9, :9] == 0).all() and (ref['index'][0, H - 9:, W - 9:] == 1).all()


def test_frame_and_depth_edges():
    img = _image(1, H, W, 50)
    inf, nan = np.inf, np.nan
    pc = _pts([(0.0, 3.5, 2.0), (float(W), 3.5, 2.0), (3.5, -0.25, 2.0), (3.5, float(H), 4.0), (W - 0.25, 0.0, 2.0),
               (3.5, 3.5, 0.5), (3.5, 3.5, 0.25), (3.5, 3.5, 1.0)])
    got, ref = _check(pc, img, IDENT, min_depth=0.5)
    assert ref['state'].tolist() == [[3, 1, 1, 1, 3, 0, 0, 3]]      # w == min_depth is not in front: the comparison is strict
    assert ref['index'][0, 3, 0] == 0 and ref['index'][0, 0, W - 1] == 4
    raw = np.array([[7., 7., -2.], [7., 7., 0.], [0., 0., 0.], [nan, 7., 2.], [7., nan, 2.], [7., 7., nan], [inf, 7., 2.],
                    [7., -inf, 2.], [7., 7., inf], [7., 7., -inf], [inf, inf, inf], [7., 7., 2.]], np.float32).T[None]
    got, ref = _check(np.ascontiguousarray(raw), img, IDENT)
    assert ref['state'].tolist() == [[0] * 11 + [3]]
    assert np.isnan(ref['uv'][0, :11]).all() and ref['uv'][0, 11].tolist() == [3.5, 3.5]


def test_bilinear_rounding_and_nearest():
    img = np.array([[[[0, 0, 0], [1, 1, 1]]]], dtype=np.uint8)    # 1 x 2: neighbours 0 and 1, tx = 0.5 -> 0.5 + 0.5 -> 1
    got, ref = _check(_pts([(1.0, 0.5, 2.0)]), img, IDENT)
    assert ref['rgb'].tolist() == [[[1, 1, 1]]]
    rs = np.random.RandomState(60)
    n = 3000
    u, v, d = rs.rand(n) * W, rs.rand(n) * H, 1 + rs.rand(n)
    pc = np.stack([u * d, v * d, d]).astype(np.float32)[None]
    img = _image(1, H, W, 61)
    got, ref = _check(pc, img, IDENT, bilinear=True)
    _, near = _check(pc, img, IDENT, bilinear=False)
    assert (ref['rgb'] != near['rgb']).any(1).mean() > 0.5
    p = FC.project(pc[0], IDENT[0], H, W)
    assert (near['rgb'][0][p['frame']] == img[0][p['r'][p['frame']], p['c'][p['frame']]]).all()


@pytest.fixture(scope='module')
def random_case():
    pc, img, P = _case(4099, H, W, 70, C=4)
    return pc, img, P, FC.fuse(pc, img, P, radius=1, rel_tol=0.02, abs_tol=0.05, min_depth=1.5)


def test_random_case_all_outputs_twice_inputs_untouched(random_case):
    pc, img, P, ref = random_case
    assert (ref['state'] <= 1).mean() > 0.25 and (ref['state'] == 2).sum() > 200 and (ref['state'] == 3).sum() > 200
    t = [torch.from_numpy(a).cuda() for a in (pc, img, P)]
    kw = dict(radius=1, rel_tol=0.02, abs_tol=0.05, min_depth=1.5)
    one, two = _fuse(*t, **kw), _fuse(*t, **kw)
    _same(one, ref)
    for k in WANT:
        a, b = getattr(one, k), getattr(two, k)
        assert a.data_ptr() != b.data_ptr()
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    assert torch.equal(one.visible, one.state == 3)
    for a, b in zip(t, (pc, img, P)):
        assert (a.cpu().numpy().view(np.uint8) == b.view(np.uint8)).all()


SUBSETS = [c for k in range(1, len(WANT)) for c in itertools.combinations(WANT, k)]


@pytest.mark.parametrize('subset', SUBSETS, ids=['+'.join(c) for c in SUBSETS])
def test_random_case_each_subset_of_the_outputs(random_case, subset):
    pc, img, P, ref = random_case
    got = _fuse(torch.from_numpy(pc).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(P).cuda(), radius=1, rel_tol=0.02,
                abs_tol=0.05, min_depth=1.5, want=subset)
    _same(got, ref, subset)


def _summary_case():
    """a cloud back-projected through the synthetic calibration from chosen (u, v, integer depth): every projected coordinate is,
    by the contract, at least 1e-3 px from an integer and from the frame, so that `x / w < W` and `x < w * W` cannot disagree"""
    from efgh_amd import synthetic as syn
    h, w, n = 48, 96, 1500
    calib, _ = syn.calib_and_A((h, w))
    rs = np.random.RandomState(80)
    d = rs.randint(1, 201, n).astype(np.float64)
    u = rs.randint(-8, w + 8, n) + 0.05 + 0.9 * rs.rand(n)
    v = rs.randint(-6, h + 6, n) + 0.05 + 0.9 * rs.rand(n)
    cam = np.stack([(u - w / 2) * d / 600.0, (v - h / 2) * d / 600.0, d])          # calib = K [camera <- lidar axes]
    pc = np.stack([cam[2], -cam[0], -cam[1]]).astype(np.float32)
    p = FC.project(pc, calib, h, w)
    for c, size in ((p['u'], w), (p['v'], h)):
        assert (np.abs(c - np.round(c)) >= 1e-3).all() and (np.abs(c) >= 1e-3).all() and (np.abs(c - size) >= 1e-3).all()
    assert (p['d'] == d).all() and 0.3 < p['frame'].mean() < 0.9
    return pc, calib, h, w


def test_occupancy_is_the_last_wins_rasters():
    from efgh_amd.common import summary
    pc, calib, h, w = _summary_case()
    t = torch.from_numpy(pc).cuda()
    last = summary.depth_image_last(t, calib, (h, w)).cpu().numpy()
    got = _fuse(t[None], torch.zeros(h, w, 3, dtype=torch.uint8, device='cuda'), torch.from_numpy(calib[None]).cuda(),
                want=('index', 'depth'))
    idx, dep = got.index[0].cpu().numpy(), got.depth[0].cpu().numpy()
    assert ((idx >= 0) == (last != 0)).all() and 500 < (idx >= 0).sum()
    assert (dep[idx >= 0] <= last[idx >= 0]).all() and (dep[idx >= 0] < last[idx >= 0]).any()      # nearest against last


def test_errors_name_the_argument_and_launch_nothing():
    from efgh_amd import _C
    pc, img, P = _case(64, H, W, 90, B=2)
    t = dict(pc=torch.from_numpy(pc).cuda(), img=torch.from_numpy(img).cuda(), T=torch.from_numpy(P).cuda())
    bad = [('radius', dict(radius=-1)), ('radius', dict(radius=9)), ('pc', dict(pc=t['pc'].cpu())), ('img', dict(img=t['img'].cpu())),
           ('cam_T_velo', dict(T=t['T'].cpu())), ('pc', dict(pc=t['pc'].half())), ('cam_T_velo', dict(T=t['T'][:, :, :3])),
           ('img', dict(img=t['img'][:1])), ('abs_tol', dict(abs_tol=-1.0))]
    for name, kw in bad:
        a = dict(t)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        with pytest.raises(_C.EfghError, match=r'fuse: %s\b' % name):
            _fuse(a['pc'], a['img'], a['T'], **kw)
        torch.cuda.synchronize()
    # the C entry points check for themselves, in front of the first launch
    L, z = _C.lib(), torch.empty(H * W, dtype=torch.int64, device='cuda')
    p, P0 = t['pc'], t['T'].contiguous()
    for radius, min_depth in ((9, 0.0), (-1, 0.0), (0, -1.0), (0, float('nan'))):
        assert L.efgh_fuse_zbuffer(_C.ptr(p), p.stride(0), p.stride(1), 1, 64, _C.ptr(P0), H, W, radius, min_depth, _C.ptr(z), _C.stream_ptr()) != 0
        assert b'efgh_fuse_zbuffer' in L.efgh_last_error()
    assert L.efgh_fuse_zbuffer(_C.ptr(p), p.stride(0), p.stride(1), 1, 64, _C.ptr(P0), H, W, 0, 0.0, None, _C.stream_ptr()) != 0
    assert L.efgh_fuse_maps(_C.ptr(z), 1, H * W, None, None, _C.stream_ptr()) != 0
    assert L.efgh_fuse_workspace_bytes(2, H, W) == 16 * H * W and L.efgh_fuse_workspace_bytes(1, 65536, 65536) == -1
    torch.cuda.synchronize()
    _check(pc, img, P)                                           # and the library goes on working
