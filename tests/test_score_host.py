"""tests/score_contract.py held to properties that are not taken from it (no GPU): totals against fuse_contract's frame mask, marginals
against np.bincount, permutation invariance, the value-bin edges, the entropy identities of a bijective and of an independent pair,
the peak property the whole feature rests on; `candidates_around` and the argument refusals of `score`, which need no device."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_contract as FC  # noqa: E402
import score_contract as SC  # noqa: E402
from efgh_amd.common import Score, candidates_around, score, stage_poses  # noqa: E402  (the feature under test: no CPU path, but it imports and checks)


def pinhole(h, w, f=40.0):
    return np.array([[f, 0, w / 2, 0.3], [0, f, h / 2, -0.2], [0, 0, 1., 0.1]])


def cloud(N, h, w, seed, C=4, margin=0.1):
    """points back-projected through pinhole(h, w) from drawn (u, v, depth): a part out of frame, a twentieth behind the camera;
    row 3 (C >= 4) is a reflectance in [0, 1)"""
    rs = np.random.RandomState(seed)
    P = pinhole(h, w) + 0.02 * rs.randn(3, 4)
    d = 1.0 + 29.0 * rs.rand(N)
    d[rs.rand(N) < 0.05] *= -1
    u, v = (rs.rand(N) * (1 + 2 * margin) - margin) * w, (rs.rand(N) * (1 + 2 * margin) - margin) * h
    pc = np.zeros((C, N), np.float32)
    pc[:3] = np.linalg.solve(P[:, :3], np.stack([u * d, v * d, d]) - P[:, 3:]).astype(np.float32)
    if C > 3:
        pc[3:] = rs.rand(C - 3, N)
    return pc, P


def image(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def smooth_image(h, w, seed, cell=8):
    """grey (R = G = B, so L is the level itself): random levels on a coarse grid, interpolated bilinearly, stretched to 0 .. 255"""
    rs = np.random.RandomState(seed)
    gh, gw = h // cell + 2, w // cell + 2
    g = rs.rand(gh, gw)
    yy, xx = np.arange(h) / cell, np.arange(w) / cell
    y0, x0 = yy.astype(int), xx.astype(int)
    ty, tx = (yy - y0)[:, None], (xx - x0)[None, :]
    a = g[y0][:, x0] * (1 - ty) * (1 - tx) + g[y0][:, x0 + 1] * (1 - ty) * tx + g[y0 + 1][:, x0] * ty * (1 - tx) + g[y0 + 1][:, x0 + 1] * ty * tx
    a = (a - a.min()) / (a.max() - a.min())
    lev = np.minimum((a * 256).astype(np.int64), 255).astype(np.uint8)
    return np.repeat(lev[:, :, None], 3, 2)


PEAK = dict(h=48, w=64, N=3000, seed=7, bins=8)
SHIFTS = [(du, dv) for du in (-8, -4, 0, 4, 8) for dv in (-8, -4, 0, 4, 8) if (du, dv) != (0, 0)] + [(5, -6), (-7, 4), (12, 0), (0, -12)]


def peak_case():
    """-> pc (1,3,N), img uint8 (1,h,w,3), P (1,K,3,4) with candidate 0 the true pose and every other one shifted by at least 4 pixels
    (row 0 += du row 2, row 1 += dv row 2 moves every projection by exactly (du, dv)), value (1,N) float32 = the grey level under
    the true projection (0 where the point is not in frame), to be binned over (0, 256)"""
    h, w, N = PEAK['h'], PEAK['w'], PEAK['N']
    pc, P0 = cloud(N, h, w, PEAK['seed'], C=3, margin=0.0)
    pc[2] = np.abs(pc[2])                                        # in front of the camera
    img = smooth_image(h, w, PEAK['seed'] + 1)
    p = FC.project(pc, P0, h, w)
    value = np.where(p['frame'], SC.luma(img[p['r'], p['c']]), 0).astype(np.float32)
    P = [P0]
    for du, dv in SHIFTS:
        Q = P0.copy()
        Q[0] += du * P0[2]
        Q[1] += dv * P0[2]
        P.append(Q)
    return pc[None], img[None], np.stack(P)[None], value[None]


def test_total_and_marginals():
    h, w = 37, 53
    pc, P = cloud(2000, h, w, 1)
    img = image(h, w, 2)
    for bins in SC.BINS:
        hist = SC.hist1(pc, pc[3], P, img, bins, 0.0, 1.0)
        p = FC.project(pc, P, h, w)
        f = p['frame']
        assert 500 < f.sum() < 2000 and hist.sum() == f.sum()
        px = img[p['r'][f], p['c'][f]].astype(np.int64)
        # Pillow's ImageMath-free statement of L: the rounded weighted mean with the weights as 16-bit fractions
        L = (px @ np.array([19595, 38470, 7471]) + 32768) // 65536
        assert (hist.sum(0) == np.bincount(L * bins // 256, minlength=bins)).all()
        xb = np.minimum((pc[3][f].astype(np.float64) * bins).astype(np.int64), bins - 1)      # [0,1) times a power of two: exact in float32 too
        assert (hist.sum(1) == np.bincount(xb, minlength=bins)).all()
        e = SC.entropies(hist)
        assert e['count'] == f.sum() and e['mi'] >= 0 and abs(e['mi'] - (e['hx'] + e['hy'] - e['hxy'])) < 1e-12


def test_min_depth_follows_the_frame_mask():
    h, w = 20, 30
    pc, P = cloud(500, h, w, 3)
    img = image(h, w, 4)
    near = FC.project(pc, P, h, w, 10.0)['frame'].sum()
    assert 0 < near < FC.project(pc, P, h, w)['frame'].sum()
    assert SC.hist1(pc, pc[3], P, img, 16, 0.0, 1.0, min_depth=10.0).sum() == near


def test_permutation_of_the_points():
    h, w = 37, 53
    pc, P = cloud(1500, h, w, 5)
    img = image(h, w, 6)
    perm = np.random.RandomState(7).permutation(1500)
    a = SC.hist1(pc, pc[3], P, img, 32, 0.1, 0.9)
    b = SC.hist1(np.ascontiguousarray(pc[:, perm]), pc[3][perm], P, img, 32, 0.1, 0.9)
    assert (a == b).all() and a.sum() > 500


def test_value_bin_edges():
    lo, hi = np.float32(0.25), np.float32(2.5)
    below = np.nextafter(hi, np.float32(0))
    v = np.array([lo, hi, below, np.nan, np.inf, -np.inf, lo - 1, hi + 1, np.nextafter(lo, np.float32(9)), 3e38, -3e38], np.float32)
    for bins in SC.BINS:
        x, keep = SC.value_bin(v, lo, hi, bins)
        assert keep.tolist() == [True, True, True, False] + [True] * 7
        assert x[[0, 1, 2]].tolist() == [0, bins - 1, bins - 1]
        assert x[4:].tolist() == [bins - 1, 0, 0, bins - 1, 0, bins - 1, 0]
    # interior edges of an exactly representable grid: bin j starts AT lo + j (hi - lo) / bins
    x, _ = SC.value_bin(np.arange(0, 64, dtype=np.float32) / 64, 0.0, 1.0, 64)
    assert x.tolist() == list(range(64))
    x, _ = SC.value_bin(np.nextafter(np.arange(1, 8, dtype=np.float32) / 8, np.float32(0)), 0.0, 1.0, 8)
    assert x.tolist() == list(range(7))
    # a NaN value drops the point from the histogram, an infinite one stays
    img = np.full((1, 1, 3), 200, np.uint8)
    pc = np.array([[.5, .5, .5], [.5, .5, .5], [1., 1., 1.]], np.float32)
    T = np.array([[1., 0, 0, 0], [0, 1., 0, 0], [0, 0, 1., 0]])
    hist = SC.hist1(pc, np.array([np.nan, np.inf, -np.inf], np.float32), T, img, 8, 0.0, 1.0)
    assert hist.sum() == 2 and hist[7, 6] == 1 and hist[0, 6] == 1


def _strip(bins, per_cell, value_of):
    """a 1 x bins image whose pixel y has grey bin y, `per_cell(x, y)` points on pixel y with value bin x"""
    img = np.zeros((1, bins, 3), np.uint8)
    img[0, :, :] = (np.arange(bins) * (256 // bins))[:, None]
    T = np.array([[1., 0, 0, 0], [0, 1., 0, 0], [0, 0, 1., 0]])
    us, vs = [], []
    for x in range(bins):
        for y in range(bins):
            m = per_cell(x, y)
            us += [y + 0.5] * m
            vs += [value_of(x)] * m
    n = len(us)
    pc = np.stack([np.array(us), np.full(n, 0.5), np.ones(n)]).astype(np.float32)
    return pc, np.array(vs, np.float32), T, img


@pytest.mark.parametrize('bins', SC.BINS)
def test_bijective_pair_has_one_entropy(bins):
    sigma = np.random.RandomState(bins).permutation(bins)          # value bin x <-> grey bin sigma[x], 3 + x points each
    pc, v, T, img = _strip(bins, lambda x, y: (3 + x) if sigma[x] == y else 0, lambda x: (x + 0.5) / bins)
    hist = SC.hist1(pc, v, T, img, bins, 0.0, 1.0)
    assert (hist[np.arange(bins), sigma] == 3 + np.arange(bins)).all() and hist.sum() == (3 + np.arange(bins)).sum()
    e = SC.entropies(hist)
    for k in ('hx', 'hy', 'hxy'):
        assert abs(e[k] - e['mi']) < 1e-13 * max(1.0, e['mi']), k
    assert e['mi'] > 1.0 and abs(e['nmi'] - 2.0) < 1e-13


@pytest.mark.parametrize('bins', SC.BINS)
def test_independent_pair_has_no_information(bins):
    pc, v, T, img = _strip(bins, lambda x, y: 5, lambda x: (x + 0.5) / bins)
    hist = SC.hist1(pc, v, T, img, bins, 0.0, 1.0)
    assert (hist == 5).all()
    e = SC.entropies(hist)
    assert abs(e['mi']) < 1e-13 and abs(e['hx'] - math.log(bins)) < 1e-13 and abs(e['hxy'] - 2 * math.log(bins)) < 1e-13
    assert abs(e['nmi'] - 1.0) < 1e-13


def test_empty_and_one_cell():
    z = SC.entropies(np.zeros((8, 8), np.int64))
    assert [z[k] for k in ('mi', 'nmi', 'hx', 'hy', 'hxy', 'count')] == [0.0] * 5 + [0]
    h = np.zeros((8, 8), np.int64)
    h[3, 5] = 63                                                   # 63 log 63 / 63 need not round to log 63: defined as 0
    e = SC.entropies(h)
    assert [e[k] for k in ('mi', 'nmi', 'hx', 'hy', 'hxy', 'count')] == [0.0] * 5 + [63]
    h[3, 6] = 1                                                    # one row, two columns: Hx = 0 exactly, Hy = Hxy > 0
    e = SC.entropies(h)
    assert e['hx'] == 0.0 and e['hy'] == e['hxy'] > 0 and abs(e['mi']) < 1e-15 and abs(e['nmi'] - 1.0) < 1e-13


def test_peak_property():
    """the true pose scores strictly higher than every candidate at least 4 pixels off, on the contract alone"""
    pc, img, P, value = peak_case()
    ref = SC.score(pc, img, P, value, 0.0, 256.0, PEAK['bins'])
    mi, cnt = ref['mi'][0], ref['count'][0]
    assert cnt[0] > 2000 and cnt[1:].min() > 1000
    assert (mi[0] > mi[1:]).all() and mi[0] > 1.5 * mi[1:].max(), mi
    assert (ref['nmi'][0, 0] > ref['nmi'][0, 1:]).all()
    assert int(np.argmax(mi)) == 0


def _tree(t):
    t = list(t)
    s = len(t) // 2
    while s:
        t = [t[i] + t[i + s] for i in range(s)]
        s //= 2
    return t[0]


def test_bounds_hold_a_numpy_model_of_the_kernels_arithmetic():
    """the kernel's order of operations with numpy's log in place of the device's: inside the bound, with room to spare"""
    rs = np.random.RandomState(11)
    for bins in SC.BINS:
        for scale in (3, 200, 100000):
            h = (rs.rand(bins, bins) ** 6 * scale).astype(np.int64)
            e, n = SC.entropies(h), int(h.sum())
            bd = SC.bounds(e, bins)
            term = lambda c: [float(v) * math.log(v) if v else 0.0 for v in c]
            H = lambda c: math.log(n) - _tree(term(c)) / n
            hx, hy, hxy = H(h.sum(1)), H(h.sum(0)), H(h.reshape(-1))
            got = dict(hx=hx, hy=hy, hxy=hxy, mi=(hx + hy) - hxy, nmi=(hx + hy) / hxy)
            for k, v in got.items():
                assert abs(v - e[k]) <= bd[k], (bins, scale, k, v - e[k], bd[k])
                assert bd[k] < 1e-11 * max(1.0, abs(e[k])), (bins, scale, k, bd[k])         # and the bound is no licence


def test_candidates_around():
    import torch
    from efgh_amd import _C
    from efgh_amd.common.score import perturbations
    P = torch.randn(2, 3, 4, dtype=torch.float64)
    for rot, tr, steps, K in (((0.5, 0.5, 0.5), (0.1, 0.1, 0.1), 1, 729), ((1.0, 0, 0), (0, 0, 0), 3, 7), ((0, 0, 0), (0, 0, 0), 1, 1),
                              ((0, 2.0, 0), (0.5, 0, 0.25), 2, 125), ((1, 1, 1), (1, 1, 1), 1, 729)):
        D = perturbations(rot, tr, steps)
        assert D.dtype == torch.float64 and tuple(D.shape) == (K, 4, 4)
        R, t = D[:, :3, :3], D[:, :3, 3]
        assert (R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-15
        assert (torch.linalg.det(R) - 1).abs().max() <= 1e-15 and torch.equal(D[:, 3], torch.tensor([0., 0, 0, 1], dtype=torch.float64).expand(K, 4))
        assert torch.equal(D[0], torch.eye(4, dtype=torch.float64))
        assert len({tuple(d.reshape(-1).tolist()) for d in D}) == K                          # all different
        assert t.abs().max() <= steps * max(map(abs, tr)) and (K == 1 or (D[1:] - D[0]).abs().amax((1, 2)).min() > 0)
        for Pin in (P, P.float()):
            C = candidates_around(Pin, rot, tr, steps)
            assert C.dtype == torch.float64 and tuple(C.shape) == (2, K, 3, 4)
            assert torch.equal(C[:, 0], Pin.double())                                        # bit for bit
            assert torch.allclose(C, torch.einsum('bij,kjl->bkil', Pin.double(), D), rtol=0, atol=1e-14 * float(Pin.abs().max()) * 4)
    # steps = 2 on six axes: 5^6 = 15625 candidates
    with pytest.raises(_C.EfghError, match='15625 candidates, at most 4096'):
        candidates_around(P, (1, 1, 1), (1, 1, 1), steps=2)
    assert candidates_around(P, (1, 1, 1), (1, 1, 0), steps=np.int64(2)).shape[1] == 3125       # a numpy integer is an integer
    for bad in (dict(rot_deg=(1, 1)), dict(trans=(1, float('nan'), 0)), dict(steps=0), dict(steps=1.5), dict(P=P[0]), dict(P=P.long())):
        a = dict(P=P, rot_deg=(1, 1, 1), trans=(0, 0, 0), steps=1)
        a.update(bad)
        with pytest.raises(_C.EfghError, match='candidates_around'):
            candidates_around(**a)


def test_score_is_exported_and_checks_its_arguments_before_any_launch():
    import torch
    from efgh_amd import _C
    assert Score.__slots__ == ('mi', 'nmi', 'hx', 'hy', 'hxy', 'count', 'hist')
    pc, img = torch.zeros(2, 4, 5), torch.zeros(2, 4, 6, 3, dtype=torch.uint8)
    T, val = torch.zeros(2, 3, 3, 4, dtype=torch.float64), torch.zeros(2, 5)
    bad = [
        ('pc', dict(pc=pc.half())), ('pc', dict(pc=pc[:, :2])), ('pc', dict(pc=pc[0])),
        ('cam_T_velo', dict(T=torch.zeros(2, 3, 3))), ('cam_T_velo', dict(T=T.half())), ('cam_T_velo', dict(T={'cam_T_velo': T})),
        ('cam_T_velo', dict(T=T[:1])), ('cam_T_velo', dict(T=torch.zeros(2, 4097, 3, 4))), ('cam_T_velo', dict(T=T[:, :0])),
        ('img', dict(img=img[:1])), ('img', dict(img=torch.zeros(2, 4, 6, 3))), ('img', dict(img=img.int())),
        ('value', dict(pc=pc[:, :3])),                           # None takes pc[:, 3]: there is none
        ('value', dict(value=val.double())), ('value', dict(value=val[:, :4])), ('value', dict(value=[0.0] * 5)),
        ('value_range', dict(value=val, value_range=(1.0, 1.0))), ('value_range', dict(value_range=(0.0, float('inf')))),
        ('value_range', dict(value_range=3.0)), ('value_range', dict(value_range=(0.0, float('nan')))),
        ('bins', dict(bins=256)), ('bins', dict(bins=12)), ('bins', dict(bins=32.0)), ('bins', dict(bins=0)),
        ('min_depth', dict(min_depth=-1.0)), ('min_depth', dict(min_depth=float('nan'))),
        ('pc', {}),                                              # everything valid but on the CPU: there is no CPU path
    ]
    for name, kw in bad:
        a = dict(pc=pc, img=img, T=T)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        with pytest.raises(_C.EfghError, match=r'score: %s\b' % name):
            score(a['pc'], a['img'], a['T'], **kw)
    with pytest.raises(_C.EfghError, match='bins: 256'):         # the refusal names the value
        score(pc, img, T, bins=256)
    # the accepted forms reach the device check, which is the last one
    for t, im, v in ((T, img, None), (T[:, 0], torch.zeros(2, 3, 4, 6), val), (T.float(), img, val.to(torch.uint8))):
        with pytest.raises(_C.EfghError, match='CPU tensor'):
            score(pc, im, t, value=v)
    with pytest.raises(_C.EfghError, match=r"Score.best: by = 'count'"):
        Score(mi=torch.zeros(1, 2)).best('count')
    assert Score(mi=torch.tensor([[0., 2., 1.]], dtype=torch.float64)).best().tolist() == [1]
    # stage_poses: the order, the names, the missing stage
    pred = {k: torch.full((2, 3, 4), float(i)) for i, k in enumerate(('eh_cam_T_velo', 'efh_cam_T_velo', 'efgh_cam_T_velo'), 1)}
    pred['cam_T_velo'] = pred['efgh_cam_T_velo']
    poses, names = stage_poses(pred)
    assert names == ('eh_cam_T_velo', 'efh_cam_T_velo', 'efgh_cam_T_velo') and tuple(poses.shape) == (2, 3, 3, 4)
    assert poses[:, :, 0, 0].tolist() == [[1., 2., 3.]] * 2
    poses, names = stage_poses(pred, torch.zeros(2, 3, 4, dtype=torch.float64))
    assert names[0] == 'calib' and poses.dtype == torch.float64 and poses[:, :, 0, 0].tolist() == [[0., 1., 2., 3.]] * 2
    for p, c in (({'efgh_cam_T_velo': pred['efgh_cam_T_velo']}, None), (pred, torch.zeros(3, 4)), ([], None)):
        with pytest.raises(_C.EfghError, match='stage_poses'):
            stage_poses(p, c)
