"""tests/score_soft_contract.py held to properties that are not taken from it (no GPU): totals and the value marginal against
score_contract's hard histogram, permutation invariance, a constant image, the analytic gradient against central differences of the
unquantised MI, directed edge cases of the grey cell and of the clipped neighbours; `refine` run on the contract through its `scorer`
argument; the argument refusals of `score_soft` and `refine`, which need no device."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_contract as FC  # noqa: E402
import score_contract as SC  # noqa: E402
import score_soft_contract as SS  # noqa: E402
from test_score_host import PEAK, cloud, image, peak_case  # noqa: E402
from efgh_amd.common import Refined, Score, refine, score_soft  # noqa: E402  (the feature under test: no CPU path, but it imports and checks)

FRAC = SS.FRAC
# the two starts of the refinement tests: three Euler angles (rad) and a translation (m) of the LiDAR frame applied to the true pose
STARTS = ([0.05, -0.04, 0.06, 0.2, -0.15, 0.1], [-0.08, 0.06, 0.05, -0.3, 0.2, 0.2])


def shifted(P0, du, dv):
    Q = P0.copy()
    Q[0] += du * P0[2]
    Q[1] += dv * P0[2]
    return Q


def test_total_and_value_marginal_against_the_hard_histogram():
    h, w = 37, 53
    pc, P = cloud(2000, h, w, 1)
    img = image(h, w, 2)
    for bins in SC.BINS:
        hard = SC.hist1(pc, pc[3], P, img, bins, 0.0, 1.0)
        soft = SS.hist1(pc, pc[3], P, img, bins, 0.0, 1.0)
        assert soft.dtype == np.int64 and (soft >= 0).all() and hard.sum() > 500
        assert soft.sum() == FRAC * hard.sum()
        assert (soft.sum(1) == FRAC * hard.sum(1)).all()           # the value bin is the hard one; only the grey axis is spread
        ref = SS.score_soft(pc[None], img[None], P[None, None], pc[None, 3], 0.0, 1.0, bins, want_grad=False)
        assert ref['count'].tolist() == [[hard.sum()]] and ref['hist'].dtype == np.int32
        # the unquantised histogram: one a point, the same marginal
        fl = SS.hist1(pc, pc[3], P, img, bins, 0.0, 1.0, frac=None)
        assert abs(fl.sum() - hard.sum()) < 1e-9 * hard.sum() and np.abs(fl.sum(1) - hard.sum(1)).max() < 1e-9 * hard.sum()
        assert np.abs(fl * FRAC - soft).max() <= 0.5 * hard.sum()         # a point's weight is rounded by at most half a unit a cell
    assert SS.hist1(pc, pc[3], P, img, 16, 0.0, 1.0, min_depth=10.0).sum() == FRAC * FC.project(pc, P, h, w, 10.0)['frame'].sum()


def test_permutation_of_the_points():
    h, w = 37, 53
    pc, P = cloud(1500, h, w, 5)
    img = image(h, w, 6)
    perm = np.random.RandomState(7).permutation(1500)
    a = SS.hist1(pc, pc[3], P, img, 32, 0.1, 0.9)
    b = SS.hist1(np.ascontiguousarray(pc[:, perm]), pc[3][perm], P, img, 32, 0.1, 0.9)
    assert (a == b).all() and a.sum() > 500 * FRAC
    ra = SS.score_soft(pc[None], img[None], P[None, None], pc[None, 3], 0.1, 0.9, 32)
    rb = SS.score_soft(np.ascontiguousarray(pc[:, perm])[None], img[None], P[None, None], pc[3][perm][None], 0.1, 0.9, 32)
    assert np.abs(ra['grad']).max() > 0 and (ra['grad'] == rb['grad']).all()      # (math.fsum: the exact sum, rounded once)


def test_constant_image_has_no_gradient():
    h, w = 20, 30
    pc, P = cloud(800, h, w, 9)
    for level in (0, 100, 255):
        img = np.full((h, w, 3), level, np.uint8)
        ref = SS.score_soft(pc[None], img[None], P[None, None], pc[None, 3], 0.0, 1.0, 16)
        assert ref['count'][0, 0] > 200 and (ref['grad'] == 0).all() and (ref['grad_bound'] == 0).all()
        assert abs(ref['mi'][0, 0]) <= 1e-12 + (0 if level in (0, 255) else math.log(2))
        mi, G = SS.grad_float(pc, pc[3], P, img, 16, 0.0, 1.0)
        assert (G == 0).all()


@pytest.mark.parametrize('bins', [8, 32])
def test_gradient_against_central_differences(bins):
    """all 12 entries of dMI/dP of the unquantised function, on the peak scene with the pose 2.3 px right and 1.7 px up of the truth"""
    pc, img, P, value = peak_case()
    pc, img, value = pc[0], img[0], value[0]
    Q = shifted(P[0, 0], 2.3, -1.7)
    mi, G = SS.grad_float(pc, value, Q, img, bins, 0.0, 256.0)
    eps = 1e-6
    FD = np.zeros((3, 4))
    for i in range(3):
        for c in range(4):
            E = np.zeros((3, 4))
            E[i, c] = eps
            up = SS.mi_float(SS.hist1(pc, value, Q + E, img, bins, 0.0, 256.0, frac=None))
            dn = SS.mi_float(SS.hist1(pc, value, Q - E, img, bins, 0.0, 256.0, frac=None))
            FD[i, c] = (up - dn) / (2 * eps)
    err = np.abs(G - FD).max() / np.abs(G).max()
    print('bins %d: mi %.4f, max|G| %.3e, max|G - FD| / max|G| %.2e' % (bins, mi, np.abs(G).max(), err))
    assert np.abs(G).max() > 1e-3 and (G != 0).all()
    assert err <= 1e-5
    # and the quantised histogram's gradient is that of a neighbour of the function: the same to a few per cent
    q = SS.score_soft(pc[None], img[None], Q[None, None], value[None], 0.0, 256.0, bins)
    assert np.abs(q['grad'][0, 0] - G).max() <= 0.05 * np.abs(G).max()


def edge_case(bins=8):
    """a 6 x 8 grey image and points under the pinhole-free matrix u = x / z, v = y / z with z = 1: pixel centres (tx = ty = 0) on
    L = 48 (t - j exactly 0 at bins 8), 240 (exactly 1 in the clipped top cell), 0 and 255; points in the half-pixel rim on all four
    borders and in two corners, where neighbours are clipped; 300 ordinary points -> pc (1,3,N), img (1,6,8,3), P (1,1,3,4), value (1,N)"""
    h, w = 6, 8
    rs = np.random.RandomState(31)
    lev = rs.randint(0, 256, (h, w))
    lev[3, 2], lev[1, 5], lev[4, 4], lev[2, 6] = 48, 240, 0, 255
    img = np.repeat(lev[:, :, None], 3, 2).astype(np.uint8)
    fixed = [(2.5, 3.5), (5.5, 1.5), (4.5, 4.5), (6.5, 2.5),                                   # centres: u = c + 0.5, v = r + 0.5
             (0.25, 2.7), (7.75, 2.2), (3.3, 0.2), (4.6, 5.9), (0.1, 0.1), (7.9, 5.95), (0.0, 0.0), (0.5, 0.5)]
    uv = np.array(fixed + [(rs.rand() * w, rs.rand() * h) for _ in range(300)])
    pc = np.stack([uv[:, 0], uv[:, 1], np.ones(len(uv))]).astype(np.float32)
    value = rs.rand(len(uv)).astype(np.float32)
    value[:12] = 0.3
    P = np.array([[1., 0, 0, 0], [0, 1., 0, 0], [0, 0, 1., 0]])
    return pc[None], img[None], P[None, None], value[None]


def test_directed_edge_cases():
    pc, img, P, value = edge_case()
    pt = SS.points1(pc[0], value[0], P[0, 0], img[0], 8, 0.0, 1.0)
    assert pt['idx'][:12].tolist() == list(range(12))                # every directed point is in frame
    lev = img[0, :, :, 0].astype(np.int64)
    # u, v exactly on a pixel centre: the sample is the pixel, the slopes are the forward differences
    for i, (r, c) in enumerate(((3, 2), (1, 5), (4, 4), (2, 6))):
        assert pt['gu'][i] == lev[r, c + 1] - lev[r, c] and pt['gv'][i] == lev[r + 1, c] - lev[r, c]
    # L = 48: t = 1 exactly, all of the weight on cell 1, gate shut; L = 240: t = 7, j clipped to 6, all on cell 7, gate shut
    assert (pt['j'][0], pt['q'][0], pt['fr'][0], bool(pt['s'][0])) == (1, 0, 0.0, False)
    assert (pt['j'][1], pt['q'][1], pt['fr'][1], bool(pt['s'][1])) == (6, FRAC, 1.0, False)
    # L = 0: t = -0.5 clamps to the bottom cell; L = 255: beyond the top cell's centre, clamps to it
    assert (pt['j'][2], pt['q'][2], bool(pt['s'][2])) == (0, 0, False)
    assert (pt['j'][3], pt['q'][3], bool(pt['s'][3])) == (6, FRAC, False)
    # the half-pixel rim: both neighbours across the border are the border pixel, the slope across it is 0
    assert pt['gu'][4] == 0 and pt['gu'][5] == 0 and pt['gv'][4] != 0 and pt['gv'][5] != 0
    assert pt['gv'][6] == 0 and pt['gv'][7] == 0 and pt['gu'][6] != 0 and pt['gu'][7] != 0
    for i, (r, c) in ((8, (0, 0)), (9, (5, 7)), (10, (0, 0))):
        assert pt['gu'][i] == 0 and pt['gv'][i] == 0
        t = lev[r, c] * (8 / 256.0) - 0.5
        assert pt['j'][i] == min(max(math.floor(t), 0), 6)
    for bins in (8, 64):
        ref = SS.score_soft(pc, img, P, value, 0.0, 1.0, bins)
        assert ref['count'][0, 0] == pc.shape[2] and np.isfinite(ref['grad']).all() and np.abs(ref['grad']).max() > 0
        h = ref['hist'][0, 0]
        assert h.sum() == FRAC * pc.shape[2] and (h.sum(1) == FRAC * np.bincount(SC.value_bin(value[0], 0.0, 1.0, bins)[0], minlength=bins)).all()


def reprojection_offset(pc, P, P0, h, w):
    """mean distance in pixels between the projections under P and under P0, over the points in frame under P0"""
    a, b = FC.project(pc, P, h, w), FC.project(pc, P0, h, w)
    m = b['frame']
    return float(np.hypot(a['u'][m] - b['u'][m], a['v'][m] - b['v'][m]).mean())


def start_pose(P0, z):
    from efgh_amd.common.score import _rigid
    z = torch.tensor(z, dtype=torch.float64)[None]
    return (torch.from_numpy(P0) @ _rigid(z[:, :3], z[:, 3:])[0]).numpy()


def contract_scorer(pc, img, P, value=None, value_range=(0.0, 1.0), bins=32, pool=False):
    """`score_soft` on the numpy contract, for CPU tensors: mi carries the contract's gradient to P"""
    lo, hi = value_range
    args = pc.numpy(), img.numpy(), value.numpy()

    class F(torch.autograd.Function):
        @staticmethod
        def forward(ctx, P):
            ref = SS.score_soft(args[0], args[1], P.detach().numpy()[:, None], args[2], lo, hi, bins, pool=pool)
            ctx.G, ctx.pool = torch.from_numpy(ref['grad'][:, 0]), pool
            return torch.from_numpy(np.ascontiguousarray(ref['mi'].reshape(-1)))

        @staticmethod
        def backward(ctx, g):
            return ctx.G * (g[0] if ctx.pool else g[:, None, None])
    return Score(mi=F.apply(P))


@pytest.mark.parametrize('bins', [8, 32])
@pytest.mark.parametrize('start', [0, 1])
def test_refine_on_the_contract(start, bins):
    pc, img, P, value = peak_case()
    P0 = P[0, 0]
    Pst = start_pose(P0, STARTS[start])
    before = reprojection_offset(pc[0], Pst, P0, PEAK['h'], PEAK['w'])
    r = refine(torch.from_numpy(pc), torch.from_numpy(img), torch.from_numpy(Pst)[None], value=torch.from_numpy(value), value_range=(0.0, 256.0),
               bins=bins, iters=200, rot_step_deg=0.2, trans_step=0.02, scorer=contract_scorer)
    assert isinstance(r, Refined) and r.pose.dtype == torch.float64 and tuple(r.pose.shape) == (1, 3, 4) and tuple(r.trace.shape) == (200, 1)
    after = reprojection_offset(pc[0], r.pose[0].numpy(), P0, PEAK['h'], PEAK['w'])
    print('start %d bins %d: offset %.2f px -> %.3f px, mi %.4f -> %.4f at iterate %d'
          % (start, bins, before, after, float(r.start_mi), float(r.mi), int(r.best_iter)))
    assert 3.0 < before < 6.0
    assert float(r.mi) > float(r.start_mi) and float(r.mi) == float(r.trace.max()) and int(r.best_iter) == int(r.trace[:, 0].argmax())
    assert float(r.start_mi) == float(r.trace[0, 0])
    assert after <= 0.5


def test_refine_iterate_zero_is_the_start_and_frozen_axes_stay():
    pc, img, P, value = peak_case()
    Pst = start_pose(P[0, 0], STARTS[0])
    t = torch.from_numpy(pc), torch.from_numpy(img), torch.from_numpy(Pst)[None]
    kw = dict(value=torch.from_numpy(value), value_range=(0.0, 256.0), bins=8, scorer=contract_scorer)
    r = refine(*t, iters=1, **kw)
    assert torch.equal(r.pose, t[2]) and r.best_iter.tolist() == [0] and torch.equal(r.mi, r.start_mi)
    # only the translation along x is free: P = P0 D with D the identity but for its entry (0, 3).  On a scorer that is linear in
    # P every step climbs, so the last iterate is the best one
    linear = lambda pc, img, P, **kw: Score(mi=(P * torch.arange(1., 13., dtype=torch.float64).reshape(3, 4)).sum((1, 2)))
    r = refine(*t, iters=5, dof=(0, 0, 0, 1, 0, 0), scorer=linear)
    assert r.best_iter.tolist() == [4] and (r.trace[1:] > r.trace[:-1]).all()
    got = r.pose[0].numpy()
    d, c = got[:, 3] - Pst[:, 3], Pst[:, 0]
    along = float(d @ c / (c @ c))
    assert (got[:, :3] == Pst[:, :3]).all() and along != 0 and np.abs(d - along * c).max() < 1e-12 * np.abs(Pst).max()
    # float32 start, pooled: one parameter set for the batch
    two = torch.from_numpy(np.concatenate([pc, pc])), torch.from_numpy(np.concatenate([img, img])), torch.from_numpy(np.stack([Pst, Pst])).float()
    kw['value'] = torch.from_numpy(np.concatenate([value, value]))
    r = refine(*two, iters=3, pool=True, **kw)
    assert tuple(r.pose.shape) == (2, 3, 4) and tuple(r.mi.shape) == (1,) and tuple(r.trace.shape) == (3, 1) and torch.equal(r.pose[0], r.pose[1])


def test_arguments_are_checked_before_any_launch():
    from efgh_amd import _C
    pc, img = torch.zeros(2, 4, 5), torch.zeros(2, 4, 6, 3, dtype=torch.uint8)
    T, val = torch.zeros(2, 3, 3, 4, dtype=torch.float64), torch.zeros(2, 5)
    bad = [
        ('pc', dict(pc=pc.half())), ('pc', dict(pc=pc[:, :2])), ('cam_T_velo', dict(T=torch.zeros(2, 3, 3))), ('cam_T_velo', dict(T=T.half())),
        ('cam_T_velo', dict(T=torch.zeros(2, 4097, 3, 4))), ('img', dict(img=img[:1])), ('value', dict(pc=pc[:, :3])),
        ('value', dict(value=val.double())), ('value_range', dict(value=val, value_range=(1.0, 1.0))), ('bins', dict(bins=256)),
        ('bins', dict(bins=12)), ('min_depth', dict(min_depth=-1.0)), ('pool', dict(pool=1)), ('pool', dict(pool=None)),
        ('pc', {}),                                              # everything valid but on the CPU: there is no CPU path
    ]
    for name, kw in bad:
        a = dict(pc=pc, img=img, T=T)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        with pytest.raises(_C.EfghError, match=r'score_soft: %s\b' % name):
            score_soft(a['pc'], a['img'], a['T'], **kw)
    with pytest.raises(_C.EfghError, match='CPU tensor'):
        score_soft(pc, img, T.float().requires_grad_(), value=val.to(torch.uint8), pool=True)
    P0 = torch.zeros(2, 3, 4)
    for name, kw in (('P0', dict(P0=P0[0])), ('P0', dict(P0=P0.long())), ('P0', dict(P0=None)), ('iters', dict(iters=0)), ('iters', dict(iters=2.5)),
                     ('rot_step_deg', dict(rot_step_deg=0.0)), ('rot_step_deg', dict(trans_step=float('nan'))), ('rot_step_deg', dict(dof=(1, 1, 1))),
                     ('pool', dict(pool=1)), ('scorer', dict(scorer=None))):
        a = dict(P0=P0)
        a.update(kw)
        with pytest.raises(_C.EfghError, match=r'refine: %s\b' % name):
            refine(pc, img, **a)
    with pytest.raises(_C.EfghError, match=r'score_soft: pc: a CPU tensor'):      # the default scorer checks the rest, in front of any launch
        refine(pc, img, P0)
    assert Refined.__slots__ == ('pose', 'mi', 'start_mi', 'trace', 'best_iter')
