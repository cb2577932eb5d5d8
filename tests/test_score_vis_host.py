"""tests/score_vis_contract.py held to properties that are not taken from it (no GPU): a tolerance that hides nothing gives the frame
mask and score_contract's histogram, cell 1 is fuse_contract's z-buffer and resolve at radius 0, one cell over the image keeps exactly
the nearest points, the mask is a subset of the frame and grows with either tolerance, permutation invariance, occupancy against
np.count_nonzero, the Miller-Madow identity of a full histogram, and a parallax scene in which the mask hides the wall points behind a
plate and raises the score at the true pose; the header, the binding, the pinned __slots__ and the argument refusals of the new
functions, which need no device."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_contract as FC  # noqa: E402
import score_contract as SC  # noqa: E402
import score_soft_contract as SS  # noqa: E402
import score_vis_contract as SV  # noqa: E402
from test_score_host import cloud, image  # noqa: E402
from efgh_amd.common import (Fused, Occlusion, Refined, Score, Visibility, VisibleScore, miller_madow, occupancy, refine,  # noqa: E402
                             score_soft_visible, score_visible, visible_mask)

CELLS = (1, 8, (6, 2), 64)
TOLS = ((0.0, 0.0), (0.25, 0.0), (0.0, 0.5))


def test_a_tolerance_that_hides_nothing_gives_the_frame_and_the_plain_histogram():
    h, w = 37, 53
    pc, P = cloud(2000, h, w, 1)
    img = image(h, w, 2)
    frame = FC.project(pc, P, h, w)['frame']
    for cell in CELLS:
        vis, z = SV.visible1(pc, P, h, w, cell, abs_tol=1e30)
        assert (vis == frame).all() and 500 < frame.sum() < 2000
        ref = SV.score_visible(pc[None], img[None], P[None, None], pc[None, 3], 0.0, 1.0, 16, cell, abs_tol=1e30)
        plain = SC.score(pc[None], img[None], P[None, None], pc[None, 3], 0.0, 1.0, 16)
        assert (ref['hist'] == plain['hist']).all() and (ref['count'] == plain['count']).all() and ref['mi'][0, 0] == plain['mi'][0, 0]
        soft = SV.score_soft_visible(pc[None], img[None], P[None, None], pc[None, 3], 0.0, 1.0, 16, cell, abs_tol=1e30)
        plain = SS.score_soft(pc[None], img[None], P[None, None], pc[None, 3], 0.0, 1.0, 16)
        assert (soft['hist'] == plain['hist']).all() and (soft['grad'] == plain['grad']).all() and np.abs(plain['grad']).max() > 0


@pytest.mark.parametrize('tol', TOLS)
def test_cell_one_is_fuse_at_radius_zero(tol):
    h, w = 12, 17                                                 # few pixels: most of them hold several points
    pc, P = cloud(1500, h, w, 3)
    pc[2, 100:200] = pc[2, 300:400]                               # some equal float32 depths as well
    img = image(h, w, 4)
    zb = FC.zbuffer(pc, P, h, w, 0)
    state, _, _ = FC.resolve(pc, P, img, zb, True, 0.0, tol[0], tol[1])
    vis, z = SV.visible1(pc, P, h, w, 1, tol[0], tol[1])
    assert (vis == (state == FC.VISIBLE)).all()
    assert 0 < vis.sum() < (state >= FC.OCCLUDED).sum()             # something is hidden, something is not
    empty = zb == FC.EMPTY
    assert (np.isinf(z) == empty).all() and not empty.all()
    depth = (zb >> np.uint64(32)).astype(np.uint32).view(np.float32)
    assert (z[~empty].view(np.uint32) == depth[~empty].view(np.uint32)).all()


def test_one_cell_over_the_image_keeps_exactly_the_nearest_points():
    h, w = 37, 53
    pc, P = cloud(800, h, w, 5)
    p = FC.project(pc, P, h, w)
    f = np.nonzero(p['frame'])[0]
    near = f[np.argmin(p['d'][f])]
    pc[:, f[:5]] = pc[:, [near]]                                  # five more points with the same coordinates: the same depth bits
    p = FC.project(pc, P, h, w)
    vis, z = SV.visible1(pc, P, h, w, 64)
    assert z.shape == (1, 1) and z[0, 0] == p['d'][p['frame']].min()
    want = p['frame'] & (p['d'] == z[0, 0])
    assert (vis == want).all() and vis.sum() >= 6


def test_subset_of_the_frame_and_monotone_in_both_tolerances():
    h, w = 48, 64
    pc, P = cloud(3000, h, w, 7)
    frame = FC.project(pc, P, h, w)['frame']
    for cell in CELLS:
        for which in (0, 1):
            last = None
            for t in (0.0, 0.05, 0.25, 1.0, 10.0, 1e30):
                vis, _ = SV.visible1(pc, P, h, w, cell, *((t, 0.0) if which == 0 else (0.0, t)))
                assert not (vis & ~frame).any()
                assert last is None or not (last & ~vis).any()
                last = vis
            assert (last == frame).all()                          # 1e30 of either kind admits every point in frame
        zero, _ = SV.visible1(pc, P, h, w, cell)
        if cell != 1:
            assert 0 < zero.sum() < frame.sum()
    # min_depth moves the frame, and the mask with it
    vis, _ = SV.visible1(pc, P, h, w, 8, min_depth=10.0)
    assert vis.any() and not (vis & ~FC.project(pc, P, h, w, 10.0)['frame']).any()


def test_permutation_of_the_points():
    h, w = 37, 53
    pc, P = cloud(1500, h, w, 9)
    img = image(h, w, 10)
    perm = np.random.RandomState(11).permutation(1500)
    pcp = np.ascontiguousarray(pc[:, perm])
    for cell in ((6, 2), 8):
        a = SV.score_visible(pc[None], img[None], P[None, None], pc[None, 3], 0.1, 0.9, 32, cell, 0.5, 0.1)
        b = SV.score_visible(pcp[None], img[None], P[None, None], pcp[None, 3], 0.1, 0.9, 32, cell, 0.5, 0.1)
        assert (a['zmin'].view(np.uint32) == b['zmin'].view(np.uint32)).all() and (a['vis'][0, 0][perm] == b['vis'][0, 0]).all()
        assert (a['hist'] == b['hist']).all() and np.isfinite(a['zmin']).sum() <= a['count'][0, 0] < a['frame'].sum()      # a cell's nearest point is visible
        assert (SV.pack(a['vis'][0, 0][perm]) == b['mask'][0, 0]).all()


def test_packed_words():
    rs = np.random.RandomState(12)
    for n in (1, 31, 32, 33, 64, 100):
        vis = rs.rand(2, 3, n) < 0.5
        words = SV.pack(vis)
        assert words.dtype == np.int32 and words.shape == (2, 3, -(-n // 32))
        for i in range(n):
            assert (((words[..., i // 32].view(np.uint32) >> np.uint32(i % 32)) & 1) == vis[..., i]).all()
        assert sum(bin(int(x)).count('1') for x in words.view(np.uint32).reshape(-1)) == vis.sum()       # nothing past N
        # the package unpacks them the same way (torch ops, CPU here)
        v = Visibility(torch.from_numpy(words), None, n)
        assert (v.unpack().numpy() == vis).all() and (v.count().numpy() == vis.sum(-1)).all() and v.count().dtype == torch.int32


def test_occupancy_and_the_miller_madow_identity():
    rs = np.random.RandomState(13)
    for bins in SC.BINS:
        h = (rs.rand(bins, bins) ** 8 * 50).astype(np.int64)
        h[3] = 0
        h[:, 5] = 0
        rx, ry, rxy = SV.occupancy(h)
        assert rx == np.count_nonzero(h.any(1)) and ry == np.count_nonzero(h.any(0)) and rxy == np.count_nonzero(h)
        assert rx < bins and ry < bins and 0 < rxy < rx * ry
        e = SC.entropies(h)
        mm, corr = SV.mi_mm(e['mi'], e['count'], (rx, ry, rxy))
        assert corr == (rxy - rx - ry + 1) / (2.0 * e['count']) and mm == e['mi'] - corr
        full = h + 1
        n = int(full.sum())
        mm, corr = SV.mi_mm(0.25, n, SV.occupancy(full))
        assert SV.occupancy(full) == (bins, bins, bins * bins) and corr == (bins - 1) ** 2 / (2.0 * n)
    assert SV.mi_mm(0.0, 0, (0, 0, 0)) == (0.0, 0.0) and SV.occupancy(np.zeros((8, 8), np.int64)) == (0, 0, 0)
    # a bijective pair: Rxy = Rx = Ry = bins, the term is (1 - bins) / (2 n) - the plug-in estimate of a diagonal is biased DOWNWARDS
    d = np.diag(np.arange(1, 9))
    assert SV.mi_mm(1.0, 36, SV.occupancy(d))[1] == -7 / 72.0


def test_a_nan_value_leaves_the_soft_gradient_as_it_leaves_the_histogram():
    h, w = 37, 53
    pc, P = cloud(1500, h, w, 14)
    img = image(h, w, 15)
    drop = np.random.RandomState(16).rand(1500) < 0.4
    value = np.where(drop, np.float32(np.nan), pc[3]).astype(np.float32)
    pt = SS.points1(pc, value, P, img, 16, 0.0, 1.0)
    assert not drop[pt['idx']].any() and pt['idx'].shape[0] == (FC.project(pc, P, h, w)['frame'] & ~drop).sum()
    sub = np.ascontiguousarray(pc[:, ~drop])
    a = SS.score_soft(pc[None], img[None], P[None, None], value[None], 0.0, 1.0, 16)
    b = SS.score_soft(sub[None], img[None], P[None, None], sub[None, 3], 0.0, 1.0, 16)
    assert (a['hist'] == b['hist']).all() and (a['grad'] == b['grad']).all() and np.abs(a['grad']).max() > 0


# ---------------------------------------------------------------------------------------------------------------- the parallax scene
SCENE = dict(h=48, w=64, f=40.0, wall=10.0, plate=2.5, baseline=0.5, box=(16, 48, 8, 40), bins=8, cell=8)


def _texture(x, y):
    """the wall's grey level, smooth in the wall's own coordinates (metres), 0 .. 255"""
    return 127.5 + 60.0 * np.sin(0.9 * x + 0.4) + 60.0 * np.cos(0.7 * y - 0.3 * x)


def parallax_scene():
    """A far wall (z = 10 m in the camera frame) whose reflectance is its grey level, and a near plate (z = 2.5 m) of unrelated
    reflectance and grey that covers pixels u 16 .. 48, v 8 .. 40 of the 48 x 64 image (cell-aligned for cell 8, so that a wall point
    beside the plate shares no cell with it).  The LiDAR sits 0.5 m to the right of the camera: X_cam = X_lidar + (0.5, 0, 0).  It
    shoots one ray through every 0.8 pixel of a virtual image of its own; a ray that meets the plate returns a plate point, any
    other the wall.  The wall points whose ray passes the plate's edge on the LiDAR's side land, in the CAMERA's image, on pixels
    that show the plate: by parallax a strip baseline (wall - plate) / plate = 1.5 m wide on the wall, 6 pixels.
    -> pc (1,3,N) in the LiDAR frame, img uint8 (1,h,w,3), P (1,1,3,4) the true pose, value (1,N) to be binned over (0, 256),
    on_plate bool (N,), covered bool (N,): a wall point whose camera pixel shows the plate"""
    S = SCENE
    h, w, f, zw, zp, bl = S['h'], S['w'], S['f'], S['wall'], S['plate'], S['baseline']
    u0, u1, v0, v1 = S['box']
    rs = np.random.RandomState(21)
    # the plate in camera coordinates (metres): the back-projection of the pixel box at depth zp
    px0, px1, py0, py1 = (u0 - w / 2) * zp / f, (u1 - w / 2) * zp / f, (v0 - h / 2) * zp / f, (v1 - h / 2) * zp / f
    # the camera's image: per pixel centre, the plate where its ray meets it, else the wall's texture
    uu, vv = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    plate_px = (uu >= u0) & (uu < u1) & (vv >= v0) & (vv < v1)
    lev = _texture((uu - w / 2) * zw / f, (vv - h / 2) * zw / f)
    lev = np.where(plate_px, rs.randint(0, 256, (h, w)), lev)
    img = np.repeat(np.clip(lev, 0, 255).astype(np.uint8)[:, :, None], 3, 2)
    # the LiDAR's rays: directions ((a - w/2) / f, (b - h/2) / f, 1) from its origin at camera x = -bl ... +bl: X_cam = X_lidar + t
    t = np.array([bl, 0.0, 0.0])
    a, b = np.meshgrid(np.arange(-40, w + 40, 0.8) + 0.31, np.arange(-10, h + 10, 0.8) + 0.17)
    dx, dy = (a.reshape(-1) - w / 2) / f, (b.reshape(-1) - h / 2) / f
    at_plate = np.stack([dx * zp, dy * zp, np.full(dx.shape, zp)]) + t[:, None]          # camera coordinates of the ray at the plate's depth
    on_plate = (at_plate[0] >= px0) & (at_plate[0] < px1) & (at_plate[1] >= py0) & (at_plate[1] < py1)
    depth = np.where(on_plate, zp, zw)
    cam = np.stack([dx * depth, dy * depth, depth]) + t[:, None]
    pc = (cam - t[:, None]).astype(np.float32)
    value = np.where(on_plate, rs.randint(0, 256, dx.shape), np.clip(_texture(cam[0], cam[1]), 0, 255)).astype(np.float32)
    P = np.array([[f, 0, w / 2, f * bl], [0, f, h / 2, 0.0], [0, 0, 1.0, 0.0]])
    p = FC.project(pc, P, h, w)
    covered = ~on_plate & p['frame'] & (p['c'] >= u0) & (p['c'] < u1) & (p['r'] >= v0) & (p['r'] < v1)
    return pc[None], img[None], P[None, None], value[None], on_plate, covered


def test_parallax_scene_the_mask_hides_the_wall_behind_the_plate_and_raises_the_score():
    pc, img, P, value, on_plate, covered = parallax_scene()
    S = SCENE
    frame = FC.project(pc[0], P[0, 0], S['h'], S['w'])['frame']
    assert covered.sum() > 100 and (frame & on_plate).sum() > 500 and (frame & ~on_plate & ~covered).sum() > 1000
    plain = SC.score(pc, img, P, value, 0.0, 256.0, S['bins'])
    mm_plain, _ = SV.mi_mm(plain['mi'][0, 0], int(plain['count'][0, 0]), SV.occupancy(plain['hist'][0, 0]))
    for cell in (S['cell'], (8, 2)):
        ref = SV.score_visible(pc, img, P, value, 0.0, 256.0, S['bins'], cell)
        vis = ref['vis'][0, 0]
        assert not vis[covered].any()                             # every wall point whose pixel shows the plate is hidden
        assert (vis == (frame & ~covered)).all()                  # and nothing else is: the plate, and the wall beside it, stay
        print('cell %r: %d in frame, %d hidden; mi %.4f -> %.4f, mi_mm %.4f -> %.4f'
              % (cell, frame.sum(), covered.sum(), plain['mi'][0, 0], ref['mi'][0, 0], mm_plain, ref['mi_mm'][0, 0]))
        assert ref['count'][0, 0] == frame.sum() - covered.sum()
        assert ref['mi'][0, 0] > plain['mi'][0, 0] and ref['mi_mm'][0, 0] > mm_plain


# ------------------------------------------------------------------------------------------------ header, binding, slots, refusals
NEW = ('efgh_score_zmin_bytes', 'efgh_score_zmin', 'efgh_score_visible', 'efgh_score_hist_masked', 'efgh_score_soft_hist_masked',
       'efgh_score_soft_grad_masked', 'efgh_score_occupancy')


def test_header_and_binding_see_the_new_symbols_and_the_slots_stay():
    from efgh_amd import _C
    sigs = _C.signatures(open(_C.HEADER).read())
    i32, i64, vp, f32, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_double
    points = [vp, i64, i64, i32, i32, vp, i64, vp, i32, vp, i32, i32, i32, f32, f32, f64]
    assert sigs['efgh_score_zmin_bytes'] == (i64, [i32] * 6)
    assert sigs['efgh_score_zmin'] == (ctypes.c_int, [vp, i64, i64, i32, i32, vp, i32, i32, i32, i32, i32, f64, vp, vp])
    assert sigs['efgh_score_visible'] == (ctypes.c_int, [vp, i64, i64, i32, i32, vp, i32, i32, i32, i32, i32, f64, f64, f64, vp, vp, vp])
    assert sigs['efgh_score_occupancy'] == (ctypes.c_int, [vp, i32, i32, vp, vp])
    # the masked entry points: the arguments of the existing ones plus the mask, in front of the outputs
    assert sigs['efgh_score_hist_masked'] == (ctypes.c_int, points + [vp, vp, vp]) and sigs['efgh_score_hist'] == (ctypes.c_int, points + [vp, vp])
    assert sigs['efgh_score_soft_hist_masked'] == (ctypes.c_int, points + [i32, vp, vp, vp])
    assert sigs['efgh_score_soft_hist'] == (ctypes.c_int, points + [i32, vp, vp])
    assert sigs['efgh_score_soft_grad_masked'] == (ctypes.c_int, points + [i32, vp, vp, vp, vp, vp, vp])
    assert sigs['efgh_score_soft_grad'] == (ctypes.c_int, points + [i32, vp, vp, vp, vp, vp])
    lib = _C.lib()
    assert lib.efgh_version() == _C.ABI_VERSION == 4 and '#define EFGH_ABI_VERSION 4' in open(_C.HEADER).read()      # additive
    for name in NEW:
        assert getattr(lib, name).argtypes == sigs[name][1]
    assert Score.__slots__ == ('mi', 'nmi', 'hx', 'hy', 'hxy', 'count', 'hist')
    assert Refined.__slots__ == ('pose', 'mi', 'start_mi', 'trace', 'best_iter')
    assert Fused.__slots__ == ('rgb', 'state', 'uv', 'depth', 'index')
    assert issubclass(VisibleScore, Score) and VisibleScore.__slots__ == ('mi_mm', 'occupancy', 'mask', 'zmin')
    s = VisibleScore(mi=torch.tensor([[0., 2., 1.]], dtype=torch.float64), mi_mm=1, mask=2)
    assert s.best().tolist() == [1] and (s.mi_mm, s.mask, s.zmin, s.hist) == (1, 2, None, None) and not hasattr(s, '__dict__')
    # the workspace: 4 B K Hc Wc, cells clipped at the edges; the issue's example
    assert lib.efgh_score_zmin_bytes(1, 729, 900, 1600, 8, 8) == 4 * 729 * 113 * 200 and 65e6 < 4 * 729 * 113 * 200 < 67e6
    assert lib.efgh_score_zmin_bytes(2, 3, 48, 64, 6, 2) == 4 * 2 * 3 * 8 * 32 and lib.efgh_score_zmin_bytes(1, 1, 5, 7, 64, 64) == 4
    assert lib.efgh_score_zmin_bytes(1, 4096, 900, 1600, 1, 1) == -1 and lib.efgh_score_zmin_bytes(1, 1, 5, 7, 65, 1) == -1
    assert lib.efgh_score_zmin_bytes(1, 1, 5, 7, 0, 1) == -1 and lib.efgh_score_zmin_bytes(1, 4097, 5, 7, 1, 1) == -1


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """(addresses that are never dereferenced: every call below fails its argument checks on the host)"""
    from efgh_amd import _C
    L = _C.lib()
    PC, PP, Z, M, IMG, V, HIST, OCC = (i << 20 for i in range(1, 9))

    def head(B=2, N=64, K=2, H=48, W=64, ch=8, cw=8, min_depth=0.0, pc=PC, P=PP):
        return (pc, 256, 64, B, N, P, K, H, W, ch, cw, min_depth)
    common = ((dict(ch=0), b'cell_h = 0'), (dict(cw=65), b'cell_w = 65'), (dict(K=4097), b'K = 4097'), (dict(B=0), b'B = 0'), (dict(N=0), b'N = 0'),
              (dict(H=0), b'H = 0'), (dict(min_depth=float('nan')), b'min_depth'), (dict(pc=None), b'null pointer'),
              (dict(B=1, K=4096, H=900, W=1600, ch=1, cw=1), b'5898240000 cells (23592960000 bytes)'))
    for kw, word in common:
        assert L.efgh_score_zmin(*head(**kw), Z, None) != 0
        assert b'efgh_score_zmin' in L.efgh_last_error() and word in L.efgh_last_error(), (kw, L.efgh_last_error())
        assert L.efgh_score_visible(*head(**kw), 0.0, 0.0, Z, M, None) != 0
        assert b'efgh_score_visible' in L.efgh_last_error() and word in L.efgh_last_error(), (kw, L.efgh_last_error())
    assert L.efgh_score_zmin(*head(), None, None) != 0 and b'null pointer' in L.efgh_last_error()
    for tol, word in (((-1.0, 0.0), b'rel_tol = -1'), ((0.0, float('inf')), b'abs_tol = inf'), ((float('nan'), 0.0), b'rel_tol')):
        assert L.efgh_score_visible(*head(), *tol, Z, M, None) != 0 and word in L.efgh_last_error(), L.efgh_last_error()
    assert L.efgh_score_visible(*head(), 0.0, 0.0, Z, None, None) != 0 and b'null pointer' in L.efgh_last_error()
    points = (PC, 256, 64, 2, 64, V, 64, PP, 2, IMG, 48, 64, 8, 0.0, 1.0, 0.0)
    assert L.efgh_score_hist_masked(*points, None, HIST, None) != 0
    assert b'efgh_score_hist_masked: null pointer (mask' in L.efgh_last_error()
    assert L.efgh_score_hist_masked(*points[:12], 12, 0.0, 1.0, 0.0, M, HIST, None) != 0 and b'efgh_score_hist_masked: bins = 12' in L.efgh_last_error()
    assert L.efgh_score_soft_hist_masked(*points, 0, None, HIST, None) != 0 and b'efgh_score_soft_hist_masked: null pointer (mask' in L.efgh_last_error()
    assert L.efgh_score_soft_hist_masked(*points, 2, M, HIST, None) != 0 and b'efgh_score_soft_hist_masked: pool = 2' in L.efgh_last_error()
    assert L.efgh_score_soft_grad_masked(*points, 0, Z, Z, Z, None, Z, None) != 0
    assert b'efgh_score_soft_grad_masked: null pointer (mask' in L.efgh_last_error()
    assert L.efgh_score_soft_grad_masked(*points[:4], 1 << 23, *points[5:], 0, Z, Z, Z, M, Z, None) != 0 and b'N = 8388608' in L.efgh_last_error()
    for a, word in (((HIST, 0, 8), b'n_hist = 0'), ((HIST, 4, 12), b'bins = 12'), ((None, 4, 8), b'null pointer')):
        assert L.efgh_score_occupancy(*a, OCC, None) != 0
        assert b'efgh_score_occupancy' in L.efgh_last_error() and word in L.efgh_last_error()
    assert L.efgh_score_occupancy(HIST, 4, 8, None, None) != 0 and b'null pointer' in L.efgh_last_error()


def test_arguments_are_checked_before_any_launch():
    from efgh_amd import _C
    for bad in (0, 65, (8,), (8, 0), (1, 2, 3), 8.0, True, None, 'a'):
        with pytest.raises(_C.EfghError, match=r'Occlusion: cell: '):
            Occlusion(cell=bad)
    for kw, name in ((dict(rel_tol=-0.1), 'rel_tol: -0.1'), (dict(abs_tol=float('inf')), 'abs_tol: inf'), (dict(abs_tol=float('nan')), 'abs_tol: nan'),
                     (dict(rel_tol='x'), "rel_tol: 'x'")):
        with pytest.raises(_C.EfghError, match='Occlusion: ' + name):
            Occlusion(**kw)
    o = Occlusion((6, 2), 0.02, np.float32(0.5))
    assert (o.cell, o.rel_tol, o.abs_tol, o.grid(48, 64), o.grid(5, 7)) == ((6, 2), 0.02, 0.5, (8, 32), (1, 4))
    assert Occlusion().cell == (8, 8) and Occlusion(np.int64(64)).grid(5, 7) == (1, 1) and 'cell=(6, 2)' in repr(o)

    pc, img = torch.zeros(2, 4, 5), torch.zeros(2, 4, 6, 3, dtype=torch.uint8)
    T, val = torch.zeros(2, 3, 3, 4, dtype=torch.float64), torch.zeros(2, 5)
    bad = [('pc', dict(pc=pc.half())), ('pc', dict(pc=pc[:, :2])), ('cam_T_velo', dict(T=torch.zeros(2, 3, 3))), ('cam_T_velo', dict(T=T.half())),
           ('cam_T_velo', dict(T=torch.zeros(2, 4097, 3, 4))), ('img', dict(img=img[:1])), ('value', dict(pc=pc[:, :3])),
           ('value', dict(value=val.double())), ('value_range', dict(value=val, value_range=(1.0, 1.0))), ('bins', dict(bins=256)),
           ('bins', dict(bins=12)), ('min_depth', dict(min_depth=-1.0)), ('occlusion', dict(occlusion=8)), ('occlusion', dict(occlusion=(8, 2))),
           ('pc', {})]                                           # everything valid but on the CPU: there is no CPU path
    for who, fn, more in (('score_visible', score_visible, []), ('score_soft_visible', score_soft_visible, [('pool', dict(pool=1)), ('pool', dict(pool=None))])):
        for name, kw in bad + more:
            kw = dict(kw)
            a = dict(pc=pc, img=img, T=T)
            a.update({k: kw.pop(k) for k in list(kw) if k in a})
            with pytest.raises(_C.EfghError, match=r'%s: %s\b' % (who, name)):
                fn(a['pc'], a['img'], a['T'], **kw)
        with pytest.raises(_C.EfghError, match='bins: 256'):
            fn(pc, img, T, bins=256)
        with pytest.raises(_C.EfghError, match='CPU tensor'):
            fn(pc, img, T.float(), value=val.to(torch.uint8), occlusion=Occlusion(1), want_mask=True)
    # the workspace limit: 4096 candidates of a 900 x 1600 image at cell 1 are 5.9e9 cells
    wide_T, wide_img = torch.zeros(1, 4096, 3, 4), torch.zeros(1, 900, 1600, 3, dtype=torch.uint8)
    for fn, who in ((score_visible, 'score_visible'), (score_soft_visible, 'score_soft_visible')):
        with pytest.raises(_C.EfghError, match=r'%s: occlusion: B = 1, K = 4096 and cell = \(1, 1\) on 900 x 1600 need a zmin workspace of 23592960000 bytes'
                           r'.*larger cell or fewer candidates' % who):
            fn(pc[:1], wide_img, wide_T, occlusion=Occlusion(1))
    with pytest.raises(_C.EfghError, match=r'visible_mask: occlusion: B = 1, K = 4096 .* 23592960000 bytes'):
        visible_mask(pc[:1], (900, 1600), wide_T, Occlusion(1))
    for name, a in (('pc', (pc.half(), img, T)), ('cam_T_velo', (pc, img, T[:1])), ('img', (pc, img[:1], T)), ('img', (pc, (4, 0), T)),
                    ('img', (pc, (4, 6, 3), T)), ('img', (pc, (4.0, 6), T)), ('occlusion', (pc, img, T, 8)), ('min_depth', (pc, img, T, None, -1.0)),
                    ('pc', (pc, (4, 6), T)), ('pc', (pc, img, T[:, 0]))):
        with pytest.raises(_C.EfghError, match=r'visible_mask: %s\b' % name):
            visible_mask(*a)
    with pytest.raises(_C.EfghError, match='CPU tensor'):
        visible_mask(pc, (4, 6), T)
    # occupancy and miller_madow
    for bad, word in ((None, 'expected a tensor'), (torch.zeros(8, 8), 'dtype'), (torch.zeros(8, 16, dtype=torch.int32), 'bins, bins'),
                      (torch.zeros(12, 12, dtype=torch.int32), 'bins, bins'), (torch.zeros(0, 8, 8, dtype=torch.int32), 'bins, bins'),
                      (torch.zeros(3, 8, 8, dtype=torch.int32), 'CPU tensor')):
        with pytest.raises(_C.EfghError, match='occupancy: hist: .*' + word):
            occupancy(bad)
    with pytest.raises(_C.EfghError, match='miller_madow: s: expected a Score'):
        miller_madow(torch.zeros(3))
    with pytest.raises(_C.EfghError, match='miller_madow: s: .*want_hist=True'):
        miller_madow(Score(mi=torch.zeros(1, 1), count=torch.zeros(1, 1, dtype=torch.int32)))
    # refine hands its keywords through a partial of the new scorer, which checks them in front of any launch
    with pytest.raises(_C.EfghError, match=r'score_soft_visible: pc: a CPU tensor'):
        refine(pc, img, torch.zeros(2, 3, 4), scorer=functools.partial(score_soft_visible, occlusion=Occlusion((8, 2), 0.02, 0.1)))
