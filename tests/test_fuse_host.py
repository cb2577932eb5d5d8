"""tests/fuse_contract.py (the numpy statement the fuse kernels are held to bit for bit) against properties that are not taken from
it, the PLY writer / reader, and the argument checks of `fuse`, which come before any launch.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_contract as FC  # noqa: E402

H, W = 13, 17
IDENT = np.array([[1., 0, 0, 0], [0, 1., 0, 0], [0, 0, 1., 0]])


def _cloud(n, seed, spread=1.3):
    """points that project (through IDENT) around and into the H x W frame, a tenth of them behind the camera; many share pixels"""
    rs = np.random.RandomState(seed)
    w = rs.randint(1, 40, n) / 4.0                              # few distinct depths: equal float32 depths do occur
    w[rs.rand(n) < 0.1] *= -1
    u = (rs.rand(n) * spread - (spread - 1) / 2) * W
    v = (rs.rand(n) * spread - (spread - 1) / 2) * H
    return np.stack([u * w, v * w, w]).astype(np.float32)


def _project_scalar(p, T, min_depth):
    """one point in Python floats (float64, one rounding per operation): (in front, in frame, r, c, float32 depth)"""
    px, py, pz = float(p[0]), float(p[1]), float(p[2])
    x = ((T[0][0] * px + T[0][1] * py) + T[0][2] * pz) + T[0][3]
    y = ((T[1][0] * px + T[1][1] * py) + T[1][2] * pz) + T[1][3]
    w = ((T[2][0] * px + T[2][1] * py) + T[2][2] * pz) + T[2][3]
    if not w > min_depth:
        return False, False, 0, 0, None
    u, v = x / w, y / w
    if not (0 <= u < W and 0 <= v < H):
        return True, False, 0, 0, None
    return True, True, int(v), int(u), np.float32(w)


@pytest.mark.parametrize('radius', [0, 2])
def test_zbuffer_is_the_brute_force_nearest_per_pixel(radius):
    pc = _cloud(400, 1)
    T = IDENT.tolist()
    best = {}
    for i in range(pc.shape[1]):
        _, frame, r, c, d = _project_scalar(pc[:, i], T, 0.0)
        if not frame:
            continue
        for rr in range(max(r - radius, 0), min(r + radius, H - 1) + 1):
            for cc in range(max(c - radius, 0), min(c + radius, W - 1) + 1):
                if (rr, cc) not in best or (d, i) < best[(rr, cc)]:
                    best[(rr, cc)] = (d, i)
    depth, index = FC.maps(FC.zbuffer(pc, IDENT, H, W, radius))
    assert len(best) > 50 and (index >= 0).sum() == len(best)
    for (rr, cc), (d, i) in best.items():
        assert index[rr, cc] == i and depth[rr, cc] == d


def test_radius_zero_occludes_only_behind_a_strictly_nearer_float32_depth():
    pc = _cloud(600, 2)
    state, _, _ = FC.resolve(pc, IDENT, np.zeros((H, W, 3), np.uint8), FC.zbuffer(pc, IDENT, H, W, 0))
    proj = [_project_scalar(pc[:, i], IDENT.tolist(), 0.0) for i in range(pc.shape[1])]
    seen = {2: 0, 3: 0}
    for i, (front, frame, r, c, d) in enumerate(proj):
        if not frame:
            continue
        nearer = any(f2 and (r2, c2) == (r, c) and d2 < d for _, f2, r2, c2, d2 in proj)
        assert state[i] == (FC.OCCLUDED if nearer else FC.VISIBLE), i
        seen[int(state[i])] += 1
    assert seen[2] > 20 and seen[3] > 20


def test_states_partition_the_points():
    pc = _cloud(500, 3)
    pc[:, :4] = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [np.inf, np.inf, np.inf]], np.float32).T
    img = np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)
    state, rgb, uv = FC.resolve(pc, IDENT, img, FC.zbuffer(pc, IDENT, H, W, 1, 0.5), min_depth=0.5)
    proj = [_project_scalar(pc[:, i], IDENT.tolist(), 0.5) for i in range(pc.shape[1])]
    assert set(np.unique(state)) == {0, 1, 2, 3}
    assert (state[:4] == 0).all()
    for i, (front, frame, _, _, _) in enumerate(proj[4:], 4):
        assert (state[i] >= 1) == front and (state[i] >= 2) == frame
    assert (rgb[state < 2] == 0).all()
    assert (np.isnan(uv).all(1) == (state == 0)).all() and not np.isnan(uv[state >= 1]).any()


def _at(u, v, w=2.0):
    return np.array([[u * w], [v * w], [w]], dtype=np.float32)


def test_bilinear_at_a_pixel_centre_is_that_pixel():
    img = np.random.RandomState(4).randint(0, 256, (H, W, 3)).astype(np.uint8)
    for r, c in ((0, 0), (H - 1, W - 1), (5, 9), (0, W - 1)):
        pc = _at(c + 0.5, r + 0.5)
        state, rgb, _ = FC.resolve(pc, IDENT, img, FC.zbuffer(pc, IDENT, H, W), bilinear=True)
        assert state[0] == 3 and (rgb[0] == img[r, c]).all()


def test_bilinear_clamps_at_the_frame():
    img = np.random.RandomState(5).randint(0, 256, (H, W, 3)).astype(np.uint8)
    for u, c in ((0.0, 0), (W - 2.0 ** -10, W - 1)):            # fx = -0.5: both taps are column 0; fx just below W - 0.5: both W - 1
        pc = _at(u, 3.5)
        state, rgb, _ = FC.resolve(pc, IDENT, img, FC.zbuffer(pc, IDENT, H, W), bilinear=True)
        assert state[0] == 3 and (rgb[0] == img[3, c]).all(), u
    for v, r in ((0.0, 0), (H - 2.0 ** -10, H - 1)):
        pc = _at(6.5, v)
        state, rgb, _ = FC.resolve(pc, IDENT, img, FC.zbuffer(pc, IDENT, H, W), bilinear=True)
        assert state[0] == 3 and (rgb[0] == img[r, 6]).all(), v


def test_bilinear_half_way_between_0_and_1_rounds_up():
    img = np.array([[[0, 0, 0], [1, 1, 1]]], dtype=np.uint8)      # 1 x 2
    pc = _at(1.0, 0.5)
    _, rgb, _ = FC.resolve(pc, IDENT, img, FC.zbuffer(pc, IDENT, 1, 2), bilinear=True)
    assert (rgb[0] == 1).all()


def test_ply_round_trip(tmp_path):
    from efgh_amd.io.formats import read_ply, write_ply
    rs = np.random.RandomState(6)
    xyz = rs.randn(37, 3).astype(np.float32)
    rgb = rs.randint(0, 256, (37, 3)).astype(np.uint8)
    inten, lab = rs.rand(37).astype(np.float32), rs.randint(0, 256, 37).astype(np.uint8)
    path = str(tmp_path / 'a.ply')
    write_ply(path, xyz, rgb, intensity=inten, label=lab)
    head = open(path, 'rb').read().split(b'end_header\n')[0].decode().split('\n')
    assert head[:3] == ['ply', 'format binary_little_endian 1.0', 'element vertex 37']
    assert head[3:-1] == ['property float x', 'property float y', 'property float z', 'property uchar red', 'property uchar green',
                          'property uchar blue', 'property float intensity', 'property uchar label']
    assert os.path.getsize(path) == len('\n'.join(head)) + len('end_header\n') + 37 * (12 + 3 + 4 + 1)
    got = read_ply(path)
    assert sorted(got) == ['intensity', 'label', 'rgb', 'xyz']
    assert got['xyz'].dtype == np.float32 and (got['xyz'] == xyz).all() and got['rgb'].dtype == np.uint8 and (got['rgb'] == rgb).all()
    assert got['intensity'].dtype == np.float32 and (got['intensity'] == inten).all() and (got['label'] == lab).all()
    # no rows, and no colours
    write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), intensity=np.zeros(0, np.float32))
    got = read_ply(path)
    assert got['xyz'].shape == (0, 3) and got['rgb'].shape == (0, 3) and got['intensity'].shape == (0,)
    write_ply(path, xyz)
    got = read_ply(path)
    assert got['rgb'] is None and (got['xyz'] == xyz).all()
    with pytest.raises(ValueError):
        write_ply(path, xyz, rgb, red=inten)
    with pytest.raises(ValueError):
        write_ply(path, xyz, rgb, intensity=inten[:5])


def test_fuse_is_exported_and_checks_its_arguments_before_any_launch():
    import torch
    from efgh_amd import _C
    from efgh_amd.common import Fused, fuse
    assert Fused.__slots__ == ('rgb', 'state', 'uv', 'depth', 'index')
    pc, img, T = torch.zeros(2, 3, 5), torch.zeros(2, 4, 6, 3, dtype=torch.uint8), torch.zeros(2, 3, 4, dtype=torch.float64)
    bad = [
        ('pc', dict(pc=pc.half())), ('pc', dict(pc=pc[:, :2])), ('pc', dict(pc=pc[0])),
        ('cam_T_velo', dict(T=torch.zeros(2, 3, 3))), ('cam_T_velo', dict(T=T.half())), ('cam_T_velo', dict(T={'e_l': T})),
        ('img', dict(img=img[:1])), ('img', dict(img=torch.zeros(2, 4, 6, 3))), ('img', dict(img=img.int())),
        ('radius', dict(radius=-1)), ('radius', dict(radius=9)), ('radius', dict(radius=1.5)),
        ('rel_tol', dict(rel_tol=-1e-3)), ('abs_tol', dict(abs_tol=float('inf'))), ('min_depth', dict(min_depth=float('nan'))),
        ('want', dict(want=('rgb', 'colour'))), ('want', dict(want=())),
        ('pc', {}),                                              # everything valid but on the CPU: there is no CPU path
    ]
    for name, kw in bad:
        a = dict(pc=pc, img=img, T=T)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        with pytest.raises(_C.EfghError, match=r'fuse: %s\b' % name):
            fuse(a['pc'], a['img'], a['T'], **kw)
    # the accepted image forms reach the device check, which is the last one
    for im in (torch.zeros(2, 3, 4, 6), img, torch.zeros(2, 3, 4, 6, dtype=torch.float64)):
        with pytest.raises(_C.EfghError, match='CPU tensor'):
            fuse(pc, im, {'cam_T_velo': T.float()})
    with pytest.raises(_C.EfghError, match='CPU tensor'):
        fuse(pc[:1], img[0], T[:1])
