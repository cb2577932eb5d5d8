"""Scoring a pose on the points the camera can see: a far wall whose reflectance is its grey level, a near plate of unrelated
reflectance and grey in the middle of the image, and a LiDAR that sits beside the camera.  By parallax the LiDAR sees a strip of the
wall whose pixels show the plate; `score` pairs those reflectances with the plate's grey, `score_visible` drops them with a depth test
per candidate (efgh_amd.common.score_vis) and returns the Miller-Madow corrected estimate next to the plug-in one.

    python examples/score_visible_synthetic.py
    python examples/score_visible_synthetic.py --baseline 1.0 --cell 8 2 --abs-tol 0.1

The wall and the plate face the camera, so under the true pose a zero tolerance hides nothing by mistake.  Under the perturbed pose
both are oblique to the image plane, and the stated limit of a cell-based test shows: with the default zero tolerance a cell hides
the far end of a surface from its near end, and only a few hundred points stay visible (`count` says so, and `mi_mm` charges the
sparse histogram for it).  A tolerance (--rel-tol, --abs-tol) that allows for the depth range of a surface inside one cell is the
caller's choice.  What the example prints is what this one synthetic scene gives: no effect on registration accuracy is claimed."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efgh_amd.common import Occlusion, candidates_around, miller_madow, score, score_visible  # noqa: E402


def texture(x, y):
    return 127.5 + 60.0 * np.sin(0.9 * x + 0.4) + 60.0 * np.cos(0.7 * y - 0.3 * x)


def scene(h, w, f, wall, plate, baseline, seed=0):
    """-> pc float32 (1,3,N) in the LiDAR frame, img uint8 (1,h,w,3), P (1,3,4) float64 the true pose, value float32 (1,N) over (0, 256)"""
    rs = np.random.RandomState(seed)
    u0, u1, v0, v1 = w // 4, 3 * w // 4, h // 6, 5 * h // 6           # the plate's pixels in the camera image
    uu, vv = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    on = (uu >= u0) & (uu < u1) & (vv >= v0) & (vv < v1)
    lev = np.where(on, rs.randint(0, 256, (h, w)), texture((uu - w / 2) * wall / f, (vv - h / 2) * wall / f))
    img = np.repeat(np.clip(lev, 0, 255).astype(np.uint8)[:, :, None], 3, 2)
    t = np.array([baseline, 0.0, 0.0])                            # X_cam = X_lidar + t
    a, b = np.meshgrid(np.arange(-w, 2 * w, 0.8) + 0.31, np.arange(-h // 4, h + h // 4, 0.8) + 0.17)
    dx, dy = (a.reshape(-1) - w / 2) / f, (b.reshape(-1) - h / 2) / f
    px, py = dx * plate + t[0], dy * plate                        # the ray at the plate's depth, camera coordinates
    hit = (px >= (u0 - w / 2) * plate / f) & (px < (u1 - w / 2) * plate / f) & (py >= (v0 - h / 2) * plate / f) & (py < (v1 - h / 2) * plate / f)
    depth = np.where(hit, plate, wall)
    cam = np.stack([dx * depth, dy * depth, depth]) + t[:, None]
    value = np.where(hit, rs.randint(0, 256, dx.shape), np.clip(texture(cam[0], cam[1]), 0, 255)).astype(np.float32)
    P = np.array([[f, 0, w / 2, f * baseline], [0, f, h / 2, 0.0], [0, 0, 1.0, 0.0]])
    return (cam - t[:, None]).astype(np.float32)[None], img[None], P[None], value[None]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--raw', type=int, nargs=2, default=[96, 128])
    ap.add_argument('--baseline', type=float, default=0.5, help='metres between LiDAR and camera')
    ap.add_argument('--cell', type=int, nargs=2, default=[8, 8])
    ap.add_argument('--rel-tol', type=float, default=0.0)
    ap.add_argument('--abs-tol', type=float, default=0.0)
    ap.add_argument('--bins', type=int, default=8)
    a = ap.parse_args(argv)
    h, w = a.raw
    pc, img, P, value = (torch.from_numpy(x).cuda() for x in scene(h, w, 80.0, 10.0, 2.5, a.baseline))
    # candidate 0: the true pose; candidate 1: half a degree and 5 cm off on every axis
    around = candidates_around(P, (0.5,) * 3, (0.05,) * 3, steps=1)
    poses = torch.stack([around[:, 0], around[:, -1]], 1)
    kw = dict(value=value, value_range=(0.0, 256.0), bins=a.bins)
    plain = score(pc, img, poses, want_hist=True, **kw)
    vis = score_visible(pc, img, poses, occlusion=Occlusion(tuple(a.cell), a.rel_tol, a.abs_tol), **kw)
    rows = [[t[0].tolist() for t in (s.mi, mm, s.count)] for s, mm in ((plain, miller_madow(plain)), (vis, vis.mi_mm))]      # the host reads
    for name, (mi, mm, count) in zip(('every point in frame', 'visible points only'), rows):
        for i, pose in enumerate(('true pose', 'perturbed')):
            print('%-22s %-10s mi %.4f nats   mi_mm %.4f   %d points' % (name, pose, mi[i], mm[i], count[i]))
    return rows


if __name__ == '__main__':
    main()
