"""Improving a pose without ground truth: a coherent synthetic sweep and a smooth image, the true pose perturbed by a fraction of a
degree and a few centimetres, and `efgh_amd.common.refine` climbing the mutual information of the soft histogram (score_soft) back.

As in examples/score_synthetic.py the two sensors are made to agree the way a real pair does: every point's value is the grey level
the TRUE pose finds under it.  Printed: the MI at the start and at the best iterate, and the mean reprojection offset against the
true pose before and after, over the points the true pose has in frame.  `refine` is a local optimiser: start it too far off (try
--rot-deg 3) and it stops on another maximum.

    python examples/refine_synthetic.py
    python examples/refine_synthetic.py --raw 376 1241 --points 65536 --rot-deg 0.3 --trans 0.03 --bins 32 --iters 150
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efgh_amd import synthetic as syn  # noqa: E402
from efgh_amd.common import candidates_around, fuse, refine  # noqa: E402


def smooth_image(h, w):
    """uint8 (1,h,w,3): a few low-frequency waves around a mid grey"""
    y, x = np.mgrid[0:h, 0:w]
    a = 128 + 60 * np.sin(x / w * 9.0 + 1.0) * np.cos(y / h * 5.0) + 40 * np.sin((x + 2 * y) / w * 14.0)
    return np.repeat(np.clip(a, 0, 255).astype(np.uint8)[None, :, :, None], 3, 3)


def offset(pc, P, true, h, w):
    """mean distance in pixels between the projections under P and under `true`, over the points `true` has in frame (torch, float64)"""
    X = torch.cat([pc[0, :3].double(), torch.ones_like(pc[0, :1], dtype=torch.float64)])
    a, b = P[0] @ X, true[0].double() @ X
    ua, ub = a[:2] / a[2], b[:2] / b[2]
    m = (b[2] > 0) & (ub[0] >= 0) & (ub[0] < w) & (ub[1] >= 0) & (ub[1] < h)
    return float((ua - ub)[:, m].norm(dim=0).mean())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--raw', type=int, nargs=2, default=[256, 512])
    ap.add_argument('--points', type=int, default=32768)
    ap.add_argument('--rot-deg', type=float, default=0.3, help='the start: this much about every LiDAR axis off the true pose')
    ap.add_argument('--trans', type=float, default=0.03, help='... and this many metres along every axis')
    ap.add_argument('--bins', type=int, default=32)
    ap.add_argument('--iters', type=int, default=150)
    ap.add_argument('--rot-step-deg', type=float, default=0.02)
    ap.add_argument('--trans-step', type=float, default=0.002)
    a = ap.parse_args(argv)
    h, w = a.raw
    pcd = torch.from_numpy(syn.coherent_sweep(a.points, 3)).cuda()[None].contiguous()
    cam = torch.from_numpy(smooth_image(h, w)).cuda()
    true = torch.from_numpy(np.ascontiguousarray(syn.calib_and_A((h, w))[0][None])).cuda()
    # the grey level under the true projection, as a uint8 value per point (0 where the point is not in frame)
    rgb = fuse(pcd, cam, true, bilinear=False, want=('rgb',)).rgb.to(torch.int64)
    value = ((19595 * rgb[..., 0] + 38470 * rgb[..., 1] + 7471 * rgb[..., 2] + 32768) >> 16).to(torch.uint8)
    start = candidates_around(true, (a.rot_deg,) * 3, (a.trans,) * 3, steps=1)[:, -1]      # every axis at +1 step
    r = refine(pcd, cam, start, value=value, bins=a.bins, iters=a.iters, rot_step_deg=a.rot_step_deg, trans_step=a.trans_step)
    before, after = offset(pcd, start, true, h, w), offset(pcd, r.pose, true, h, w)      # the host reads, for the print
    print('start    mi %.4f nats   reprojection offset %.3f px' % (float(r.start_mi), before))
    print('refined  mi %.4f nats   reprojection offset %.3f px   (iterate %d of %d)' % (float(r.mi), after, int(r.best_iter), a.iters))
    return before, after


if __name__ == '__main__':
    main()
