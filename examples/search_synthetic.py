"""The whole chain without ground truth: look around a pose, climb from the few best places, hand back the best end.  The scene is
examples/refine_synthetic.py's - a coherent synthetic sweep, a smooth image, every point's value the grey level the TRUE pose finds
under it - but the start is several times further off.

`efgh_amd.common.search` scores the grid of `candidates_around` the start, keeps the --keep best candidates, and climbs from all of
them at once with `refine_multi` (one device-side step an iteration for every start).  Printed: `refine` from the start alone, then
the search: the MI and the mean reprojection offset against the true pose, over the points the true pose has in frame.  With the
defaults (this smooth scene has a wide basin, so `refine` alone gets home from here too; the search ends closer):

    start          mi 0.6669 nats   reprojection offset 25.737 px
    refine alone   mi 2.3067 nats   reprojection offset 0.301 px
    search         mi 2.3071 nats   reprojection offset 0.104 px   (grid of 125, kept [1, 26, 2, 27, 51, 3, 52, 6], start 0 of them won)

A start from which `refine` alone does NOT get home is in tests/test_refine_multi_host.py (the peak scene's far start).

    python examples/search_synthetic.py
    python examples/search_synthetic.py --raw 376 1241 --points 65536 --rot-deg 1.5 --trans 0.15 --grid-steps 2 --keep 8
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efgh_amd import synthetic as syn  # noqa: E402
from efgh_amd.common import candidates_around, fuse, refine, search  # noqa: E402
from refine_synthetic import offset, smooth_image  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--raw', type=int, nargs=2, default=[256, 512])
    ap.add_argument('--points', type=int, default=32768)
    ap.add_argument('--rot-deg', type=float, default=1.5, help='the start: this much about the LiDAR x and z axes off the true pose')
    ap.add_argument('--trans', type=float, default=0.15, help='... and this many metres along y')
    ap.add_argument('--grid-steps', type=int, default=2, help='the grid has 2 * steps + 1 values on each of the three axes, rot-deg / steps apart')
    ap.add_argument('--keep', type=int, default=8)
    ap.add_argument('--bins', type=int, default=32)
    ap.add_argument('--iters', type=int, default=150)
    ap.add_argument('--rot-step-deg', type=float, default=0.02)
    ap.add_argument('--trans-step', type=float, default=0.002)
    a = ap.parse_args(argv)
    h, w = a.raw
    pcd = torch.from_numpy(syn.coherent_sweep(a.points, 3)).cuda()[None].contiguous()
    cam = torch.from_numpy(smooth_image(h, w)).cuda()
    true = torch.from_numpy(np.ascontiguousarray(syn.calib_and_A((h, w))[0][None])).cuda()
    rgb = fuse(pcd, cam, true, bilinear=False, want=('rgb',)).rgb.to(torch.int64)
    value = ((19595 * rgb[..., 0] + 38470 * rgb[..., 1] + 7471 * rgb[..., 2] + 32768) >> 16).to(torch.uint8)
    start = candidates_around(true, (a.rot_deg, 0, a.rot_deg), (0, a.trans, 0), steps=1)[:, -1]      # the three axes at +1 step
    kw = dict(value=value, bins=a.bins, iters=a.iters, rot_step_deg=a.rot_step_deg, trans_step=a.trans_step)
    alone = refine(pcd, cam, start, **kw)
    s = a.grid_steps
    found = search(pcd, cam, start, rot_deg=(a.rot_deg / s, 0, a.rot_deg / s), trans=(0, a.trans / s, 0), steps=s, keep=a.keep, **kw)
    r = found.refined                                            # (the host reads, for the print)
    before, lone, after = offset(pcd, start, true, h, w), offset(pcd, alone.pose, true, h, w), offset(pcd, found.pose, true, h, w)
    print('start          mi %.4f nats   reprojection offset %.3f px' % (float(alone.start_mi), before))
    print('refine alone   mi %.4f nats   reprojection offset %.3f px' % (float(alone.mi), lone))
    print('search         mi %.4f nats   reprojection offset %.3f px   (grid of %d, kept %s, start %d of them won)'
          % (float(r.mi[0, r.best()]), after, found.coarse.mi.shape[1], found.kept[0].tolist(), int(r.best())))
    return before, lone, after


if __name__ == '__main__':
    main()
