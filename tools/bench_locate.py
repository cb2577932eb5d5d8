"""Lattice point query alone at the bench size: the vertex index of level 0 of a 131072-point sweep (efgh_lattice_index_build) and
one query of 131072 points on it (efgh_lattice_locate) - the level's own points (every corner found) and a second sweep (a mix of
found and absent corners).  Event time of `--iters` back-to-back launches, after warm-up; a launch sequence this short is mostly
launch overhead, so the per-launch figure is an upper bound of the kernel time."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from efgh_amd import lattice, ops, synthetic as syn

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=int, default=131072)
ap.add_argument('--iters', type=int, default=50)
a = ap.parse_args()
SCALES = (1.0, 0.75, 0.5, 0.25, 0.125)


def timed(fn):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.iters * 1e3


pc = torch.from_numpy(syn.lidar_sweep(a.points, 0)).cuda()
other = torch.from_numpy(syn.lidar_sweep(a.points, 1)).cuda()
lv = lattice.build_pyramid(pc, SCALES)[0]
pts, cstride, sid, pps, s = lv._src
us = timed(lambda: ops.lattice_index(pts, cstride, sid, pps, 1, s, lv.list, lv.vseg, lv.vsid, lv.info, lv.H))
print('index build, level 0: %d points, H = %d: %.1f us (allocation + 3 launches)' % (lv.n_in, lv.H, us))
index = lv.vertex_index()
for name, q in (('own points', pc), ('second sweep', other)):
    us = timed(lambda: ops.lattice_locate(index, q, q.shape[1], None, q.shape[1], q.shape[1], s, 1, lv.H, lv.info))
    absent, none = lattice.OutPoints.locate(lv, q).missing()
    print('locate %d points (%s): %.1f us (2 allocations + counter fill + 1 launch); absent corners %d, points without a corner %d'
          % (q.shape[1], name, us, absent, none))
