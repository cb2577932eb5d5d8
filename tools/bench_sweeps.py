"""What multi-sweep accumulation costs in sample preparation: `preproc_pcd` on a 7-sweep SweepSet against `preproc_pcd` on
ONE [n, 4] array of the same total point count (the single-sweep path, whose kernels this feature does not touch), at a
nuScenes-sized set (7 x ~34k points, ego box on) and a KITTI-sized one (7 x ~120k points).

Method: inputs resident on the device, warm-up, then ROUNDS interleaved rounds (plain, sweeps, plain, sweeps, ...) of CALLS
calls each, every round closed by a device synchronise; per-call time of a round = round time / CALLS.  Reported: the median
over the rounds and their min .. max (the spread), and the ratio of the medians.  A second pair of columns includes staging
from host arrays (the concatenate of the float32 sweeps and the uploads).  The last column is the host time of the numpy
accumulation the reference's loaders do for the same set (float64 transform per sweep, concatenate; ego mask for nuScenes),
on one core, as INTEGRATION section 5 gives it for the single sweep.

    python tools/bench_sweeps.py [--out profiles/sweeps.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from efgh_amd.data import SweepSet, preproc_gt, preproc_pcd  # noqa: E402

ROUNDS, CALLS, WARM = 9, 40, 10
NUM_POINTS = 131072


def make_set(k, n_each, stride, seed, spread):
    rng = np.random.default_rng(seed)
    sweeps, Ms = [], []
    for i in range(k):
        p = np.empty((n_each, stride), np.float32)
        p[:, :2] = rng.uniform(-spread, spread, (n_each, 2))
        p[:, 2] = rng.uniform(-3, 3, n_each)
        if stride == 4:
            p[:, 3] = 0.5
        sweeps.append(p)
        if i:
            a = 0.01 * i
            M = np.eye(4)
            M[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
            M[:3, 3] = (0.8 * i, 0.05 * i, 0.01 * i)
            Ms.append(M)
    return sweeps, Ms


def numpy_accumulation(sweeps, Ms, ego_box):
    """the loaders' host work (kitti_odom_loader.py:184-186,221-223; nusc_loader.py:88-93,113-116,144)"""
    out = []
    for k, p in enumerate(sweeps):
        pc = p.T[:3, :]
        if ego_box is not None:
            inside = np.logical_and(np.logical_and(pc[0] < ego_box[0], pc[0] > -ego_box[0]),
                                    np.logical_and(pc[1] < ego_box[1], pc[1] > -ego_box[1]))
            pc = pc[:, np.logical_not(inside)]
        if k:
            pc = np.concatenate((pc, np.ones((1, pc.shape[1]), dtype=pc.dtype)), axis=0)
            pc = (Ms[k - 1] @ pc)[:3, :]
        out.append(pc)
    return np.concatenate(out, axis=1).T


def rounds(fns):
    """interleaved rounds of the callables -> per-call milliseconds, one list per callable"""
    for f in fns:
        for _ in range(WARM):
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, f in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                f()
            torch.cuda.synchronize()
            ms[i].append((time.perf_counter() - t0) / CALLS * 1e3)
    return ms


def fmt(v):
    return '%.3f ms (%.3f .. %.3f)' % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'sweeps.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sweeps: needs the GPU (there is no CPU path to time)')
    gts = preproc_gt(0.1, -0.05, 0.3, 0.2, 0.1, -0.3, 0.0)
    lines = ['preproc_pcd, %d points out, %s; %d interleaved rounds of %d calls, median (min .. max) per call'
             % (NUM_POINTS, torch.cuda.get_device_name(0), ROUNDS, CALLS)]
    for label, k, n_each, stride, ego, spread in (('nuScenes-sized', 7, 34720, 3, (0.8, 2.7), 60.0),
                                                  ('KITTI-sized', 7, 120000, 4, None, 70.0)):
        sweeps, Ms = make_set(k, n_each, stride, 5, spread)
        n = k * n_each
        plain = np.zeros((n, 4), np.float32)
        plain[:, :3] = np.concatenate([s[:, :3] for s in sweeps])
        plain_d = torch.from_numpy(plain).cuda()
        ss = SweepSet(sweeps, Ms, ego_box=ego)
        kept = int(ss.kept_indices().numel())
        res, res_ss = rounds([lambda: preproc_pcd(plain_d, gts, NUM_POINTS), lambda: preproc_pcd(ss, gts, NUM_POINTS)])
        h2d, h2d_ss = rounds([lambda: preproc_pcd(plain, gts, NUM_POINTS),
                              lambda: preproc_pcd(SweepSet(sweeps, Ms, ego_box=ego), gts, NUM_POINTS)])
        t0 = time.perf_counter()
        for _ in range(3):
            numpy_accumulation(sweeps, Ms, ego)
        host = (time.perf_counter() - t0) / 3 * 1e3
        ratio = statistics.median(res_ss) / statistics.median(res)
        spread_rel = (max(res) - min(res)) / statistics.median(res)
        lines += ['',
                  '%s: %d sweeps x %d points (row stride %d%s), %d of %d rows kept' % (
                      label, k, n_each, stride, ', ego box (%.1f, %.1f)' % ego if ego else '', kept, n),
                  '  one [n, 4] array, resident      %s' % fmt(res),
                  '  SweepSet, resident              %s   ratio %.3f (the single-sweep path spreads %.1f %% round to round)'
                  % (fmt(res_ss), ratio, 100 * spread_rel),
                  '  one [n, 4] array, from host     %s' % fmt(h2d),
                  '  SweepSet, from host arrays      %s' % fmt(h2d_ss),
                  '  numpy accumulation on the host  %.1f ms (one core; the GPU path never builds this cloud)' % host]
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
