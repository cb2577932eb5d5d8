"""What thinning on a voxel grid costs in sample preparation, and that leaving it off costs nothing: `preproc_pcd` on a 7-sweep
SweepSet with voxel_size = None, 0.1 and 0.2 at the two sizes of tools/bench_sweeps.py (7 x 34 720 rows at stride 3, 7 x 120 000 rows
at stride 4), both with the ego box, 131 072 points out.

The scene.  bench_sweeps.py draws every sweep uniformly in a box, so no two points share a 0.1 m voxel and there is nothing to
thin.  Here the sweeps re-observe ONE static scene, as accumulated sweeps do: a ground plane and a ring of walls sampled with a
spinning sensor's density (range uniform, so the density per area falls with 1/r), every sweep from its own pose a little further
along the drive, moved into its own frame and stored as float32.  Seeded; no dataset is involved.

A third input is one plain [220 000, 4] tensor with flip_xy, the RELLIS-sized sample of tests/tools/bench_prep.py: the path that
runs efgh_prep_radius_filter / efgh_prep_gather_transform.

Method: inputs resident on the device, warm-up, then ROUNDS interleaved rounds (off, 0.1, 0.2, and the parent's off, 0.1, 0.2; every
round starts one further on) of CALLS calls each, every round closed by a device synchronise; per-call time of a round = round time /
CALLS.  Reported: the median over the rounds and their min .. max, the kept count, and the device time of the five thinning kernels
(table init / insert / flag count / block scan / compaction) from torch.profiler's kernel records of separate, untimed calls.

The gate: with `--parent DIR`, a checkout of the parent commit with its library built (git worktree add DIR HEAD~1 && (cd DIR &&
python -m efgh_amd.build)), the parent's own preproc_pcd runs every setting in the same rounds on the same resident input.  A setting
passes when its outputs equal the parent's bit for bit and its median lies inside the parent's min .. max of this run, or below it.

Not measured: sets of more than 7 sweeps, host-array inputs, any effect on training or on registration accuracy.

    python tools/bench_voxel.py [--parent DIR] [--out profiles/voxel.txt]
"""
import argparse
import importlib
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from efgh_amd.data import SweepSet, preproc_gt, preproc_pcd  # noqa: E402

ROUNDS, CALLS, WARM = 9, 40, 10
NUM_POINTS = 131072
# label, and the words a kernel's name holds: the voxel instances of the compaction templates (k_voxel_flag_count / k_voxel_compact
# in a checkout from before there was one compaction)
KERNELS = (('table init', (('k_voxel_init',),)), ('insert', (('k_voxel_insert',),)),
           ('flag count', (('k_flag_count', 'VoxelPred'), ('k_voxel_flag_count',))), ('block scan', (('k_scan_blocks',),)),
           ('compaction', (('k_compact', 'VoxelPred'), ('k_voxel_compact',))))


def make_scene(k, n_each, stride, seed, reach):
    """k sweeps of n_each points of one static scene (ground plane, walls at `reach` / 2), each in its own frame, + the 4x4s"""
    rng = np.random.default_rng(seed)
    sweeps, Ms = [], []
    for i in range(k):
        a = 0.01 * i
        M = np.eye(4)
        M[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        M[:3, 3] = (0.8 * i, 0.05 * i, 0.01 * i)
        r = rng.uniform(2.0, reach, n_each)
        th = rng.uniform(-np.pi, np.pi, n_each)
        w = np.stack([r * np.cos(th), r * np.sin(th), -1.7 + 0.02 * rng.standard_normal(n_each)], axis=1)
        wall = r > reach / 2                                  # what would lie behind a wall lands on it, at some height
        w[wall, 0], w[wall, 1] = (reach / 2) * np.cos(th[wall]), (reach / 2) * np.sin(th[wall])
        w[wall, 2] = rng.uniform(-1.7, 2.0, int(wall.sum()))
        w += M[:3, 3]                                         # the sensor stands at its pose in the frame of sweep 0
        p = np.zeros((n_each, stride), np.float32)
        p[:, :3] = (w - M[:3, 3]) @ M[:3, :3]                 # R^T (w - t): into the sweep's own frame
        if stride == 4:
            p[:, 3] = 0.5
        sweeps.append(p)
        if i:
            Ms.append(M)
    return sweeps, Ms


def load_parent(path):
    """the parent commit's efgh_amd.data.prepare under another package name, bound to its own library"""
    pkg = os.path.join(os.path.abspath(path), 'efgh_amd')
    if not os.path.exists(os.path.join(pkg, 'lib', 'libefgh_hip.so')):
        raise SystemExit('bench_voxel: %s has no built library (python -m efgh_amd.build in that checkout)' % path)
    spec = importlib.util.spec_from_file_location('efgh_parent', os.path.join(pkg, '__init__.py'), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules['efgh_parent'] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module('efgh_parent.data.prepare')


def rounds(fns):
    """interleaved rounds of the callables -> per-call milliseconds, one list per callable.  Every round starts one callable
    further on, so each stands at every place of the order equally often and none always runs behind the same neighbour"""
    for f in fns:
        for _ in range(WARM):
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for r in range(ROUNDS):
        for i in [(r + o) % len(fns) for o in range(len(fns))]:
            f = fns[i]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                f()
            torch.cuda.synchronize()
            ms[i].append((time.perf_counter() - t0) / CALLS * 1e3)
    return ms


def kernel_split(fn, calls=10):
    """mean device microseconds per call of the five thinning kernels, from the profiler's kernel records"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')]
    except Exception as e:                                    # (a profiler that cannot attach here: say so in the file)
        return 'n/a (%s)' % type(e).__name__
    out = []
    for label, names in KERNELS:
        us = [float(getattr(e, 'device_time', None) or getattr(e, 'cuda_time', 0.0)) for e in ev
              if any(all(w in e.name for w in words) for words in names)]
        if label == 'block scan':                             # the radius filter in front launches it too: every second record
            us = us[1::2]
        if not us:
            return 'n/a (no kernel records)'
        out.append('%s %.1f' % (label, sum(us) / calls))
    return ', '.join(out) + ' us'


def fmt(v):
    return '%.3f ms (%.3f .. %.3f)' % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='checkout of the parent commit with its library built')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'voxel.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_voxel: needs the GPU (there is no CPU path to time)')
    parent = load_parent(a.parent) if a.parent else None
    gts = preproc_gt(0.1, -0.05, 0.3, 0.2, 0.1, -0.3, 0.0)
    pgts = parent.preproc_gt(0.1, -0.05, 0.3, 0.2, 0.1, -0.3, 0.0) if parent else None
    sel = np.arange(NUM_POINTS)
    lines = ['preproc_pcd, %d points out, %s; %d interleaved rounds of %d calls, median (min .. max) per call'
             % (NUM_POINTS, torch.cuda.get_device_name(0), ROUNDS, CALLS)]
    verdicts = []

    def measure(settings, src, psrc):
        """settings: (label, keyword arguments).  -> per setting (ms of this checkout, ms of the parent or None, outputs identical or None);
        this checkout's and the parent's calls of every setting share the interleaved rounds"""
        fns = [lambda kw=kw: preproc_pcd(src, gts, NUM_POINTS, **kw) for _, kw in settings]
        same = [None] * len(settings)
        if parent is not None:
            fns += [lambda kw=kw: parent.preproc_pcd(psrc, pgts, NUM_POINTS, **kw) for _, kw in settings]
            same = [torch.equal(parent.preproc_pcd(psrc, pgts, NUM_POINTS, sampled_indices=sel, **kw).view(torch.int32),
                                preproc_pcd(src, gts, NUM_POINTS, sampled_indices=sel, **kw).view(torch.int32)) for _, kw in settings]
        ms = rounds(fns)
        k = len(settings)
        return fns, [(ms[i], ms[k + i] if parent is not None else None, same[i]) for i in range(k)]

    def gate(label, new, old, same):
        """the lines of one setting's comparison with the parent, and its verdict into `verdicts`"""
        if old is None:
            return ['  %s: parent commit not measured (no --parent checkout given)' % label]
        med, lo, hi = statistics.median(new), min(old), max(old)
        ok = med <= hi and same
        verdicts.append(ok)
        return ['  %s: parent commit, same input   %s   outputs bit-identical: %s' % (label, fmt(old), same),
                '  gate: %s median %.3f ms %s the parent\'s round-to-round spread %.3f .. %.3f ms (%.1f %% of its median)'
                % (label, med, 'lies inside' if lo <= med <= hi else ('lies BELOW' if med < lo else 'lies ABOVE'), lo, hi,
                   100 * (hi - lo) / statistics.median(old))]

    settings = (('voxel_size=None', {}), ('voxel_size=0.1', {'voxel_size': 0.1}), ('voxel_size=0.2', {'voxel_size': 0.2}))
    for label, k, n_each, stride, ego, reach in (('nuScenes-sized', 7, 34720, 3, (0.8, 2.7), 60.0),
                                                 ('KITTI-sized', 7, 120000, 4, (0.8, 2.7), 70.0)):
        sweeps, Ms = make_scene(k, n_each, stride, 5, reach)
        ss = SweepSet(sweeps, Ms, ego_box=ego)
        fns, res = measure(settings, ss, parent.SweepSet(sweeps, Ms, ego_box=ego) if parent else None)
        kept = [int(ss.kept_indices().numel())] + [int(ss.kept_indices(voxel_size=v).numel()) for v in (0.1, 0.2)]
        lines += ['',
                  '%s SweepSet: %d sweeps x %d points (row stride %d%s), %d of %d rows pass the ego box and the radius' % (
                      label, k, n_each, stride, ', ego box (%.1f, %.1f)' % ego if ego else '', kept[0], k * n_each),
                  '  voxel_size=None                 %s' % fmt(res[0][0])]
        for i, v in ((1, 0.1), (2, 0.2)):
            lines += ['  voxel_size=%.1f                  %s   %+.3f ms   %d rows kept (%.1f %%)%s'
                      % (v, fmt(res[i][0]), statistics.median(res[i][0]) - statistics.median(res[0][0]), kept[i],
                         100.0 * kept[i] / kept[0],
                         '' if kept[i] > NUM_POINTS else '   (fewer than the points out: zero-padded, no permutation is drawn)'),
                      '      kernels per call: %s' % kernel_split(fns[i])]
            if parent is not None:
                lines += ['      the parent\'s:     %s' % kernel_split(fns[len(settings) + i])]
        for (name, _), r in zip(settings, res):
            lines += gate(name, *r)
    # one plain [n, 4] array, the RELLIS-sized sample of tests/tools/bench_prep.py: 220 000 rows, x and y flipped
    rng = np.random.default_rng(0)
    n = 220000
    pcd = np.empty((n, 4), np.float32)
    pcd[:, :2], pcd[:, 2], pcd[:, 3] = rng.uniform(-60, 60, (n, 2)), rng.uniform(-3, 3, n), .5
    pcd = torch.from_numpy(pcd).cuda()
    _, res = measure((('flip_xy=True', {'flip_xy': True}),), pcd, pcd)
    lines += ['', 'plain [%d, 4] float32 tensor, flip_xy' % n, '  flip_xy=True                    %s' % fmt(res[0][0])]
    lines += gate('flip_xy=True', *res[0])
    lines += ['', 'not measured: sets of more than 7 sweeps, host-array inputs, any effect on training or on registration accuracy']
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)
    if verdicts and not all(verdicts):
        raise SystemExit('bench_voxel: a setting lies above the parent\'s spread, or its outputs differ from the parent\'s')


if __name__ == '__main__':
    main()
