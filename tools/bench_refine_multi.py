"""What climbing from many starts costs (efgh_amd.common.refine_multi / search: csrc/refine.hip behind the unchanged scoring kernels),
against `refine` - the yardstick: one start a sample, about forty small torch launches an iteration between two scorings.

Per image size (900x1600 nuScenes, 376x1241 KITTI), 32 bins: 131 072 points of the coherent synthetic sweep, the synthetic calibration
and perturbations of it, a smooth image and uniform values, everything resident, B = 1.  Timed in the same interleaved rounds
(tools/bench_voxel.py's order: every round starts one callable further on; ROUNDS rounds of CALLS calls, a device synchronise around
each, median and min .. max), every call ITERS iterations long and reported PER ITERATION:
  * `refine` of the parent commit (--parent DIR, a checkout with its library built): the yardstick, wall time and device time;
  * `refine` of this tree: unchanged, so it must give the parent's bits and lie inside the parent's own round-to-round spread;
  * `refine_multi` at S = 1, 8 and 64 starts (perturbations of the calibration);
  * `search` on the K = 729 grid with keep = 8 (per call, and per iteration of its climb);
  * `score_soft` with its backward, K = 1, of the parent and of this tree (per call).
The device time is the sum of torch.profiler's kernel records of separate, untimed calls; the two new kernels' own times come from
the same records.  No ratio is fixed in advance: the file says what was measured, the parent's spread, and where S = 1 lands.

Not measured: pooled batches, batches above 1, float32 starts, 64 bins, a visible-points scorer, any effect on registration accuracy.

    python tools/bench_refine_multi.py [--parent DIR] [--out profiles/refine_multi.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_fuse as BF  # noqa: E402  (kernel_us, ratio)
import bench_score as BS  # noqa: E402  (the sizes, the image, the poses, the parent's package)
import bench_voxel as BV  # noqa: E402  (fmt)
from efgh_amd import synthetic as syn  # noqa: E402
from efgh_amd.common import candidates_around, refine, refine_multi, score_soft, search  # noqa: E402

N = 131072
ITERS = 20
BINS = 32
ROUNDS, CALLS, WARM = 9, 10, 2                    # a call is ITERS iterations: a round times 200 of them
STARTS = (1, 8, 64)
GRID = dict(rot_deg=(0.2, 0.2, 0.2), trans=(0.05, 0.05, 0.05), steps=1)      # bench_score's K = 729


def rounds(fns):
    """bench_voxel.rounds with this file's ROUNDS, CALLS and WARM -> per-call milliseconds, one list per callable"""
    for f in fns:
        for _ in range(WARM):
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for r in range(ROUNDS):
        for i in [(r + o) % len(fns) for o in range(len(fns))]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fns[i]()
            torch.cuda.synchronize()
            ms[i].append((time.perf_counter() - t0) / CALLS * 1e3)
    return ms


def device_ms(fn):
    us = BF.kernel_us(fn, ('', 'k_refine_step', 'k_refine_select'), calls=2)
    return us if isinstance(us, dict) else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'refine_multi.txt'))
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: its refine and score_soft in the same rounds')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_refine_multi: needs the GPU (there is no CPU path to time)')
    parent = None
    if a.parent:
        BS.load_parent_fuse(a.parent)                            # imports the parent's efgh_amd.common under another name
        parent = sys.modules['efgh_parent.common.score_soft']
    pc = torch.from_numpy(syn.coherent_sweep(N, 3)).cuda()[None].contiguous()
    n = pc.shape[2]
    v = torch.from_numpy(np.random.RandomState(5).rand(1, n).astype(np.float32)).cuda()
    lines = ['refine_multi / search on %d resident points, %s; %d bins, B = 1; %d interleaved rounds of %d calls of %d iterations, median '
             '(min .. max) PER ITERATION unless it says per call' % (n, torch.cuda.get_device_name(0), BINS, ROUNDS, CALLS, ITERS)]
    for h, w in BS.SIZES:
        calib, _ = syn.calib_and_A((h, w))
        img = torch.from_numpy(BS.smooth_image(h, w, h)).cuda()
        T = BS.poses(calib, 1)[:, 0].contiguous()                # (1,3,4)
        around = candidates_around(T, **GRID)
        kw = dict(value=v, bins=BINS)
        names, fns = [], []

        def add(name, fn):
            names.append(name)
            fns.append(fn)
        if parent:
            add('parent refine', lambda: parent.refine(pc, img, T, iters=ITERS, **kw))
        add('refine', lambda: refine(pc, img, T, iters=ITERS, **kw))
        first = {S: around[:, :S].contiguous() for S in STARTS}  # (sliced once, outside the timed calls)
        for S in STARTS:
            add('refine_multi S=%d' % S, lambda S=S: refine_multi(pc, img, first[S], iters=ITERS, **kw))
        add('search', lambda: search(pc, img, T, keep=8, iters=ITERS, **GRID, **kw))

        def soft(fn):
            P = T.clone().requires_grad_()
            fn(pc, img, P, **kw).mi.sum().backward()
            return P.grad
        if parent:
            add('parent score_soft', lambda: soft(parent.score_soft))
        add('score_soft', lambda: soft(score_soft))
        ms = dict(zip(names, rounds(fns)))
        lines += ['', '%d x %d' % (h, w)]
        per_it = lambda m: [x / ITERS for x in m]
        for name, fn in zip(names, fns):
            call = 'score_soft' in name
            m = ms[name] if call else per_it(ms[name])
            line = '  %-20s %s%s' % (name, BV.fmt(m), ' per call (forward + backward, K = 1)' if call else '')
            us = device_ms(fn)
            if us:
                dev = us[''] / 1e3 / (1 if call else ITERS)
                line += '   device kernels %.3f ms: idle %.0f %% of the wall time' % (dev, 100.0 * (1.0 - dev / statistics.median(m)))
                if 'k_refine_step' in us:
                    line += '; k_refine_step %.1f us a launch' % (us['k_refine_step'] / ITERS)
                if 'k_refine_select' in us:
                    line += ', k_refine_select %.1f us a launch (K = 729, keep 8)' % us['k_refine_select']
            lines.append(line)
            if name.startswith('refine_multi'):
                S = int(name.split('=')[1])
                lines.append('  %-20s per start and iteration %.3f ms; %s x refine per iteration in the same rounds'
                             % ('', statistics.median(m) / S, BF.ratio(ms[name], ms['refine'])))
            if name == 'search':
                lines.append('  %-20s per call %s: the grid of 729, the selection, %d iterations from 8 starts' % ('', BV.fmt(ms[name]), ITERS))
        if parent:
            theirs, mine, one = per_it(ms['parent refine']), per_it(ms['refine']), per_it(ms['refine_multi S=1'])
            rp, rm = parent.refine(pc, img, T, iters=ITERS, **kw), refine(pc, img, T, iters=ITERS, **kw)
            same = all(torch.equal(getattr(rp, k), getattr(rm, k)) for k in rm.__slots__)
            lines.append("  refine against the parent commit: bit-identical %s; ratio per round %s; this tree's median %s the parent's round-to-round "
                         'spread' % ('yes' if same else 'NO', BF.ratio(mine, theirs),
                                     'lies inside or below' if statistics.median(mine) <= max(theirs) else 'lies ABOVE'))
            gp, gm = soft(parent.score_soft), soft(score_soft)
            lines.append("  score_soft against the parent commit: gradient bit-identical %s; ratio per round %s; this tree's median %s the parent's "
                         'round-to-round spread' % ('yes' if torch.equal(gp, gm) else 'NO', BF.ratio(ms['score_soft'], ms['parent score_soft']),
                                                    'lies inside or below' if statistics.median(ms['score_soft']) <= max(ms['parent score_soft']) else 'lies ABOVE'))
            lines.append("  refine_multi at S = 1 against the parent's refine: ratio per round %s; the parent's spread is %.3f .. %.3f ms, S = 1 has its "
                         'median at %.3f ms: %s it' % (BF.ratio(one, theirs), min(theirs), max(theirs), statistics.median(one),
                                                       'below' if statistics.median(one) < min(theirs) else ('inside' if statistics.median(one) <= max(theirs) else 'ABOVE')))
    lines += ['', 'not measured: pooled batches, batches above 1, float32 starts, 64 bins, a visible-points scorer, any effect on registration accuracy']
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
