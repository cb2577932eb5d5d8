"""What the differentiable score costs (efgh_amd.common.score_soft / refine: soft histogram, table, pose gradient, fold), against the
hard histogram of `score` on the same inputs in the same rounds - the yardstick: the same projection and the same LDS counters, one
nearest pixel and one LDS atomic a point where the soft kernel reads four pixels and issues two.

Per image size (900x1600 nuScenes, 376x1241 KITTI), K (1; 4; 729, a steps=1 grid on six axes) and bins (32, 64): 131 072 points of the
coherent synthetic sweep, the synthetic calibration and perturbations of it, a smooth image and uniform values, everything resident.
Timed in the same interleaved rounds (tools/bench_voxel.py's: warm-up, ROUNDS rounds of CALLS calls, a device synchronise around each,
median and min .. max per call):
  * efgh_score_hist alone (the yardstick) and efgh_score_soft_hist alone, on preallocated buffers;
  * the backward's three launches alone: efgh_score_soft_table + _grad + _fold;
  * `score(...)` of this tree and, with --parent DIR (a checkout of the parent commit with its library built), of the parent: the
    unchanged path must cost what it did, judged against the parent's own round-to-round spread.  The rounds keep every callable
    behind the same neighbour, so the two that are compared each run behind a `score` call on the same inputs;
and per bins, outside those rounds, `refine(..., iters=ITERS)` end to end divided by its iterations, with the share of that time in
which the device runs no kernel (1 - device time / wall time; the device time is the sum of torch.profiler's kernel records).
The device time of each kernel comes from the profiler's records of separate, untimed calls.

No target is set.  Not measured: pooled batches, float32 leaves, batches above 1, any effect on registration accuracy.

    python tools/bench_score_soft.py [--parent DIR] [--out profiles/score_soft.txt]
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
import bench_voxel as BV  # noqa: E402  (the interleaved rounds)
from efgh_amd import _C  # noqa: E402
from efgh_amd import synthetic as syn  # noqa: E402
from efgh_amd.common import refine, score  # noqa: E402

N = 131072
ITERS = 20
KERNELS = ('k_score_hist', 'k_soft_hist', 'k_soft_table', 'k_soft_grad', 'k_soft_fold')


def load_parent_score(path):
    BS.load_parent_fuse(path)                                    # imports the parent's efgh_amd.common under another name
    return sys.modules['efgh_parent.common.score'].score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_soft.txt'))
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: time its score(...) in the same rounds')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_score_soft: needs the GPU (there is no CPU path to time)')
    parent_score = load_parent_score(a.parent) if a.parent else None
    L, st = _C.lib(), _C.stream_ptr
    chunk = int(L.efgh_score_chunk())
    pc = torch.from_numpy(syn.coherent_sweep(N, 3)).cuda()[None].contiguous()
    n = pc.shape[2]
    n_chunk = -(-n // chunk)
    v = torch.from_numpy(np.random.RandomState(5).rand(1, n).astype(np.float32)).cuda()
    lines = ['score_soft on %d resident points, %s; chunk %d; %d interleaved rounds of %d calls, median (min .. max) per call'
             % (n, torch.cuda.get_device_name(0), chunk, BV.ROUNDS, BV.CALLS)]
    for h, w in BS.SIZES:
        calib, _ = syn.calib_and_A((h, w))
        img = torch.from_numpy(BS.smooth_image(h, w, h)).cuda()
        P = {K: BS.poses(calib, K) for K in BS.KS}
        buf = {}
        for K in BS.KS:
            for b in BS.BINS:
                i32, f64 = dict(dtype=torch.int32, device='cuda'), dict(dtype=torch.float64, device='cuda')
                buf[(K, b)] = dict(hard=torch.empty((1, K, b, b), **i32), hist=torch.empty((1, K, b, b), **i32), table=torch.empty((K, b, b), **f64),
                                   flag=torch.empty((K, b, b), dtype=torch.uint8, device='cuda'), tot=torch.empty((K,), **i32),
                                   part=torch.empty((1, K, n_chunk, 12), **f64), G=torch.empty((1, K, 12), **f64))

        def hard(K, b):
            _C.check(L.efgh_score_hist(_C.ptr(pc), pc.stride(0), pc.stride(1), 1, n, _C.ptr(v), v.stride(0), _C.ptr(P[K]), K, _C.ptr(img), h, w, b,
                                       0.0, 1.0, 0.0, _C.ptr(buf[(K, b)]['hard']), st()))

        def soft(K, b):
            _C.check(L.efgh_score_soft_hist(_C.ptr(pc), pc.stride(0), pc.stride(1), 1, n, _C.ptr(v), v.stride(0), _C.ptr(P[K]), K, _C.ptr(img), h,
                                            w, b, 0.0, 1.0, 0.0, 0, _C.ptr(buf[(K, b)]['hist']), st()))

        def back(K, b):
            B = buf[(K, b)]
            _C.check(L.efgh_score_soft_table(_C.ptr(B['hist']), K, b, _C.ptr(B['table']), _C.ptr(B['flag']), _C.ptr(B['tot']), st()))
            _C.check(L.efgh_score_soft_grad(_C.ptr(pc), pc.stride(0), pc.stride(1), 1, n, _C.ptr(v), v.stride(0), _C.ptr(P[K]), K, _C.ptr(img), h,
                                            w, b, 0.0, 1.0, 0.0, 0, _C.ptr(B['table']), _C.ptr(B['flag']), _C.ptr(B['tot']), _C.ptr(B['part']), st()))
            _C.check(L.efgh_score_soft_fold(_C.ptr(B['part']), 1, K, n_chunk, _C.ptr(B['G']), st()))

        cases = [(K, b) for K in BS.KS for b in BS.BINS]
        per = 6 if parent_score else 4
        fns = []
        for K, b in cases:
            soft(K, b)                                           # the histogram the backward's launches read
            fns += [lambda K=K, b=b: hard(K, b), lambda K=K, b=b: soft(K, b), lambda K=K, b=b: back(K, b),
                    lambda K=K, b=b: score(pc, img, P[K], value=v, bins=b)]
            if parent_score:
                # every callable runs behind the same neighbour in every round, so the pair is timed as parent, this tree: each behind
                # a `score` call on the same inputs (the call in front of the parent's is this tree's, reported on its own)
                fns += [lambda K=K, b=b: parent_score(pc, img, P[K], value=v, bins=b), lambda K=K, b=b: score(pc, img, P[K], value=v, bins=b)]
        ms = BV.rounds(fns)
        s0 = score(pc, img, P[1], value=v, bins=64)
        lines += ['', '%d x %d: %d of the points in frame under the unperturbed matrix' % (h, w, int(s0.count[0, 0]))]
        for j, (K, b) in enumerate(cases):
            m_hard, m_soft, m_back, m_score = ms[per * j:per * j + 4]
            us = BF.kernel_us(lambda: (hard(K, b), soft(K, b), back(K, b)), KERNELS)
            if isinstance(us, dict):
                g = [us.get(k, 0.0) for k in KERNELS]
                dev = ('kernels: hard hist %.1f us, soft hist %.1f us = %.2f x; table %.1f + grad %.1f + fold %.1f = %.1f us'
                       % (g[0], g[1], g[1] / g[0] if g[0] else float('nan'), g[2], g[3], g[4], g[2] + g[3] + g[4]))
            else:
                dev = 'kernels ' + us
            head = '  K %3d, %2d bins  ' % (K, b)
            lines += [head + 'efgh_score_hist (yardstick)    %s' % BV.fmt(m_hard),
                      head + 'efgh_score_soft_hist           %s   %s x the yardstick call' % (BV.fmt(m_soft), BF.ratio(m_soft, m_hard)),
                      head + 'table + grad + fold            %s   %.0f us' % (BV.fmt(m_back), 1e3 * statistics.median(m_back)),
                      head + dev]
            if parent_score:
                theirs, mine = ms[per * j + 4], ms[per * j + 5]
                inside = statistics.median(mine) <= max(theirs)
                lines += [head + 'score(...) behind the backward\'s launches: this tree %s' % BV.fmt(m_score),
                          head + "score(...) behind a score(...): this tree %s   the parent commit %s   ratio per round %s   this tree's median %s the "
                          "parent's round-to-round spread" % (BV.fmt(mine), BV.fmt(theirs), BF.ratio(mine, theirs), 'lies inside or below' if inside else 'lies ABOVE')]
            else:
                lines += [head + 'score(...): this tree %s' % BV.fmt(m_score)]
        T = P[1][:, 0].contiguous()
        for b in BS.BINS:
            run = lambda: refine(pc, img, T, value=v, bins=b, iters=ITERS)
            run()
            wall = []
            for _ in range(BV.ROUNDS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3 / ITERS)
            us = BF.kernel_us(run, ('',), calls=2)
            line = '  refine, %2d bins, per iteration of %d, end to end: %s' % (b, ITERS, BV.fmt(wall))
            if isinstance(us, dict):
                dev_ms = us[''] / ITERS / 1e3
                line += '   device kernels %.3f ms an iteration: the device is idle for %.0f %% of the time (host-bound)' \
                        % (dev_ms, 100.0 * (1.0 - dev_ms / statistics.median(wall)))
            else:
                line += '   device share ' + us
            lines.append(line)
    lines += ['', 'not measured: pooled batches, float32 leaves, batches above 1, any effect on registration accuracy']
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
