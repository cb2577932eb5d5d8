"""What scoring on visible points costs (efgh_amd.common.score_vis: a coarse z-buffer per candidate, the mask, the masked histogram,
the occupancy counts), against the unchanged hard histogram of `score` on the same inputs in the same rounds - the yardstick: the
same projection and grid, one LDS atomic a point where the zmin kernel issues one GLOBAL atomic a point.

Per image size (900x1600 nuScenes, 376x1241 KITTI), K (1; 4; 729, a steps=1 grid on six axes) and cell (8; (8, 2)): 131 072 points of
the coherent synthetic sweep, the synthetic calibration and perturbations of it, a smooth image and uniform values, 32 bins, a
tolerance of 2 % + 0.1 m, everything resident.  Timed in the same interleaved rounds (tools/bench_voxel.py's: warm-up, ROUNDS rounds of
CALLS calls, a device synchronise around each, median and min .. max per call):
  * efgh_score_hist alone (the yardstick), on preallocated buffers;
  * efgh_score_zmin, efgh_score_visible, efgh_score_hist_masked and efgh_score_occupancy, each alone on preallocated buffers;
  * `score_visible(...)`, the whole call;
  * with --parent DIR (a checkout of the parent commit with its library built): `score(...)` and `score_soft(...)` (forward and
    backward) of this tree and of the parent, each behind a call of the same kind on the same inputs: score.hip and score_soft.hip
    now hold one templated body for the plain and the masked kernels, and the plain path must cost what it did, judged against the
    parent's own round-to-round spread.
The device time of each kernel comes from torch.profiler's kernel records of separate, untimed calls; the fill in front of the zmin
kernel and the zeroing in front of the histogram are in the call times and not in the kernel times.  Atomics per ns of the zmin kernel:
the in-frame points of all candidates (one atomic each) over the kernel's device time.

No ratio is fixed in advance.  Not measured: pooled batches, the soft masked kernels, batches above 1, tolerances other than the one
above, any effect on registration accuracy (there is no dataset here).

    python tools/bench_score_vis.py [--parent DIR] [--out profiles/score_vis.txt]
"""
import argparse
import os
import statistics
import sys

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
from efgh_amd.common import Occlusion, score, score_soft, score_visible  # noqa: E402

N = 131072
BINS = 32
CELLS = ((8, 8), (8, 2))
REL, ABS = 0.02, 0.1
KERNELS = ('k_score_zmin', 'k_score_visible', 'k_score_hist', 'k_score_occ')      # of the four new calls; the yardstick is profiled apart


def load_parent(path):
    BS.load_parent_fuse(path)                                    # imports the parent's efgh_amd.common under another name
    return sys.modules['efgh_parent.common.score'].score, sys.modules['efgh_parent.common.score_soft'].score_soft


def soft_step(fn, pc, img, P, v):
    T = P.clone().requires_grad_()
    fn(pc, img, T, value=v, bins=BINS).mi.sum().backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_vis.txt'))
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: time its score(...) and score_soft(...) in the same rounds')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_score_vis: needs the GPU (there is no CPU path to time)')
    parent = load_parent(a.parent) if a.parent else None
    L, st = _C.lib(), _C.stream_ptr
    pc = torch.from_numpy(syn.coherent_sweep(N, 3)).cuda()[None].contiguous()
    n = pc.shape[2]
    v = torch.from_numpy(np.random.RandomState(5).rand(1, n).astype(np.float32)).cuda()
    lines = ['score_visible on %d resident points, %s; chunk %d; %d bins; visible iff d <= zmin (1 + %g) + %g; %d interleaved rounds of %d '
             'calls, median (min .. max) per call' % (n, torch.cuda.get_device_name(0), int(L.efgh_score_chunk()), BINS, REL, ABS, BV.ROUNDS, BV.CALLS)]
    i32 = dict(dtype=torch.int32, device='cuda')
    for h, w in BS.SIZES:
        calib, _ = syn.calib_and_A((h, w))
        img = torch.from_numpy(BS.smooth_image(h, w, h)).cuda()
        P = {K: BS.poses(calib, K) for K in BS.KS}
        buf = {}
        for K in BS.KS:
            for c in CELLS:
                Hc, Wc = -(-h // c[0]), -(-w // c[1])
                buf[(K, c)] = dict(hard=torch.empty((1, K, BINS, BINS), **i32), hist=torch.empty((1, K, BINS, BINS), **i32),
                                   zmin=torch.empty((1, K, Hc, Wc), **i32), mask=torch.empty((1, K, -(-n // 32)), **i32), occ=torch.empty((1, K, 3), **i32))

        def head(K, c):
            return (_C.ptr(pc), pc.stride(0), pc.stride(1), 1, n, _C.ptr(P[K]), K, h, w, c[0], c[1], 0.0)

        def points(K):
            return (_C.ptr(pc), pc.stride(0), pc.stride(1), 1, n, _C.ptr(v), v.stride(0), _C.ptr(P[K]), K, _C.ptr(img), h, w, BINS, 0.0, 1.0, 0.0)

        def hard(K, c):
            _C.check(L.efgh_score_hist(*points(K), _C.ptr(buf[(K, c)]['hard']), st()))

        def zmin(K, c):
            _C.check(L.efgh_score_zmin(*head(K, c), _C.ptr(buf[(K, c)]['zmin']), st()))

        def visible(K, c):
            _C.check(L.efgh_score_visible(*head(K, c), REL, ABS, _C.ptr(buf[(K, c)]['zmin']), _C.ptr(buf[(K, c)]['mask']), st()))

        def masked(K, c):
            _C.check(L.efgh_score_hist_masked(*points(K), _C.ptr(buf[(K, c)]['mask']), _C.ptr(buf[(K, c)]['hist']), st()))

        def occ(K, c):
            _C.check(L.efgh_score_occupancy(_C.ptr(buf[(K, c)]['hist']), K, BINS, _C.ptr(buf[(K, c)]['occ']), st()))

        cases = [(K, c) for K in BS.KS for c in CELLS]
        fns = []
        for K, c in cases:
            for f in (zmin, visible, masked, occ):               # what the later launches read is there before the rounds start
                f(K, c)
            o = Occlusion(c, REL, ABS)
            fns += [lambda K=K, c=c: hard(K, c), lambda K=K, c=c: zmin(K, c), lambda K=K, c=c: visible(K, c), lambda K=K, c=c: masked(K, c),
                    lambda K=K, c=c: occ(K, c), lambda K=K, o=o: score_visible(pc, img, P[K], occlusion=o, value=v, bins=BINS)]
        ms = BV.rounds(fns)
        s0 = score(pc, img, P[1], value=v, bins=BINS)
        lines += ['', '%d x %d: %d of the points in frame under the unperturbed matrix' % (h, w, int(s0.count[0, 0]))]
        for j, (K, c) in enumerate(cases):
            m_hard, m_z, m_v, m_m, m_o, m_call = ms[6 * j:6 * j + 6]
            sv = score_visible(pc, img, P[K], occlusion=Occlusion(c, REL, ABS), value=v, bins=BINS)
            frame = int(score(pc, img, P[K], value=v, bins=BINS).count.sum())
            # (the plain and the masked histogram are two instances of one kernel name: two profiles)
            us0 = BF.kernel_us(lambda: hard(K, c), ('k_score_hist',))
            us = BF.kernel_us(lambda: (zmin(K, c), visible(K, c), masked(K, c), occ(K, c)), KERNELS)
            head_ = '  K %3d, cell %d x %d  ' % (K, c[0], c[1])
            total = [p + q + r + s for p, q, r, s in zip(m_z, m_v, m_m, m_o)]
            lines += [head_ + '%d in frame over the candidates, %d visible; zmin workspace %d bytes' % (frame, int(sv.count.sum()), 4 * buf[(K, c)]['zmin'].numel()),
                      head_ + 'efgh_score_hist (yardstick)    %s' % BV.fmt(m_hard),
                      head_ + 'efgh_score_zmin                %s' % BV.fmt(m_z),
                      head_ + 'efgh_score_visible             %s' % BV.fmt(m_v),
                      head_ + 'efgh_score_hist_masked         %s' % BV.fmt(m_m),
                      head_ + 'efgh_score_occupancy           %s' % BV.fmt(m_o),
                      head_ + 'the four calls together        %s   %s x the yardstick call' % (BV.fmt(total), BF.ratio(total, m_hard)),
                      head_ + 'score_visible(...)             %s' % BV.fmt(m_call)]
            if isinstance(us, dict) and isinstance(us0, dict):
                g = [us0.get('k_score_hist', 0.0)] + [us.get(k, 0.0) for k in KERNELS]
                four = sum(g[1:])
                lines += [head_ + 'kernels: hist (yardstick) %.1f us; zmin %.1f + visible %.1f + masked hist %.1f + occupancy %.1f = %.1f us = %.2f x the '
                          'yardstick kernel; zmin: %.1f atomics per ns' % (g[0], g[1], g[2], g[3], g[4], four, four / g[0] if g[0] else float('nan'),
                                                                           frame / (g[1] * 1e3) if g[1] else float('nan'))]
            else:
                lines += [head_ + 'kernels ' + str(us if not isinstance(us, dict) else us0)]
        if parent:
            p_score, p_soft = parent
            for K in BS.KS:
                fns = [lambda K=K: p_score(pc, img, P[K], value=v, bins=BINS), lambda K=K: score(pc, img, P[K], value=v, bins=BINS),
                       lambda K=K: soft_step(p_soft, pc, img, P[K], v), lambda K=K: soft_step(score_soft, pc, img, P[K], v)]
                # twice over: every callable that is compared runs behind a call of its own kind on the same inputs
                pm = BV.rounds(fns[:2] + fns[:2] + fns[2:] + fns[2:])
                for name, theirs, mine in (('score(...)', pm[2], pm[3]), ('score_soft(...) forward + backward', pm[6], pm[7])):
                    inside = statistics.median(mine) <= max(theirs)
                    lines += ["  K %3d  %s: this tree %s   the parent commit %s   ratio per round %s   this tree's median %s the parent's "
                              'round-to-round spread' % (K, name, BV.fmt(mine), BV.fmt(theirs), BF.ratio(mine, theirs),
                                                         'lies inside or below' if inside else 'lies ABOVE')]
    lines += ['', 'not measured: pooled batches, the soft masked kernels, batches above 1, other tolerances, any effect on registration accuracy']
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
