"""What scoring candidate poses costs (efgh_amd.common.score: joint histogram of value and grey level per candidate, then mutual
information), against the z-buffer launch of `fuse`, which runs the same projection with one atomic per in-frame point.

Per image size (900x1600 nuScenes, 376x1241 KITTI), K (1; 4, the stages; 729, a steps=1 grid on six axes) and bins (32, 64): 131 072
points of the coherent synthetic sweep, the synthetic calibration and perturbations of it (0.2 degrees, 5 cm a step), everything
resident on the device.  Timed in the same interleaved rounds:
  * `score(...)`: the whole call, allocations and the float64 copy of the matrices included;
  * the two entry points alone on preallocated buffers (efgh_score_hist + efgh_score_mi);
  * the yardstick: `efgh_fuse_zbuffer` at radius 0 on the same cloud and the unperturbed matrix, preallocated too.
Method: tools/bench_voxel.py's rounds (warm-up, ROUNDS interleaved rounds of CALLS calls, a device synchronise around each, median and
min .. max per call).  The device time of each kernel comes from torch.profiler's kernel records of separate, untimed calls; the memsets
in front of the histogram and of the z-buffer are in the call times and not in the kernel times.

Two inputs, because same-address LDS atomics are the likely cost of the histogram kernel: PILED (a smooth image and a reflectance
that sits in a tenth of its range: nearly every point of a wave adds to one of a few cells) and SPREAD (a random image and uniform
values: the adds of a wave scatter over the whole histogram).  The projection and the counts of in-frame points are the same in both.

No ratio is fixed in advance.  The chunk (points a workgroup counts in LDS before it flushes) is a build constant; to compare:

    EFGH_BUILD_FLAGS=-DEFGH_SCORE_CHUNK=16384 EFGH_BUILD_DIR=lib_ab python -m efgh_amd.build
    EFGH_LIB=efgh_amd/lib_ab/libefgh_hip.so python tools/bench_score.py --quick --append --label 'chunk 16384'

--parent DIR (a checkout of the parent commit with its library built) adds `fuse(...)` of both trees in the same rounds: fuse.hip
takes its projection from a header it now shares with score.hip, and must cost what it did.

Not measured: any effect on registration accuracy (there is no dataset here), K beyond 729, batches above 1, host-array inputs.

    python tools/bench_score.py [--out profiles/score.txt]
"""
import argparse
import importlib
import importlib.util
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_fuse as BF  # noqa: E402  (kernel_us, ratio)
import bench_voxel as BV  # noqa: E402  (the interleaved rounds)
from efgh_amd import _C  # noqa: E402
from efgh_amd import synthetic as syn  # noqa: E402
from efgh_amd.common import candidates_around, fuse, score  # noqa: E402

SIZES = ((900, 1600), (376, 1241))
KS = (1, 4, 729)
BINS = (32, 64)
N = 131072
KERNELS = ('k_score_hist', 'k_score_mi')


def smooth_image(h, w, seed):
    """uint8 (1,h,w,3): a few low-frequency waves around a mid grey, +-2 levels of noise"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = 110 + 40 * np.sin(x / w * 5.0 + 1.0) * np.cos(y / h * 3.0) + 2 * rs.randn(h, w)
    return np.repeat(np.clip(a, 0, 255).astype(np.uint8)[None, :, :, None], 3, 3)


def poses(calib, K):
    P = torch.from_numpy(np.ascontiguousarray(calib[None])).cuda()
    if K == 1:
        return P[:, None].contiguous()
    if K == 4:
        return candidates_around(P, (0.2, 0, 0), (0.05, 0, 0), steps=1)[:, :4].contiguous()
    return candidates_around(P, (0.2, 0.2, 0.2), (0.05, 0.05, 0.05), steps=1)


def load_parent_fuse(path):
    """the parent commit's efgh_amd.common.fuse under another package name, bound to its own library"""
    pkg = os.path.join(os.path.abspath(path), 'efgh_amd')
    if not os.path.exists(os.path.join(pkg, 'lib', 'libefgh_hip.so')):
        raise SystemExit('bench_score: %s has no built library (python -m efgh_amd.build in that checkout)' % path)
    spec = importlib.util.spec_from_file_location('efgh_parent', os.path.join(pkg, '__init__.py'), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules['efgh_parent'] = mod
    spec.loader.exec_module(mod)
    importlib.import_module('efgh_parent.common')
    return sys.modules['efgh_parent.common.fuse'].fuse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score.txt'))
    ap.add_argument('--label', default=None, help='what is special about the library measured (EFGH_LIB selects an A/B build)')
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    ap.add_argument('--quick', action='store_true', help='the first image size, K = 1 and 729, 64 bins: for A/B builds of the chunk')
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: time its fuse(...) in the same rounds')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_score: needs the GPU (there is no CPU path to time)')
    L, st = _C.lib(), _C.stream_ptr
    chunk = int(L.efgh_score_chunk())
    pc = torch.from_numpy(syn.coherent_sweep(N, 3)).cuda()[None].contiguous()
    n = pc.shape[2]
    rs = np.random.RandomState(5)
    values = {'piled': torch.from_numpy(np.clip(0.12 + 0.025 * rs.randn(1, n), 0, 1).astype(np.float32)).cuda(),
              'spread': torch.from_numpy(rs.rand(1, n).astype(np.float32)).cuda()}
    lines = ['score on %d resident points, %s; chunk %d; %d interleaved rounds of %d calls, median (min .. max) per call'
             % (n, torch.cuda.get_device_name(0), chunk, BV.ROUNDS, BV.CALLS)]
    if a.label:
        lines = ['', '=== ' + a.label + ' ==='] + lines
    sizes, ks, binss = (SIZES[:1], (1, 729), (64,)) if a.quick else (SIZES, KS, BINS)
    for h, w in sizes:
        calib, _ = syn.calib_and_A((h, w))
        T = torch.from_numpy(np.ascontiguousarray(calib[None])).cuda()
        imgs = {'piled': torch.from_numpy(smooth_image(h, w, h)).cuda(),
                'spread': torch.from_numpy(np.random.default_rng(h).integers(0, 256, (1, h, w, 3), dtype=np.uint8)).cuda()}
        zbuf = torch.empty(h * w, dtype=torch.int64, device='cuda')
        P = {K: poses(calib, K) for K in ks}
        hist = {(K, b): torch.empty((1, K, b, b), dtype=torch.int32, device='cuda') for K in ks for b in binss}
        out = {K: torch.empty((1, K, 5), dtype=torch.float64, device='cuda') for K in ks}
        cnt = {K: torch.empty((1, K), dtype=torch.int32, device='cuda') for K in ks}

        def yard():
            _C.check(L.efgh_fuse_zbuffer(_C.ptr(pc), pc.stride(0), pc.stride(1), 1, n, _C.ptr(T), h, w, 0, 0.0, _C.ptr(zbuf), st()))

        def launches(K, b, kind):
            v, im = values[kind], imgs[kind]
            _C.check(L.efgh_score_hist(_C.ptr(pc), pc.stride(0), pc.stride(1), 1, n, _C.ptr(v), v.stride(0), _C.ptr(P[K]), K, _C.ptr(im), h, w,
                                       b, 0.0, 1.0, 0.0, _C.ptr(hist[(K, b)]), st()))
            _C.check(L.efgh_score_mi(_C.ptr(hist[(K, b)]), 1, K, b, _C.ptr(out[K]), _C.ptr(cnt[K]), st()))

        cases = [(K, b, kind) for K in ks for b in binss for kind in ('piled', 'spread')]
        fns = [yard]
        for K, b, kind in cases:
            fns += [lambda K=K, b=b, kind=kind: launches(K, b, kind),
                    lambda K=K, b=b, kind=kind: score(pc, imgs[kind], P[K], value=values[kind], bins=b)]
        ms = BV.rounds(fns)
        us_yard = BF.kernel_us(yard, ('k_fuse_zbuffer',))
        yk = us_yard.get('k_fuse_zbuffer') if isinstance(us_yard, dict) else None
        s0 = score(pc, imgs['piled'], P[ks[-1]], value=values['piled'], bins=binss[-1], want_hist=True)
        lines += ['', '%d x %d: %d of the points in frame under the unperturbed matrix (candidates of K = %d: %d .. %d); non-zero cells of '
                  'its %d x %d histogram: piled %d, spread %d'
                  % (h, w, int(s0.count[0, 0]), ks[-1], int(s0.count.min()), int(s0.count.max()), binss[-1], binss[-1], int((s0.hist[0, 0] > 0).sum()),
                     int((score(pc, imgs['spread'], P[ks[0]], value=values['spread'], bins=binss[-1], want_hist=True).hist[0, 0] > 0).sum())),
                  '  %-44s %s   kernel %s' % ('efgh_fuse_zbuffer, radius 0 (yardstick)', BV.fmt(ms[0]), '%.1f us' % yk if yk else us_yard)]
        for j, (K, b, kind) in enumerate(cases):
            raw_ms, call_ms = ms[1 + 2 * j], ms[2 + 2 * j]
            us = BF.kernel_us(lambda: launches(K, b, kind), KERNELS)
            if isinstance(us, dict):
                hk, mk = us.get('k_score_hist', 0.0), us.get('k_score_mi', 0.0)
                dev = 'kernels hist %.1f + mi %.1f us; hist per candidate %.2f us' % (hk, mk, hk / K)
                if yk:
                    dev += ' = %.2f x the yardstick kernel' % (hk / K / yk)
            else:
                dev = 'kernels ' + us
            lines += ['  K %3d, %2d bins, %-6s two launches         %s   %.4f ms a candidate   %s'
                      % (K, b, kind, BV.fmt(raw_ms), statistics.median(raw_ms) / K, dev),
                      '  K %3d, %2d bins, %-6s score(...)           %s   %.4f ms a candidate   %s x the yardstick call'
                      % (K, b, kind, BV.fmt(call_ms), statistics.median(call_ms) / K, BF.ratio(call_ms, ms[0]))]
        if a.parent:
            parent_fuse = load_parent_fuse(a.parent)
            img = imgs['spread']
            fns = [f for r in (0, 2) for f in (lambda r=r: fuse(pc, img, T, radius=r, rel_tol=0.05), lambda r=r: parent_fuse(pc, img, T, radius=r, rel_tol=0.05))]
            pm = BV.rounds(fns)
            for j, r in enumerate((0, 2)):
                mine, theirs = pm[2 * j], pm[2 * j + 1]
                inside = min(theirs) <= statistics.median(mine) <= max(theirs)
                lines += ['  fuse(...), radius %d, every output: this tree %s   the parent commit %s   ratio per round %s   this tree\'s median %s '
                          'the parent\'s round-to-round spread' % (r, BV.fmt(mine), BV.fmt(theirs), BF.ratio(mine, theirs),
                                                                  'lies inside' if inside else 'lies OUTSIDE')]
    lines += ['', 'not measured: any effect on registration accuracy, K beyond 729, batches above 1, host-array inputs (the upload)']
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a' if a.append else 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
