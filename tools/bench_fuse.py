"""What fusing a registered pair costs (efgh_amd.common.fuse: z-buffer, visibility, point colours), against the raster the project
already has.

Per image size (900x1600 nuScenes, 376x1241 KITTI) and radius (0, 2): 131 072 points of the coherent synthetic sweep (ground plane
and walls, all around the sensor: about a fifth of it falls into the frame), a pinhole matrix centred on the image, a random uint8
image, everything resident on the device.  Timed in the same interleaved rounds:
  * `fuse(...)` with every output: the whole call, allocations and the float64 copy of the matrix included;
  * the three entry points alone on preallocated buffers (efgh_fuse_zbuffer + efgh_fuse_resolve + efgh_fuse_maps);
  * the yardstick: `efgh_sum_depth_last` on the same cloud and matrix, preallocated too - the existing two-launch "last point wins"
    raster with a 32-bit atomicMax.
Method: tools/bench_voxel.py's rounds (warm-up, ROUNDS interleaved rounds of CALLS calls, a device synchronise around each, median and
min .. max per call).  The device time of each kernel comes from torch.profiler's kernel records of separate, untimed calls; the
memsets in front of the z-buffer and of the yardstick's index plane are in the call times and not in the kernel times.

No ratio is fixed in advance.  If the z-buffer kernel at radius 2 costs more than about 25 x radius 0 (the count of atomics), the
per-kernel lines say where the time goes.  The A/B of the z-buffer's inner loop (a plain load in front of every atomic):

    EFGH_BUILD_FLAGS=-DEFGH_FUSE_PEEK=1 EFGH_BUILD_DIR=lib_peek python -m efgh_amd.build
    python tools/bench_fuse.py && EFGH_LIB=efgh_amd/lib_peek/libefgh_hip.so python tools/bench_fuse.py --append --label 'built with -DEFGH_FUSE_PEEK=1'

Not measured: host-array inputs (the upload), clouds with other overlap statistics than this sweep, any effect on anything downstream
(there is no dataset here).

    python tools/bench_fuse.py [--out profiles/fuse.txt]
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

import bench_voxel as BV  # noqa: E402  (the interleaved rounds)
from efgh_amd import _C  # noqa: E402
from efgh_amd import synthetic as syn  # noqa: E402
from efgh_amd.common import fuse  # noqa: E402

SIZES = ((900, 1600), (376, 1241))
RADII = (0, 2)
N = 131072
FUSE_KERNELS = ('k_fuse_zbuffer', 'k_fuse_resolve', 'k_fuse_maps')
LAST_KERNELS = ('k_depth_last1', 'k_depth_last2')


def kernel_us(fn, names, calls=10):
    """{kernel: mean device microseconds per call}, or a string saying why there is none"""
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
    out = {}
    for k in names:
        us = [float(getattr(e, 'device_time', None) or getattr(e, 'cuda_time', 0.0)) for e in ev if k in e.name]
        if us:
            out[k] = sum(us) / calls
    return out or 'n/a (no kernel records)'


def ratio(a, b):
    """median of the per-round ratios and their min .. max (both lists come from the same rounds)"""
    r = [x / y for x, y in zip(a, b)]
    return '%.2f (%.2f .. %.2f)' % (statistics.median(r), min(r), max(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fuse.txt'))
    ap.add_argument('--label', default=None, help='what is special about the library measured (EFGH_LIB selects an A/B build)')
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_fuse: needs the GPU (there is no CPU path to time)')
    L, st = _C.lib(), _C.stream_ptr
    pc = torch.from_numpy(syn.coherent_sweep(N, 3)).cuda()[None].contiguous()
    n = pc.shape[2]
    lines = ['fuse on %d resident points, %s; %d interleaved rounds of %d calls, median (min .. max) per call'
             % (n, torch.cuda.get_device_name(0), BV.ROUNDS, BV.CALLS)]
    if a.label:
        lines = ['', '=== ' + a.label + ' ==='] + lines
    for h, w in SIZES:
        calib, _ = syn.calib_and_A((h, w))
        T = torch.from_numpy(np.ascontiguousarray(calib[None])).cuda()
        img = torch.from_numpy(np.random.default_rng(h).integers(0, 256, (1, h, w, 3), dtype=np.uint8)).cuda()
        zbuf = torch.empty(h * w, dtype=torch.int64, device='cuda')
        state, rgb = torch.empty((1, n), dtype=torch.uint8, device='cuda'), torch.empty((1, n, 3), dtype=torch.uint8, device='cuda')
        uv = torch.empty((1, n, 2), dtype=torch.float32, device='cuda')
        depth, index = torch.empty((1, h, w), dtype=torch.float32, device='cuda'), torch.empty((1, h, w), dtype=torch.int32, device='cuda')
        ws, out8 = torch.empty(h * w, dtype=torch.int32, device='cuda'), torch.empty((h, w), dtype=torch.uint8, device='cuda')

        def launches(radius):
            _C.check(L.efgh_fuse_zbuffer(_C.ptr(pc), pc.stride(0), pc.stride(1), 1, n, _C.ptr(T), h, w, radius, 0.0, _C.ptr(zbuf), st()))
            _C.check(L.efgh_fuse_resolve(_C.ptr(pc), pc.stride(0), pc.stride(1), 1, n, _C.ptr(T), _C.ptr(img), h, w, 1, 0.0, 0.05, 0.0,
                                         _C.ptr(zbuf), _C.ptr(state), _C.ptr(rgb), _C.ptr(uv), st()))
            _C.check(L.efgh_fuse_maps(_C.ptr(zbuf), 1, h * w, _C.ptr(depth), _C.ptr(index), st()))

        def last():
            _C.check(L.efgh_sum_depth_last(_C.ptr(pc), pc.stride(1), n, _C.ptr(T), h, w, _C.ptr(ws), _C.ptr(out8), st()))

        fns = [last]
        for r in RADII:
            fns += [lambda r=r: launches(r), lambda r=r: fuse(pc, img, T, radius=r, rel_tol=0.05)]
        ms = BV.rounds(fns)
        counts = [int((fuse(pc, img, T, radius=r, rel_tol=0.05, want=('state',)).state == s).sum()) for r in RADII for s in (2, 3)]
        lines += ['', '%d x %d: %d of the points in frame; visible at radius %d: %d, at radius %d with rel_tol 0.05: %d'
                  % (h, w, counts[0] + counts[1], RADII[0], counts[1], RADII[1], counts[3])]
        us_last = kernel_us(last, LAST_KERNELS)
        dev_last = sum(us_last.values()) if isinstance(us_last, dict) else None
        lines += ['  %-40s %s   kernels %s' % ('efgh_sum_depth_last (yardstick)', BV.fmt(ms[0]),
                                                 ' + '.join('%s %.1f' % (k[2:], v) for k, v in us_last.items()) + ' = %.1f us' % dev_last
                                                 if dev_last else us_last)]
        zb = {}
        for j, r in enumerate(RADII):
            raw_ms, call_ms = ms[1 + 2 * j], ms[2 + 2 * j]
            us = kernel_us(lambda: launches(r), FUSE_KERNELS)
            if isinstance(us, dict):
                tot = sum(us.values())
                zb[r] = us.get('k_fuse_zbuffer')
                dev = 'kernels %s = %.1f us' % (' + '.join('%s %.1f' % (k[7:], v) for k, v in us.items()), tot)
                if dev_last:
                    dev += ', %.2f x the yardstick\'s kernels' % (tot / dev_last)
            else:
                dev = 'kernels ' + us
            lines += ['  %-40s %s   %s x the yardstick call   %s' % ('three launches, radius %d' % r, BV.fmt(raw_ms), ratio(raw_ms, ms[0]), dev),
                      '  %-40s %s   %s x the yardstick call' % ('fuse(...), radius %d, every output' % r, BV.fmt(call_ms), ratio(call_ms, ms[0]))]
        lines += ['  three launches, radius %d against radius %d: %s per round' % (RADII[1], RADII[0], ratio(ms[3], ms[1]))]
        if zb.get(RADII[0]) and zb.get(RADII[1]):
            k, win = zb[RADII[1]] / zb[RADII[0]], (2 * RADII[1] + 1) ** 2
            more = (counts[0] + counts[1]) * (win - 1)                      # (windows clipped at the frame not taken off)
            lines += ['  z-buffer kernel, radius %d against radius %d: %.1f x for %d x the atomics of an in-frame point; %.1f us more for '
                      '%d more atomics = %.3f ns each, %.1f atomics per ns (radius %d is launch and projection: see the yardstick\'s '
                      'first kernel)' % (RADII[1], RADII[0], k, win, zb[RADII[1]] - zb[RADII[0]], more,
                                         1e3 * (zb[RADII[1]] - zb[RADII[0]]) / more, more / (1e3 * (zb[RADII[1]] - zb[RADII[0]])), RADII[0])]
            if k > win:
                lines += ['  MORE than the count of atomics: the projection is the same, so the time is in the atomics themselves '
                          '(contention between overlapping windows)']
    lines += ['', 'not measured: host-array inputs (the upload), clouds with other overlap statistics, any effect on anything downstream']
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a' if a.append else 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
