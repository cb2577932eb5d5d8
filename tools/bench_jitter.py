"""What the photometric jitter costs in sample preparation, and that leaving it off costs nothing.

Per image size (1200x1920 RELLIS, 900x1600 nuScenes, 376x1241 KITTI; random bytes, resident on the device): `color_jitter` with all
four ops (brightness, contrast, saturation, hue: two launches), with brightness only (one launch), with contrast only and with hue
only (to see which op holds the time), and as the yardstick one `efgh_prep_crop_pad_u8` pass over the same bytes (`crop_image` to the
image's own size: one read and one write of the image, where the jitter with contrast is two reads and one write).  Then
`preproc_img` without a jitter, and with `--parent DIR` the parent commit's `preproc_img` on the same image in the same rounds.

Method: warm-up, then ROUNDS interleaved rounds (every round starts one callable further on) of CALLS calls each, every round closed
by a device synchronise; per-call time of a round = round time / CALLS, so it holds the host's share of a call (allocation, launch).
Reported: the median over the rounds and their min .. max, and the device time of the kernels from torch.profiler's kernel records of
separate, untimed calls.  The gate on the unchanged path: outputs equal to the parent's bit for bit, and the median inside the parent's
own min .. max of this run, or below it.

Not measured: host-array inputs (the upload), any effect on training or on registration accuracy.

    python tools/bench_jitter.py [--parent DIR] [--out profiles/jitter.txt]
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

import bench_voxel as BV  # noqa: E402  (the interleaved rounds and the parent loader)
from efgh_amd.data import JitterParams, color_jitter, preproc_gt, preproc_img  # noqa: E402
from efgh_amd.data.prepare import crop_image  # noqa: E402

SIZES = ((1200, 1920), (900, 1600), (376, 1241))
FACTORS = {'brightness': 1.3, 'contrast': 0.7, 'saturation': 1.4, 'hue': 0.07}
KERNELS = ('k_jitter_sum', 'k_jitter_apply', 'k_crop_pad_u8')


def kernel_us(fn, calls=10):
    """{kernel: mean device microseconds per call} of the jitter and crop kernels, or a string saying why there is none"""
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
    for k in KERNELS:
        us = [float(getattr(e, 'device_time', None) or getattr(e, 'cuda_time', 0.0)) for e in ev if k in e.name]
        if us:
            out[k] = sum(us) / calls
    return out or 'n/a (no kernel records)'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='checkout of the parent commit with its library built')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jitter.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_jitter: needs the GPU (there is no CPU path to time)')
    parent = BV.load_parent(a.parent) if a.parent else None
    gts = preproc_gt(0.1, -0.05, 0.3, 0.2, 0.1, -0.3, 0.15)
    order = ('brightness', 'contrast', 'saturation', 'hue')
    settings = [('all four ops', JitterParams(order, [FACTORS[o] for o in order]))] + \
               [('%s only' % o, JitterParams((o,), (FACTORS[o],))) for o in ('brightness', 'contrast', 'hue')]
    lines = ['color_jitter on a resident uint8 RGB image, %s; %d interleaved rounds of %d calls, median (min .. max) per call'
             % (torch.cuda.get_device_name(0), BV.ROUNDS, BV.CALLS)]
    verdicts = []
    for h, w in SIZES:
        img = torch.from_numpy(np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
        raw = (h, w)
        fns = [lambda p=p: color_jitter(img, p) for _, p in settings]
        fns += [lambda: crop_image(img, raw, init=True), lambda: preproc_img(img, gts, raw, True)]
        if parent is not None:
            fns += [lambda: parent.preproc_img(img, gts, raw, True)]
        ms = BV.rounds(fns)
        mb = h * w * 3 / 1e6
        lines += ['', '%d x %d (%.2f MB)' % (h, w, mb)]
        crop_ms, crop_us = ms[len(settings)], kernel_us(fns[len(settings)])
        dev_crop = crop_us.get('k_crop_pad_u8') if isinstance(crop_us, dict) else None
        lines += ['  %-34s %s   kernel %s' % ('crop_pad pass (yardstick)', BV.fmt(crop_ms),
                                              '%.1f us (%.2f TB/s read + write)' % (dev_crop, 2 * mb / dev_crop) if dev_crop else crop_us)]
        for (label, _), v, fn in zip(settings, ms, fns):
            us = kernel_us(fn)
            if isinstance(us, dict):
                tot = sum(us.get(k, 0.) for k in KERNELS[:2])
                dev = 'kernels %s = %.1f us' % (' + '.join('%s %.1f' % (k[2:], us[k]) for k in KERNELS[:2] if k in us), tot)
                if dev_crop:
                    dev += ', %.2f x the crop_pad kernel' % (tot / dev_crop)
            else:
                dev = 'kernels ' + us
            lines += ['  %-34s %s   %.2f x the crop_pad call   %s' % ('color_jitter, ' + label, BV.fmt(v),
                                                                       statistics.median(v) / statistics.median(crop_ms), dev)]
        new = ms[len(settings) + 1]
        lines += ['  %-34s %s' % ('preproc_img, no jitter', BV.fmt(new))]
        if parent is None:
            lines += ['  parent commit not measured (no --parent checkout given)']
            continue
        old = ms[len(settings) + 2]
        mine, theirs = preproc_img(img, gts, raw, True), parent.preproc_img(img, gts, raw, True)
        same = all(torch.equal(mine[k], theirs[k]) for k in theirs) and mine.keys() == theirs.keys()
        med, lo, hi = statistics.median(new), min(old), max(old)
        verdicts.append(med <= hi and same)
        lines += ['  %-34s %s   outputs bit-identical: %s' % ('parent commit\'s preproc_img', BV.fmt(old), same),
                  '  gate: median %.3f ms %s the parent\'s round-to-round spread %.3f .. %.3f ms (%.1f %% of its median)'
                  % (med, 'lies inside' if lo <= med <= hi else ('lies BELOW' if med < lo else 'lies ABOVE'), lo, hi,
                     100 * (hi - lo) / statistics.median(old))]
    lines += ['', 'not measured: host-array inputs (the upload), any effect on training or on registration accuracy']
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)
    if verdicts and not all(verdicts):
        raise SystemExit('bench_jitter: preproc_img without a jitter lies above the parent\'s spread, or its outputs differ')


if __name__ == '__main__':
    main()
