"""Cost of gradient accumulation at the real size (GPU box), recorded and not gated:
  1. efgh_grad_drain at n = 47 810 443, `first` and not, beside torch's `acc.add_(g)` + `g.zero_()` and beside efgh_adam_step, timed
     in ONE run with device events, alternating round by round.  Every call works on the next of `--sets` buffer sets, so that the
     191-MB buffers come from HBM and not from the 256-MB last-level cache.
  2. efgh_gimg_valid_count on a 768 x 2560 x 8 depth image.
  3. Trainer.step_accumulated with 2 micro-batches of 4 against Trainer.step at batch 8 on config S (768 x 2560 raw, 131 072 points):
     time per optimizer step and peak allocated memory of each (`--no-step` leaves this part out).

    python tools/bench_grad_accum.py [--out profiles/grad_accum.txt]

Bytes: the drain moves 12 n with `first` (read g; write acc, g) and 16 n otherwise; k_adam_flat moves 28 n."""
import statistics
import time

import cost_scaffold as cs
import torch

from efgh_amd import _C, ops

N = 47810443


def kernels(a, lines):
    lib, dev, n = _C.lib(), torch.device('cuda', 0), N
    sets = [{'w': torch.randn(n, device=dev), 'g': torch.randn(n, device=dev) * 1e-3, 'acc': torch.zeros(n, device=dev),
             'm': torch.zeros(n, device=dev), 'v': torch.zeros(n, device=dev)} for _ in range(a.sets)]
    step = [0]

    def adam(s):
        step[0] += 1
        _C.check(lib.efgh_adam_step(_C.ptr(s['w']), _C.ptr(s['g']), _C.ptr(s['m']), _C.ptr(s['v']), _C.c_int64(n), _C.c_float(1e-4),
                                    _C.c_float(0.9), _C.c_float(0.999), _C.c_float(1e-8), _C.c_float(0.0), _C.c_int32(step[0]),
                                    _C.c_float(1.0), _C.stream_ptr()))

    def torch_pair(s):
        s['acc'].add_(s['g'])
        s['g'].zero_()

    def rotating(fn, over):                                   # every call works on the next buffer set
        i = [0]

        def call():
            fn(over[i[0] % len(over)])
            i[0] += 1
        return call

    names = [('efgh_grad_drain first', rotating(lambda s: ops.grad_drain(s['acc'], s['g'], True), sets), 12 * n),
             ('efgh_grad_drain', rotating(lambda s: ops.grad_drain(s['acc'], s['g'], False), sets), 16 * n),
             ('acc.add_(g) + g.zero_()', rotating(torch_pair, sets), 16 * n),
             ('efgh_adam_step', rotating(adam, sets), 28 * n)]
    times = cs.alternate(names, a.rounds, a.calls, warm=a.sets)
    lines += ['gradient accumulation at n = %d' % n,
              'one run on one MI355X; %d rounds, the four alternating; a window = %d back-to-back calls over %d buffer sets (device '
              'events, us per call)' % (a.rounds, a.calls, a.sets),
              '%-26s %10s %10s %10s %10s' % ('', 'median us', 'min us', 'max us', 'GB/s (median)')]
    lines += cs.table(names, times, '%-26s %10.1f %10.1f %10.1f %10.0f', lambda nbytes, med: (nbytes / med / 1e3,))
    med = {k: statistics.median(t) for k, t in times.items()}
    lines.append('efgh_grad_drain / efgh_adam_step = %.3f (byte ratio 16n / 28n = 0.571); / the torch pair = %.3f'
                 % (med['efgh_grad_drain'] / med['efgh_adam_step'], med['efgh_grad_drain'] / med['acc.add_(g) + g.zero_()']))
    del sets, names
    # the valid count at the full raw size, batch 8
    B, H, W = 8, 768, 2560
    imgs = [torch.rand(B, H, W, 4, device=dev) - 0.5 for _ in range(a.sets)]
    masks = [(torch.rand(B, 1, H, W, device=dev) > 0.1).to(torch.uint8) for _ in range(a.sets)]
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    valid_count = rotating(lambda s: ops.gimg_valid_count(s[0], s[1], count), list(zip(imgs, masks)))
    ts = [cs.window(valid_count, a.calls) for _ in range(a.rounds + 1)][1:]          # (the first window warms up)
    nbytes = B * H * W * 17                                    # (the 16-byte pixel's sector is fetched for its one depth word)
    lines.append('efgh_gimg_valid_count %dx%dx%d: median %.1f us (min %.1f, max %.1f), %.0f GB/s of the %d bytes it touches'
                 % (H, W, B, statistics.median(ts), min(ts), max(ts), nbytes / statistics.median(ts) / 1e3, nbytes))


def steps(a, lines):
    from efgh_amd.train import split_micro_batches
    raw, npts = cs.RAW, cs.NPTS
    args, inp, gt = cs.config_s()
    tr = cs.trainer(args)
    mbs = split_micro_batches(*inp, gt, 2)
    forms = [('step, batch 8', lambda: tr.step(*inp, gt)),
             ('step_accumulated, 2 micro-batches of 4', lambda: tr.step_accumulated(mbs)),
             ('step_accumulated, plain mean', lambda: tr.step_accumulated(mbs, exact_depth_mean=False))]
    lines.append('config S (%dx%d raw, %d points), one optimizer step on 8 frame-pairs; %d timed steps after %d warm-up, wall clock '
                 'around a device synchronisation; peak = torch.cuda.max_memory_allocated over the timed steps'
                 % (raw[0], raw[1], npts, a.steps, a.warmup))
    for name, fn in forms:
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        lines.append('%-42s %8.1f ms per step   peak %7.2f GB' % (name, ms, torch.cuda.max_memory_allocated() / 1e9))


def main(argv=None):
    cs.main(argv, 'grad_accum.txt', kernels, steps, (12, 'calls per timed window (a multiple of --sets)'),
            extra=[('--sets', {'type': int, 'default': 3})])


if __name__ == '__main__':
    main()
