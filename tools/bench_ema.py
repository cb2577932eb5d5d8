"""Cost of the weight average (GPU box), recorded and not gated - except for one condition:
  1. efgh_ema_update (with and without a state block) and efgh_ema_swap at the full net's n = 47 810 443 next to efgh_adam_step on
     buffers of the same size, timed in ONE run with device events after warm-up, the forms alternating round by round.  The update
     moves 12 n bytes against Adam's 28 n through the same launch shape: it must take less time than Adam in this run, or the
     kernel is wrong (the tool exits with status 1 then).
  2. Trainer() against Trainer(ema_decay=0.999) at config S (768 x 2560 raw, 131 072 points, batch 8), alternating in one run.
     With the option off the step is the parent's launch for launch, so the first line is the yardstick for the second
     (`--no-step` leaves this part out).

    python tools/bench_ema.py [--out profiles/ema.txt]"""
import ctypes
import statistics
import sys

import cost_scaffold as cs
import torch

from efgh_amd import _C, ops

N_FULL = 47810443


def kernels(a, lines):
    dev = torch.device('cuda', 0)
    n = a.n
    w, g, m, v, ema, other = (torch.randn(n, device=dev) * s for s in (1.0, 1e-3, 0.0, 0.0, 1.0, 1.0))
    v.abs_()
    state = torch.zeros(ctypes.sizeof(_C.GuardState), dtype=torch.uint8, device=dev)
    off = _C.GuardState.applied.offset
    state[off:off + 8].view(torch.int64).fill_(100000)
    lib = _C.lib()

    def adam():
        _C.check(lib.efgh_adam_step(_C.ptr(w), _C.ptr(g), _C.ptr(m), _C.ptr(v), _C.c_int64(n), _C.c_float(1e-4), _C.c_float(0.9),
                                    _C.c_float(0.999), _C.c_float(1e-8), _C.c_float(0.0), _C.c_int32(1000), _C.c_float(1.0),
                                    _C.stream_ptr()))
    names = [('efgh_adam_step', adam, 28 * n),
             ('efgh_ema_update, host step', lambda: ops.ema_update(ema, w, 0.999, True, 100000), 12 * n),
             ('efgh_ema_update, state block', lambda: ops.ema_update(ema, w, 0.999, True, 0, state), 12 * n),
             ('efgh_ema_swap', lambda: ops.ema_swap(ema, other), 16 * n)]

    times = cs.alternate(names, a.rounds, a.calls)
    lines += ['weight average at n = %d (%.0f MB per buffer)' % (n, 4 * n / 1e6),
              'one run on one MI355X; %d rounds, the forms alternating; a window = %d back-to-back calls (device events, us per call)'
              % (a.rounds, a.calls),
              '%-30s %10s %10s %10s %10s %10s' % ('', 'median us', 'min us', 'max us', 'MB moved', 'TB/s')]
    lines += cs.table(names, times, '%-30s %10.2f %10.2f %10.2f %10.0f %10.2f', lambda nbytes, med: (nbytes / 1e6, nbytes / med / 1e6))
    med = {k: statistics.median(t) for k, t in times.items()}
    worst = max(med['efgh_ema_update, host step'], med['efgh_ema_update, state block'])
    ok = worst < med['efgh_adam_step']
    lines.append('efgh_ema_update / efgh_adam_step = %.3f (by bytes 12 / 28 = 0.429): %s'
                 % (worst / med['efgh_adam_step'], 'less time than Adam, as required' if ok else 'NOT less time than Adam: the kernel is wrong'))
    return ok


def steps(a, lines):
    forms, times = cs.compare_trainers(a, lines, [('Trainer()', {}), ('Trainer(ema_decay=0.999)', {'ema_decay': 0.999})])
    for name, tr in forms:
        t = times[name]
        lines.append('%-28s median %8.2f  min %8.2f  max %8.2f   (n = %d, %s)'
                     % (name, statistics.median(t), min(t), max(t), tr.flat.n,
                        'no average' if tr.ema is None else 'average: %.0f MB' % (4 * tr.ema.buf.numel() / 1e6)))
    m0, m1 = (statistics.median(times[name]) for name, _ in forms)
    spread = max(max(t) - min(t) for t in times.values())
    lines.append('with the average / without = %.4f (%+.2f ms per step; spread of the rounds up to %.2f ms)' % (m1 / m0, m1 - m0, spread))


def main(argv=None):
    ok = cs.main(argv, 'ema.txt', kernels, steps, (20, 'calls per timed window'),
                 extra=[('--n', {'type': int, 'default': N_FULL}), ('--step-rounds', {'type': int, 'default': 3})])
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
