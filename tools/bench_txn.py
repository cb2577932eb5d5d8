"""Cost of the transactional BatchNorm state (GPU box), recorded and not gated:
  1. efgh_txn_snapshot, efgh_txn_probe and efgh_txn_resolve - in both branches: nothing to do, and restore - at the full net's
     buffer sizes (186 running statistics laid out as train.BnTransaction lays them out, 93 counters), timed in ONE run with device
     events after warm-up, the four alternating round by round.
  2. Trainer(skip_nonfinite=True) against Trainer(skip_nonfinite=True, transactional=True) at config S (768 x 2560 raw, 131 072
     points, batch 8), alternating in one run.  With the option off the step is the parent's guarded step launch for launch, so
     the first line is the yardstick for the second (`--no-step` leaves this part out).

    python tools/bench_txn.py [--out profiles/txn.txt]

Bytes: snapshot and a restoring resolve move 8 nf + 16 nc (read one side, write the other), the probe reads 8 nf, a resolve with
nothing to do reads two state blocks: well under 1 MB each, so the expectation is one launch floor per call."""
import ctypes
import json
import os
import statistics

import cost_scaffold as cs
import torch

from efgh_amd import _C, ops
from efgh_amd.train import BnTransaction


def layout():
    """(starts, nf, nc) of the full net from the stored manifest (names and shapes; no model is built)"""
    man = json.load(open(os.path.join(cs.ROOT, 'tests', 'golden', 'state_dict_manifest.json')))
    starts, off, nc = [], 0, 0
    for k, shape, _ in man['state_dict']:
        if k.endswith(('running_mean', 'running_var')):
            n = 1
            for d in shape:
                n *= d
            starts.append(off)
            off += -(-n // BnTransaction.ALIGN) * BnTransaction.ALIGN
        nc += k.endswith('num_batches_tracked')
    return starts + [off], off, nc


def kernels(a, lines):
    dev = torch.device('cuda', 0)
    starts_h, nf, nc = layout()
    live, shadow = torch.randn(nf, device=dev), torch.randn(nf, device=dev)
    lc, sc = torch.arange(nc, device=dev), torch.zeros(nc, dtype=torch.int64, device=dev)
    starts = torch.tensor(starts_h, dtype=torch.int64, device=dev)
    loss = torch.ones(1, device=dev)
    txn = torch.zeros(ctypes.sizeof(_C.TxnState), dtype=torch.uint8, device=dev)
    applied = torch.zeros(ctypes.sizeof(_C.GuardState), dtype=torch.uint8, device=dev)
    skipped = applied.clone()                                 # a guard block as the decide launch leaves it after a NaN gradient
    off = _C.GuardState.nonfinite_total.offset
    skipped[off:off + 8].view(torch.int64).fill_(1)
    off = _C.GuardState.skip.offset
    skipped[off:off + 4].view(torch.int32).fill_(1)
    names = [('efgh_txn_snapshot', lambda: ops.txn_snapshot(live, shadow, lc, sc, txn), 8 * nf + 16 * nc),
             ('efgh_txn_probe', lambda: ops.txn_probe(live, shadow, starts, txn, loss, 1, 1), 8 * nf),
             ('efgh_txn_resolve, applied', lambda: ops.txn_resolve(live, shadow, lc, sc, applied, txn, 0.9, 0.999), 0),
             ('efgh_txn_resolve, restore', lambda: ops.txn_resolve(live, shadow, lc, sc, skipped, txn, 0.9, 0.999), 8 * nf + 16 * nc)]

    times = cs.alternate(names, a.rounds, a.calls)
    st = _C.TxnState.from_buffer_copy(txn.cpu().numpy().tobytes())
    lines += ['transactional BatchNorm state at the full net\'s sizes: %d running statistics in %d floats (%d KB), %d counters'
              % (len(starts_h) - 1, nf, 4 * nf // 1024, nc),
              'one run on one MI355X; %d rounds, the four alternating; a window = %d back-to-back calls (device events, us per call)'
              % (a.rounds, a.calls),
              '%-28s %10s %10s %10s %10s' % ('', 'median us', 'min us', 'max us', 'KB moved')]
    lines += cs.table(names, times, '%-28s %10.2f %10.2f %10.2f %10.0f', lambda nbytes, med: (nbytes / 1024,))
    lines.append('last txn block: forward_nonfinite %d first_bad %d rolled_back %d vetoed_total %d'
                 % (st.forward_nonfinite, st.first_bad, st.rolled_back, st.vetoed_total))


def steps(a, lines):
    forms, times = cs.compare_trainers(a, lines, [('skip_nonfinite', {'skip_nonfinite': True}),
                                                  ('skip_nonfinite + transactional', {'skip_nonfinite': True, 'transactional': True})])
    for name, tr in forms:
        t = times[name]
        s = tr.guard_stats()
        lines.append('%-34s median %8.2f  min %8.2f  max %8.2f   (applied %d, skipped %d%s)'
                     % (name, statistics.median(t), min(t), max(t), s['applied'], s['skipped'],
                        ', rolled_back %d' % s['rolled_back'] if 'rolled_back' in s else ''))
    m0, m1 = (statistics.median(times[name]) for name, _ in forms)
    lines.append('transactional / guarded = %.4f (%+.2f ms per step)' % (m1 / m0, m1 - m0))


def main(argv=None):
    cs.main(argv, 'txn.txt', kernels, steps, (50, 'calls per timed window'), extra=[('--step-rounds', {'type': int, 'default': 3})])


if __name__ == '__main__':
    main()
