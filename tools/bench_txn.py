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
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from efgh_amd import _C, ops, synthetic as syn  # noqa: E402
from efgh_amd.train import BnTransaction  # noqa: E402


def layout():
    """(starts, nf, nc) of the full net from the stored manifest (names and shapes; no model is built)"""
    man = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'state_dict_manifest.json')))
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

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls            # us per call

    for _, fn, _ in names:
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k, _, _ in names}
    for _ in range(a.rounds):
        for k, fn, _ in names:
            times[k].append(window(fn))
    st = _C.TxnState.from_buffer_copy(txn.cpu().numpy().tobytes())
    lines += ['transactional BatchNorm state at the full net\'s sizes: %d running statistics in %d floats (%d KB), %d counters'
              % (len(starts_h) - 1, nf, 4 * nf // 1024, nc),
              'one run on one MI355X; %d rounds, the four alternating; a window = %d back-to-back calls (device events, us per call)'
              % (a.rounds, a.calls),
              '%-28s %10s %10s %10s %10s' % ('', 'median us', 'min us', 'max us', 'KB moved')]
    for k, _, nbytes in names:
        t = times[k]
        lines.append('%-28s %10.2f %10.2f %10.2f %10.0f' % (k, statistics.median(t), min(t), max(t), nbytes / 1024))
    lines.append('last txn block: forward_nonfinite %d first_bad %d rolled_back %d vetoed_total %d'
                 % (st.forward_nonfinite, st.first_bad, st.rolled_back, st.vetoed_total))


def steps(a, lines):
    from efgh_amd.losses import EFGHCriterion
    from efgh_amd.nets import EFGHBackbone
    from efgh_amd.train import Trainer
    raw, npts, B = (768, 2560), 131072, 8
    dev = torch.device('cuda', 0)
    args = syn.default_args(raw, 'cuda')
    batch = syn.make_batch(raw, npts, B, first_seed=0)
    inp = [torch.from_numpy(batch[k]).to(dev) for k in ('pc', 'img', 'calib', 'A')]
    gt = {k: torch.from_numpy(v).to(dev) for k, v in batch['gt'].items()}
    forms = []
    for name, kw in (('skip_nonfinite', {}), ('skip_nonfinite + transactional', {'transactional': True})):
        torch.manual_seed(0)
        forms.append((name, Trainer(EFGHBackbone(args).to(dev), EFGHCriterion(args), lr=1e-4, skip_nonfinite=True, **kw)))
    for _, tr in forms:
        for _ in range(a.warmup):
            tr.step(*inp, gt)
    times = {name: [] for name, _ in forms}
    for _ in range(a.step_rounds):
        for name, tr in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.step(*inp, gt)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    lines.append('config S (%dx%d raw, %d points, batch %d), Trainer.step; %d rounds of %d steps per form after %d warm-up steps, the two '
                 'forms alternating; wall clock around a device synchronisation, ms per step'
                 % (raw[0], raw[1], npts, B, a.step_rounds, a.steps, a.warmup))
    for name, tr in forms:
        t = times[name]
        s = tr.guard_stats()
        lines.append('%-34s median %8.2f  min %8.2f  max %8.2f   (applied %d, skipped %d%s)'
                     % (name, statistics.median(t), min(t), max(t), s['applied'], s['skipped'],
                        ', rolled_back %d' % s['rolled_back'] if 'rolled_back' in s else ''))
    m0, m1 = (statistics.median(times[name]) for name, _ in forms)
    lines.append('transactional / guarded = %.4f (%+.2f ms per step)' % (m1 / m0, m1 - m0))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'txn.txt'))
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--calls', type=int, default=50, help='calls per timed window')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--step-rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-step', action='store_true', help='kernels only')
    a = ap.parse_args(argv)
    lines = []
    kernels(a, lines)
    if not a.no_step:
        torch.cuda.empty_cache()
        steps(a, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write(text)


if __name__ == '__main__':
    main()
