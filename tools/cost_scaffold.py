"""What the cost tools of the training step's options share (bench_grad_accum.py, bench_txn.py, bench_ema.py): device-event
windows over alternating rounds, the comparison of Trainer forms at config S, and the command line.  Not a tool of its own."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from efgh_amd import synthetic as syn  # noqa: E402

RAW, NPTS, BATCH = (768, 2560), 131072, 8                      # config S


def window(fn, calls):
    """`calls` back-to-back calls of fn between two device events -> us per call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def alternate(names, rounds, calls, warm=1):
    """names: [(label, fn, bytes)].  `warm` calls of each, then `rounds` rounds of one window per form, the forms alternating
    -> {label: [us per call, one per round]}"""
    for _, fn, _ in names:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k, _, _ in names}
    for _ in range(rounds):
        for k, fn, _ in names:
            times[k].append(window(fn, calls))
    return times


def table(names, times, row, last):
    """one line per form: row % (label, median, min, max, last(bytes, median))"""
    return [row % (k, statistics.median(times[k]), min(times[k]), max(times[k]), *last(nbytes, statistics.median(times[k])))
            for k, _, nbytes in names]


def config_s():
    """-> (args, [pc, img, calib, A], gt) of one config-S batch on the device"""
    dev = torch.device('cuda', 0)
    batch = syn.make_batch(RAW, NPTS, BATCH, first_seed=0)
    return (syn.default_args(RAW, 'cuda'), [torch.from_numpy(batch[k]).to(dev) for k in ('pc', 'img', 'calib', 'A')],
            {k: torch.from_numpy(v).to(dev) for k, v in batch['gt'].items()})


def trainer(args, **kw):
    from efgh_amd.losses import EFGHCriterion
    from efgh_amd.nets import EFGHBackbone
    from efgh_amd.train import Trainer
    torch.manual_seed(0)
    return Trainer(EFGHBackbone(args).to(torch.device('cuda', 0)), EFGHCriterion(args), lr=1e-4, **kw)


def compare_trainers(a, lines, forms):
    """forms: [(label, Trainer keywords)], one Trainer each; after warm-up a.step_rounds rounds of a.steps plain steps per form, the
    forms alternating, wall clock around a device synchronisation -> ([(label, Trainer)], {label: [ms per step, one per round]})"""
    args, inp, gt = config_s()
    forms = [(name, trainer(args, **kw)) for name, kw in forms]
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
                 % (RAW[0], RAW[1], NPTS, BATCH, a.step_rounds, a.steps, a.warmup))
    return forms, times


def main(argv, out, kernels, steps, calls, extra=()):
    """the tools' command line: kernels(a, lines), then steps(a, lines) unless --no-step; the lines are printed and written to
    --out (default profiles/<out>).  `extra`: further (flag, keywords) arguments -> what kernels() returned"""
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', out))
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--calls', type=int, default=calls[0], help=calls[1])
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-step', action='store_true', help='kernels only')
    for flag, kw in extra:
        ap.add_argument(flag, **kw)
    a = ap.parse_args(argv)
    lines = []
    result = kernels(a, lines)
    if not a.no_step:
        torch.cuda.empty_cache()
        steps(a, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write(text)
    return result
