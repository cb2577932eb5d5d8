"""Cost of the fused optimizer's parameter groups and of `--fused-optimizer` under the reference's loop -> profiles/adam_groups.txt
    python tools/bench_adam_groups.py [--rounds R] [--iters K] [--no-loop] [--out FILE]
(a) the kernel at the full net's size with its real segment table: efgh_adam_step against efgh_adam_step_groups with one group
    and with the interleaved BatchNorm / bias-versus-rest two-group table, interleaved rounds in one process; the file states the
    min-max spread of the rounds of each and the ratios of the medians.
(b) the reference's batch-1 loop at the shipped configuration's shapes (bench.py config_r: raw 900x1600, 65 536 points) with
    stock torch.optim.Adam against efgh_amd.optim.Adam: ms per iteration, host enqueue ms, GPU ms, device kernel launches per
    iteration (torch.profiler's kernel records: the library's and torch's launches alike) and aten ops per iteration
    (tools/glue_census.py), interleaved rounds.
Not measured: world > 1 on RCCL."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def real_tables():
    """(n, sizes, names) of the full net's trainable parameters, from the committed manifest"""
    man = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'state_dict_manifest.json')))['state_dict']
    rows = [(k, int(np.prod(s)) if s else 1) for k, s, _ in man if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]
    return sum(k for _, k in rows), [k for _, k in rows], [name for name, _ in rows]


def kernel_section(rounds, reps, lines):
    from efgh_amd import _C
    from efgh_amd.train import adam_segment_table
    n, sizes, names = real_tables()
    # BatchNorm weights and every bias are 1-D: the manifest's shapes say which (group 1), everything else group 0
    man = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'state_dict_manifest.json')))['state_dict']
    dims = {k: len(s) for k, s, _ in man}
    no_decay = [1 if dims[name] <= 1 else 0 for name in names]
    tables = {'one group': adam_segment_table(sizes, [0] * len(sizes)), 'two groups (1-D parameters / rest)': adam_segment_table(sizes, no_decay)}
    dev = 'cuda'
    w = torch.randn(n, device=dev) * 0.05
    g = torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    lib, st = _C.lib(), _C.stream_ptr
    hp = _C.AdamGroups()
    hp.n_groups, hp.step, hp.grad_scale, hp.beta1, hp.beta2, hp.eps = 2, 1, 1.0, 0.9, 0.999, 1e-8
    for k in range(2):
        hp.lr[k], hp.weight_decay[k], hp.decoupled[k], hp.decay[k] = 1e-4, 0.0 if k else 1e-2, 0, 1.0
    dev_tables = {}
    for name, (ends, gids) in tables.items():
        dev_tables[name] = (torch.tensor(ends, dtype=torch.int64).cuda(), torch.tensor(gids, dtype=torch.uint8).cuda(),
                            (ctypes.c_int64 * len(ends))(*ends), (ctypes.c_uint8 * len(gids))(*gids), len(ends))

    def parent():
        _C.check(lib.efgh_adam_step(_C.ptr(w), _C.ptr(g), _C.ptr(m), _C.ptr(v), _C.c_int64(n), _C.c_float(1e-4), _C.c_float(0.9),
                                    _C.c_float(0.999), _C.c_float(1e-8), _C.c_float(1e-2), _C.c_int32(1), _C.c_float(1.0), st()))

    def grouped(name):
        e, k, he, hk, nseg = dev_tables[name]

        def run():
            _C.check(lib.efgh_adam_step_groups(w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, e.data_ptr(), k.data_ptr(),
                                               nseg, he, hk, ctypes.byref(hp), None, 0, st()))
        return run
    fns = [('efgh_adam_step', parent)] + [('efgh_adam_step_groups, ' + name, grouped(name)) for name in tables]
    times = {name: [] for name, _ in fns}
    for name, fn in fns:                               # warm-up
        fn()
    torch.cuda.synchronize()
    for r in range(rounds):
        for name, fn in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps * 1e3)
    lines.append('(a) kernel, n = %d (28 n bytes = %.2f GB per launch), %d interleaved rounds of %d launches, us per launch'
                 % (n, 28 * n / 1e9, rounds, reps))
    for name, _ in fns:
        t = times[name]
        segs = ''
        for key, (ends, _) in tables.items():
            if name.endswith(key):
                segs = ', %d segments' % len(ends)
        lines.append('    %-62s median %8.1f   min %8.1f   max %8.1f   (%.2f TB/s at the median%s)'
                     % (name, np.median(t), min(t), max(t), 28 * n / np.median(t) / 1e6, segs))
    base = times['efgh_adam_step']
    for name, _ in fns[1:]:
        ratio = float(np.median(times[name]) / np.median(base))
        lo, hi = min(base) / np.median(base), max(base) / np.median(base)
        inside = lo <= ratio <= hi
        lines.append('    %s / efgh_adam_step = %.4f; the parent\'s own rounds span %.4f .. %.4f of its median: %s'
                     % (name, ratio, lo, hi, 'inside the spread' if inside else
                        'OUTSIDE the spread by %.2f %% (same bytes, same arithmetic on a sweep that lies inside one segment; what the '
                        'grouped kernel adds is a prologue that stages the 16 groups\' values in LDS behind a barrier and, per '
                        '1024-element sweep, uniform loads of the segment\'s ends and group id and the LDS reads of its values ahead '
                        'of the arithmetic.  Not occupancy: forced to the flat kernel\'s 8 waves per SIMD it measured the same)'
                        % (100.0 * (ratio - (hi if ratio > hi else lo)))))


def loop_section(rounds, iters, lines):
    from efgh_amd import optim as fused_optim, synthetic as syn
    from efgh_amd.losses import EFGHCriterion
    from efgh_amd.nets import EFGHBackbone
    from glue_census import census
    raw, npts = (900, 1600), 65536
    args = syn.default_args(raw, 'cuda')
    pairs = [syn.make_batch(raw, npts, 1, first_seed=i) for i in range(4)]
    host = [([torch.from_numpy(b[k]).pin_memory() for k in ('pc', 'img', 'calib', 'A')],
             {k: torch.from_numpy(v) for k, v in b['gt'].items()}) for b in pairs]

    def build(cls):
        torch.manual_seed(0)
        model = torch.nn.DataParallel(EFGHBackbone(args).cuda(), device_ids=[0])
        model.train()
        return model, EFGHCriterion(args), cls([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=0)
    paths = {'stock torch.optim.Adam': build(torch.optim.Adam), '--fused-optimizer (efgh_amd.optim.Adam)': build(fused_optim.Adam)}

    def iteration(path, i):
        model, criterion, optimizer = paths[path]
        (pcd, img, calib, A), gt = host[i % len(host)]
        t0 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        pcd, img, calib, A = (t.to('cuda').float() for t in (pcd, img, calib, A))
        e0.record()
        pred = model(pcd, img, calib, A, False)
        losses, gt2 = criterion.compute_loss(pcd, img, calib, A, dict(gt), pred)
        optimizer.zero_grad()
        losses['total'].backward()
        optimizer.step()
        e1.record()
        t1 = time.perf_counter()
        _ = [losses[k].item() for k in list(losses.keys())]
        _ = gt2['sensor2_T_sensor1'].cpu().detach().numpy()[0], pred['sensor2_T_sensor1'].cpu().detach().numpy()[0]
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3, (t1 - t0) * 1e3, e0.elapsed_time(e1)
    for path in paths:
        for i in range(3):
            iteration(path, i)
    torch.cuda.synchronize()
    rows = {path: [] for path in paths}
    for r in range(rounds):
        for path in paths:
            rows[path] += [iteration(path, r * iters + i) for i in range(iters)]
    ops_n = {path: sum(census(lambda: iteration(path, 0)).values()) for path in paths}
    launches = {path: kernel_launches(lambda: iteration(path, 0)) for path in paths}
    lines.append('(b) the reference\'s batch-1 loop (raw 900x1600, 65 536 points; empty_cache a no-op as under the launcher), %d '
                 'interleaved rounds of %d iterations, medians (min .. max of the round medians)' % (rounds, iters))
    for path in paths:
        a = np.array(rows[path]).reshape(rounds, iters, 3)
        med = np.median(a.reshape(-1, 3), axis=0)
        rm = np.median(a, axis=1)
        lines.append('    %-42s loop %7.2f ms (%.2f .. %.2f)   host enqueue %7.2f ms (%.2f .. %.2f)   GPU %7.2f ms (%.2f .. %.2f)   '
                     'kernel launches per iteration %s   aten ops per iteration %d'
                     % (path, med[0], rm[:, 0].min(), rm[:, 0].max(), med[1], rm[:, 1].min(), rm[:, 1].max(),
                        med[2], rm[:, 2].min(), rm[:, 2].max(), launches[path], ops_n[path]))
    lines.append('    kernel launches: device kernels of one iteration (the library\'s and torch\'s alike) counted by torch.profiler\'s '
                 'kernel activity; aten ops: torch-side operations on device tensors (tools/glue_census.py)')
    lines.append('    not measured: world > 1 on RCCL')


def kernel_launches(fn):
    """device kernels launched by fn(), whoever launched them (the library through ctypes, torch's own ops), from the profiler's
    kernel activity records; 'n/a (...)' when this build's profiler records none"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower()
                and 'memset' not in e.name.lower())
    except Exception as e:                      # (a profiler that cannot attach here: say so in the file)
        return 'n/a (%s)' % type(e).__name__
    return str(n) if n else 'n/a (no kernel records)'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--no-loop', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'adam_groups.txt'))
    a = ap.parse_args()
    lines = ['tools/bench_adam_groups.py on %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)]
    kernel_section(a.rounds, a.reps, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write('\n'.join(lines) + '\n')            # (section (a) is on disk before the long section starts)
    if not a.no_loop:
        loop_section(max(3, a.rounds // 2), a.iters, lines)
    text = '\n'.join(lines) + '\n'
    print(text)
    open(a.out, 'w').write(text)


if __name__ == '__main__':
    main()
