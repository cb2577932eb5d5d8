"""Cost of the gradient guard at the real size (GPU box): efgh_adam_step, the guard's measure + decide launches and
efgh_adam_step_guarded on n = 47 810 443 parameters cut into the model's four segments (E, H, F, G), timed in ONE run with
device events, the three alternating round by round.  Every call works on the next of `--sets` buffer sets, so that the 191 MB
gradient is read from HBM and not from the 256-MB last-level cache it would otherwise sit in.

    python tools/bench_grad_guard.py [--out profiles/grad_guard.txt]

Bytes: k_adam_flat moves 28 n (reads w, g, m, v; writes w, m, v), the measure pass reads 4 n."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from efgh_amd import _C  # noqa: E402
from efgh_amd.train import name_segments  # noqa: E402


def model_segments():
    """the four segments of the real model from the stored manifest (names and shapes; no model is built)"""
    man = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'state_dict_manifest.json')))
    shape = {k: s for k, s, _ in man['state_dict']}
    sizes = []
    for k in man['parameters']:
        n = 1
        for d in shape[k]:
            n *= d
        sizes.append(n)
    return name_segments(man['parameters'], sizes)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'grad_guard.txt'))
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--calls', type=int, default=12, help='calls per timed window (a multiple of --sets)')
    ap.add_argument('--sets', type=int, default=3)
    a = ap.parse_args(argv)
    segs = model_segments()
    n = segs[-1][2]
    lib = _C.lib()
    dev = torch.device('cuda', 0)
    bounds = (ctypes.c_int64 * (len(segs) + 1))(0, *[e for _, _, e in segs])
    sets = []
    for i in range(a.sets):
        g = torch.randn(n, device=dev) * 1e-3
        sets.append({'w': torch.randn(n, device=dev), 'g': g, 'm': torch.zeros(n, device=dev), 'v': torch.zeros(n, device=dev),
                     'ws': torch.empty(lib.efgh_grad_guard_workspace(n), dtype=torch.uint8, device=dev),
                     'st': torch.zeros(ctypes.sizeof(_C.GuardState), dtype=torch.uint8, device=dev)})
    stream = _C.stream_ptr()
    step = [0]

    def adam(s):
        step[0] += 1
        _C.check(lib.efgh_adam_step(_C.ptr(s['w']), _C.ptr(s['g']), _C.ptr(s['m']), _C.ptr(s['v']), _C.c_int64(n), _C.c_float(1e-4),
                                    _C.c_float(0.9), _C.c_float(0.999), _C.c_float(1e-8), _C.c_float(0.0), _C.c_int32(step[0]),
                                    _C.c_float(1.0), stream))

    def measure(s):
        _C.check(lib.efgh_grad_guard_measure(s['g'].data_ptr(), n, bounds, len(segs), 1.0, 1.0, 1, 0.9, 0.999, 0,
                                             s['ws'].data_ptr(), s['st'].data_ptr(), 0, stream))

    def adam_guarded(s):
        _C.check(lib.efgh_adam_step_guarded(s['w'].data_ptr(), s['g'].data_ptr(), s['m'].data_ptr(), s['v'].data_ptr(), n, 1e-4,
                                            0.9, 0.999, 1e-8, 0.0, s['st'].data_ptr(), stream))

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.calls):
            fn(sets[i % a.sets])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls            # us per call

    for s in sets:                                            # warm-up; leaves skip = 0 and a finite scale in every state block
        adam(s); measure(s); adam_guarded(s)
    torch.cuda.synchronize()
    names = [('efgh_adam_step', adam, 28 * n), ('guard measure + decide', measure, 4 * n), ('efgh_adam_step_guarded', adam_guarded, 28 * n)]
    times = {k: [] for k, _, _ in names}
    for _ in range(a.rounds):
        for k, fn, _ in names:
            times[k].append(window(fn))
    st = _C.GuardState.from_buffer_copy(sets[0]['st'].cpu().numpy().tobytes())
    lines = ['gradient guard at n = %d, segments %s' % (n, ', '.join('%s [%d, %d)' % s for s in segs)),
             'one run on one MI355X; %d rounds, the three alternating; a window = %d back-to-back calls over %d buffer sets (device '
             'events, us per call)' % (a.rounds, a.calls, a.sets),
             '%-26s %10s %10s %10s %10s' % ('', 'median us', 'min us', 'max us', 'GB/s (median)')]
    med = {}
    for k, _, nbytes in names:
        t = times[k]
        med[k] = statistics.median(t)
        lines.append('%-26s %10.1f %10.1f %10.1f %10.0f' % (k, med[k], min(t), max(t), nbytes / med[k] / 1e3))
    lines.append('measure + decide / efgh_adam_step = %.3f (byte ratio 4n / 28n = 0.143; above 0.286 wants an explanation)'
                 % (med['guard measure + decide'] / med['efgh_adam_step']))
    lines.append('efgh_adam_step_guarded / efgh_adam_step = %.3f' % (med['efgh_adam_step_guarded'] / med['efgh_adam_step']))
    lines.append('last state block: norm %.6g coef %.6g applied %d skipped %d nonfinite %d' % (st.norm, st.coef, st.applied, st.skipped,
                                                                                             st.nonfinite_total))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write(text)


if __name__ == '__main__':
    main()
