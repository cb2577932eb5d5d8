"""The bits the three Adam entry points leave, recorded -> tests/golden/adam_bits.json (replayed by tests/test_gpu_adam_bits.py).
    python tests/golden/gen_adam_bits.py            (needs the GPU; run it BEFORE a change that must not move a bit)
Every case drives efgh_adam_step, efgh_adam_step_guarded or efgh_adam_step_groups through the C ABI for three consecutive steps from
non-zero moments (from zero moments the fused and the twice-rounded form of m and v coincide) and records the sha256 of the bytes
of w, m and v after each step; cases of at most 7 elements also record the int32 bit patterns, so that a failure can be read.
Inputs: tests/ema_contract.inputs (seeded numpy: wide magnitudes, +-0, denormals), v made non-negative, a gradient of its own per
step.  lr 1e-3, betas (0.9, 0.999), eps 1e-8, steps 1, 2, 3; run `wd0`: weight_decay 0, grad_scale 1; run `wd`: weight_decay 1e-2,
grad_scale 1/3.  The grouped cases take their groups' own rates and decays (LAYOUTS of tests/test_gpu_adam_groups.py)."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from test_gpu_adam_groups import BETAS, EPS, LAYOUTS, Guard, Table, _buffers, _dev, _hp, _launch  # noqa: E402

FIXTURE = os.path.join(HERE, 'adam_bits.json')
LR = 1e-3
RUNS = {'wd0': (0.0, 1.0), 'wd': (1e-2, 1.0 / 3.0)}          # name -> (weight_decay, grad_scale)
# the grid is capped at 16384 workgroups of 1024 elements: the smallest n whose grid-stride loop takes a second trip, with a tail
N_SECOND_TRIP = 16384 * 1024 + 1027
# its inputs repeat a block of this many elements (a prime: no stride of the launch is a multiple of it)
BLOCK = 1000003
SMALL = 7                                                     # up to here the bit patterns themselves are recorded


def _cases():
    """id -> (entry point, n or layout, mode, run), in a fixed order (a case's seed is its position)"""
    out = {}
    for run in RUNS:
        # tail only, body + every tail length; one sweep of a workgroup and its edges, several workgroups; the second trip
        for n in (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4099, N_SECOND_TRIP):
            out['flat-n%d-%s' % (n, run)] = ('flat', n, 'plain', run)
        for n in (3, 5, 1025, 4099):
            out['guarded-n%d-measure-%s' % (n, run)] = ('guarded', n, 'measure', run)       # max_norm = inf
        for n in (1025, 4099):
            out['guarded-n%d-clip-%s' % (n, run)] = ('guarded', n, 'clip', run)             # max_norm = half the measured norm
        out['guarded-n1025-skip-%s' % run] = ('guarded', 1025, 'skip', run)                 # step 2: one NaN, skip_nonfinite
    for layout in ('n4099', 'mixed', 'stride_grid2'):
        for mode in ('plain', 'clip'):
            out['groups-%s-%s' % (layout, mode)] = ('groups', layout, mode, 'wd')
    return out


CASES = _cases()


def _inputs(n, seed):
    if n <= BLOCK:
        return _buffers(n, seed)
    w, m, v, grads = _buffers(BLOCK, seed)
    return np.resize(w, n), np.resize(m, n), np.resize(v, n), [np.resize(g, n) for g in grads]


def _digest(t):
    return hashlib.sha256(t.cpu().numpy()).hexdigest()


def run_case(case):
    """-> {'steps': [{'w', 'm', 'v': sha256} x 3], and, where they exist, 'bits' (n <= 7), 'scale' and 'applied' (guarded) per step}"""
    from efgh_amd import _C
    kind, shape, mode, run = CASES[case]
    wd, grad_scale = RUNS[run]
    lib, f32 = _C.lib(), _C.c_float
    if kind == 'groups':
        n, ends, gids, groups, grid = LAYOUTS[shape]
        table = Table(ends, gids)
    else:
        n = shape
    w0, m0, v0, grads = _inputs(n, 1000 + list(CASES).index(case))
    assert np.count_nonzero(m0) and np.count_nonzero(v0)
    w, m, v = _dev(w0), _dev(m0), _dev(v0)
    guard = None if mode == 'plain' else Guard(n, float('inf'), skip_nonfinite=mode == 'skip')
    rec = {'steps': []}
    for step in (1, 2, 3):
        g = grads[step - 1]
        if mode == 'skip' and step == 2:
            g = g.copy()
            g[n // 2] = np.nan
        g = _dev(g)
        if guard is not None:
            guard.max_norm = float('inf')
            guard.measure(g, step, grad_scale)
            if mode == 'clip':
                norm = guard.read().norm
                assert np.isfinite(norm) and norm > 0.0
                guard.max_norm = 0.5 * norm
                guard.measure(g, step, grad_scale)
        if kind == 'flat':
            _C.check(lib.efgh_adam_step(_C.ptr(w), _C.ptr(g), _C.ptr(m), _C.ptr(v), _C.c_int64(n), f32(LR), f32(BETAS[0]),
                                        f32(BETAS[1]), f32(EPS), f32(wd), _C.c_int32(step), f32(grad_scale), _C.stream_ptr()))
        elif kind == 'guarded':
            _C.check(lib.efgh_adam_step_guarded(w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, BETAS[0], BETAS[1],
                                                EPS, wd, guard.state.data_ptr(), _C.stream_ptr()))
        else:
            _C.check(_launch(w, g, m, v, n, table, _hp(groups, step, grad_scale), None if guard is None else guard.state, grid))
        torch.cuda.synchronize()
        rec['steps'].append({'w': _digest(w), 'm': _digest(m), 'v': _digest(v)})
        if n <= SMALL:
            rec.setdefault('bits', []).append({k: t.cpu().numpy().view(np.int32).tolist() for k, t in (('w', w), ('m', m), ('v', v))})
        if guard is not None:
            st = guard.read()
            rec.setdefault('scale', []).append(int(np.float32(st.scale).view(np.int32)))
            rec.setdefault('applied', []).append(int(st.applied))
    return rec


def main():
    out = {case: run_case(case) for case in CASES}
    with open(FIXTURE, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s: %d cases' % (FIXTURE, len(out)))


if __name__ == '__main__':
    main()
