"""Gradient guard (global-norm clipping + non-finite-step skipping inside the fused Adam step): everything that can be checked
without a GPU - the C-ABI surface and its argument refusals, the state struct's layout, the segment derivation, the constructor
refusals, and the float64 restatement of the contract (tests/grad_guard_contract.py) against torch's own clip_grad_norm_ + Adam."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_guard_contract as contract  # noqa: E402

SYMBOLS = ('efgh_grad_guard_workspace', 'efgh_grad_guard_measure', 'efgh_adam_step_guarded')
FIELDS = ('sumsq', 'sumsq_total', 'norm', 'nonfinite', 'nonfinite_total', 'applied', 'skipped', 'coef', 'scale', 'bc1',
          'bc2_sqrt', 'skip', 'nseg')


def test_entry_points_are_in_header_and_library():
    from efgh_amd import _C
    hdr = open(os.path.join(ROOT, 'include', 'efgh_hip.h')).read()
    lib = _C.lib()
    for s in SYMBOLS:
        assert s + '(' in hdr
        assert getattr(lib, s) is not None
    assert 'typedef struct efgh_guard_state' in hdr
    assert '#define EFGH_GUARD_RUN %d' % _C.GUARD_RUN in hdr and '#define EFGH_GUARD_MAX_SEGMENTS %d' % _C.GUARD_MAX_SEGMENTS in hdr
    assert lib.efgh_version() == 4 and '#define EFGH_ABI_VERSION 4' in hdr          # additive: the ABI number did not move
    assert lib.efgh_grad_guard_workspace(0) == -1 and lib.efgh_grad_guard_workspace(1 << 31) == -1
    n = 47810443
    assert lib.efgh_grad_guard_workspace(n) >= 12 * (n // _C.GUARD_RUN + _C.GUARD_MAX_SEGMENTS)


def test_state_struct_layout_matches_header():
    from efgh_amd import _C
    src = '#include <stdio.h>\n#include "efgh_hip.h"\nint main(){printf("%zu",sizeof(efgh_guard_state));' + \
          ''.join('printf(" %%zu",__builtin_offsetof(efgh_guard_state,%s));' % f for f in FIELDS) + 'return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'p.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 'p.c'), '-o', os.path.join(d, 'p')])
        got = list(map(int, subprocess.check_output([os.path.join(d, 'p')]).split()))
    assert ctypes.sizeof(_C.GuardState) == got[0]
    assert [getattr(_C.GuardState, f).offset for f in FIELDS] == got[1:]
    assert [f for f, _ in _C.GuardState._fields_] == list(FIELDS)
    assert _C.GuardState.applied.offset % 8 == 0                                     # FusedAdam.t's setter writes it as one int64


def _measure(lib, g=0x1000, n=100, bounds=(0, 100), nseg=None, max_norm=1.0, grad_scale=1.0, skip=0, b1=0.9, b2=0.999, step=1,
             ws=0x2000, state=0x3000, grid=0):
    arr = (ctypes.c_int64 * len(bounds))(*bounds) if bounds is not None else None
    return lib.efgh_grad_guard_measure(g, n, arr, len(bounds) - 1 if nseg is None else nseg, max_norm, grad_scale, skip, b1, b2,
                                       step, ws, state, grid, None)


@pytest.mark.parametrize('kw', [
    dict(g=None), dict(ws=None), dict(state=None), dict(bounds=None, nseg=1),
    dict(n=0, bounds=(0, 0)), dict(n=-5, bounds=(0, -5)), dict(n=1 << 31, bounds=(0, 1 << 31)),
    dict(bounds=tuple(range(0, 100, 10)) + (100,)),                      # ten segments
    dict(bounds=(0,), nseg=0),
    dict(bounds=(0, 60, 40, 100)),                                       # unsorted
    dict(bounds=(0, 50, 50, 100)),                                       # an empty segment
    dict(bounds=(0, 50, 90)), dict(bounds=(1, 50, 100)), dict(bounds=(0, 50, 101)),      # not covering [0, n)
    dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=float('nan')),
    dict(g=0x1004), dict(ws=0x2004), dict(state=0x3004),                 # alignment
    dict(step=0), dict(grid=-1), dict(b1=1.0), dict(grad_scale=float('nan')),
], ids=lambda kw: ','.join('%s=%s' % (k, str(v)[:24]) for k, v in kw.items()))
def test_measure_refuses_bad_arguments_before_any_device_work(kw):
    """the pointers are fake: a call that passed validation would fault, so every one of these must be refused first"""
    from efgh_amd import _C
    lib = _C.lib()
    assert _measure(lib, **kw) == -1
    msg = lib.efgh_last_error().decode()
    assert 'invalid argument' in msg and 'guard.hip' in msg


@pytest.mark.parametrize('kw', [dict(w=None), dict(g=None), dict(m=None), dict(v=None), dict(state=None), dict(n=0),
                                dict(w=0x1004), dict(g=0x2008), dict(m=0x3004), dict(v=0x400c), dict(state=0x5004)],
                         ids=lambda kw: ','.join('%s=%s' % kv for kv in kw.items()))
def test_guarded_adam_refuses_bad_arguments_before_any_device_work(kw):
    from efgh_amd import _C
    lib = _C.lib()
    a = dict(w=0x1000, g=0x2000, m=0x3000, v=0x4000, n=100, state=0x5000)
    a.update(kw)
    assert lib.efgh_adam_step_guarded(a['w'], a['g'], a['m'], a['v'], a['n'], 1e-3, 0.9, 0.999, 1e-8, 0.0, a['state'], None) == -1
    assert 'invalid argument' in lib.efgh_last_error().decode()


def test_segments_follow_the_top_level_module_names(manifest):
    from efgh_amd import synthetic as syn
    from efgh_amd.nets import EFGHBackbone
    from efgh_amd.train import name_segments
    m = EFGHBackbone(syn.default_args((128, 256)))
    named = list(m.named_parameters())
    names, sizes = [k for k, _ in named], [p.numel() for _, p in named]
    segs = name_segments(names, sizes)
    assert [s[0] for s in segs] == ['E', 'H', 'F', 'G']
    per_net = {net: sum(k for n, k in zip(names, sizes) if n.startswith(net + '.')) for net in 'EHFG'}
    ends = np.cumsum([per_net[net] for net in 'EHFG']).tolist()
    assert [(s[1], s[2]) for s in segs] == list(zip([0] + ends[:-1], ends)) and ends[-1] == 47810443
    # frozen sub-networks: fewer segments
    keep = [(n, k) for n, k in zip(names, sizes) if not n.startswith('H.')]
    assert [s[0] for s in name_segments([n for n, _ in keep], [k for _, k in keep])] == ['E', 'F', 'G']
    # more than eight runs of equal name: one segment
    assert name_segments(['a.w', 'b.w', 'c.b'] * 3, [3] * 9) == [('all', 0, 27)]            # nine runs
    assert len(name_segments(['a.w', 'a.b', 'b.w'] * 4, [3] * 12)) == 8
    assert [s[0] for s in name_segments(['m%d.w' % i for i in range(8)], [5] * 8)] == ['m%d' % i for i in range(8)]
    assert name_segments(['a.w', 'a.b', 'b.w'], [4, 1, 7]) == [('a', 0, 5), ('b', 5, 12)]


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b = torch.nn.Linear(5, 3), torch.nn.Linear(3, 2)


@pytest.mark.parametrize('bad', ['1.0', 0, 0.0, -1.0, float('nan'), True, False, 1j, [1.0]], ids=repr)
def test_constructors_refuse_a_bad_max_grad_norm(bad):
    from efgh_amd import _C
    from efgh_amd.train import FlatParams, FusedAdam, Trainer
    with pytest.raises(_C.EfghError, match='max_grad_norm') as e:
        FusedAdam(FlatParams(_Toy()), max_grad_norm=bad)
    assert repr(bad) in str(e.value)
    with pytest.raises(_C.EfghError, match='max_grad_norm'):
        Trainer(_Toy(), None, max_grad_norm=bad)


def test_constructor_checks_segments_and_defaults_stay_unguarded():
    from efgh_amd import _C
    from efgh_amd.train import FlatParams, FusedAdam
    flat = FlatParams(_Toy())
    assert flat.n == 26
    opt = FusedAdam(flat)
    assert not opt.guarded and opt.state is None and opt.t == 0 and type(opt.t) is int
    with pytest.raises(_C.EfghError, match='guard'):
        opt.guard_stats()
    for segs in ([('a', 0, 10)], [('a', 0, 10), ('b', 11, 26)], [('a', 0, 0), ('b', 0, 26)], [('a', 10, 26), ('b', 0, 10)],
                 [('s%d' % i, i, i + 1) for i in range(25)] + [('z', 25, 26)]):
        with pytest.raises(_C.EfghError, match='segments'):
            FusedAdam(flat, skip_nonfinite=True, segments=segs)
    opt = FusedAdam(flat, max_grad_norm=float('inf'), segments=[('a', 0, 18), ('b', 18, 26)])
    assert opt.guarded and not opt.skip_nonfinite and opt.state.numel() == ctypes.sizeof(_C.GuardState)
    assert FusedAdam(flat, max_grad_norm=2).max_grad_norm == 2.0


def test_contract_matches_torch_clip_grad_norm_and_adam():
    """five steps with gradient scales 1e-3, 1e2, NaN, 1e-1, 3e4: the float64 restatement against clip_grad_norm_ + torch.optim.Adam
    on float64 CPU tensors, the NaN step left out on the torch side (a skipped step is an `optimizer.step()` that was not called)"""
    n, max_norm, gs, lr = 2003, 1.0, 0.5, 1e-3
    rs = np.random.RandomState(5)
    w0 = rs.standard_normal(n)
    grads = contract.gradients(n, seed=1)
    assert [bool(np.isnan(g).any()) for g in grads] == [False, False, True, False, False]
    got = contract.run(w0, grads, max_norm, gs, lr, skip_nonfinite=True, coef_dtype=np.float64)
    got32 = contract.run(w0, grads, max_norm, gs, lr, skip_nonfinite=True)
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.Adam([p], lr=lr)
    coefs = []
    for k, g in enumerate(grads):
        if np.isnan(g).any():
            w_before = got[k - 1][0]
            assert got[k][3]['skip'] and np.array_equal(got[k][0], w_before) and np.array_equal(got[k][1], got[k - 1][1])
            continue
        p.grad = torch.from_numpy(g.astype(np.float64) * gs)                  # the mean gradient
        norm = float(torch.nn.utils.clip_grad_norm_([p], max_norm))
        opt.step()
        d = got[k][3]
        assert abs(d['norm'] - norm) <= 1e-12 * norm
        assert float(np.abs(got[k][0] - p.detach().numpy()).max()) <= 1e-12
        st = opt.state[p]
        assert float(np.abs(got[k][1] - st['exp_avg'].numpy()).max()) <= 1e-12 * max(1.0, float(st['exp_avg'].abs().max()))
        assert int(st['step']) == d['applied']
        coefs.append(float(d['coef']))
        # the device rounds the coefficient once to fp32: a 2^-24 relative change of the scale moves a weight by less than lr * 1e-6
        assert float(np.abs(got32[k][0] - got[k][0]).max()) <= lr * 1e-6
    assert got[-1][3]['applied'] == 4 and got[-1][3]['skipped'] == 1
    assert coefs[0] == 1.0 and coefs[1] < 1e-3 and coefs[2] < 1.0 and coefs[3] < 1e-5      # the sequence exercises both regimes
    # without skipping the NaN reaches every weight, as in torch (error_if_nonfinite=False)
    bad = contract.run(w0, grads[:3], max_norm, gs, lr, skip_nonfinite=False)
    assert np.isnan(bad[2][0]).all() and bad[2][3]['applied'] == 3


def test_decide_rule_edge_cases():
    d = contract.decide([1e-14], [0], 1e-7, 1.0, True, 0, 0)                   # norm 1e-7, max_norm 1e-7: the + 1e-6 is visible
    assert abs(float(d['coef']) - 1e-7 / (1e-7 + 1e-6)) < 1e-8 and 0.0909 < float(d['coef']) < 0.0910
    assert float(contract.decide([4.0, 5.0], [0, 0], float('inf'), 1.0, False, 0, 0)['coef']) == 1.0
    assert float(contract.decide([0.0], [0], 1.0, 1.0, False, 0, 0)['coef']) == 1.0
    d = contract.decide([9.0, 16.0], [0, 0], 1.0, 0.5, False, 7, 2)
    assert d['norm'] == 2.5 and d['coef'] == np.float32(1.0 / (2.5 + 1e-6)) and d['scale'] == np.float32(0.5) * d['coef']
    assert (d['applied'], d['skipped']) == (8, 2)
    d = contract.decide([float('nan')], [1], 1.0, 1.0, True, 7, 2)
    assert d['skip'] and (d['applied'], d['skipped']) == (7, 3)
    d = contract.decide([float('nan')], [1], 1.0, 1.0, False, 7, 2)
    assert not d['skip'] and np.isnan(d['coef']) and d['applied'] == 8
