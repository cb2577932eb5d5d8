"""efgh_adam_step_groups through the C-ABI.  The yardstick is the library's own ungrouped kernels, bit for bit: for any segment
table the launch must leave in every segment exactly the bits that efgh_adam_step (or efgh_adam_step_guarded reading the same
state block) leaves when run on fresh 16-byte-aligned copies of that segment alone with its group's lr / weight_decay; a decoupled
group is `w.mul_(decay)` by torch in fp32 followed by that kernel with weight_decay = 0.  (Both sides share one written-out update,
csrc/adam.hip; what anchors it is tests/test_gpu_adam_bits.py.)"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ema_contract import inputs as contract_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
BETAS, EPS = (0.9, 0.999), 1e-8
MODES = ('plain', 'measure', 'clip')          # unguarded / guarded with max_grad_norm = inf / guarded with a real clip


def _lengths_700():
    return [1 + s % 7 for s in range(700)]


def _cum(lengths):
    return list(np.cumsum(lengths).astype(np.int64))


def _groups(n_groups, decoupled=()):
    """lr / weight_decay per group: distinct rates, every other group with decay"""
    return [{'lr': 1e-3 * (1.0 + 0.25 * k), 'weight_decay': 1e-2 * (1 + k) if k % 2 else 0.0, 'decoupled': k in decoupled}
            for k in range(n_groups)]


# name -> (n, ends, group of every segment, groups, grid)
LAYOUTS = {
    'n1': (1, [1], [0], _groups(1), 0),
    'n3': (3, [3], [0], _groups(2)[1:], 0),
    'n5_cut1': (5, [1, 5], [0, 1], _groups(2), 0),
    # cuts inside a float4 and one element either side of a sweep edge (1024 elements = 256 float4); the n & 3 tail is a group of its own
    'n4099': (4099, [1, 2, 1023, 1025, 2048, 4097, 4099], [0, 1, 2, 0, 1, 2, 3], _groups(4), 0),
    'seg700': (sum(_lengths_700()), _cum(_lengths_700()), [s % 16 for s in range(700)], _groups(16), 0),
    'stride_grid2': (6149, [1000, 2049, 3001, 5121, 6149], [0, 1, 2, 1, 0], _groups(3), 2),
    'mixed': (2053, [7, 1030, 2050, 2053], [0, 1, 2, 3], _groups(4, decoupled=(1, 3)), 0),
}


def _buffers(n, seed):
    """w, m, v and three gradients as fp32 arrays: wide magnitudes, +-0 and denormals scattered in; v >= 0"""
    w, m = contract_inputs(n, seed)
    v, g0 = contract_inputs(n, seed + 1)
    g1, g2 = contract_inputs(n, seed + 2)
    return w, m, np.abs(v), [g0, g1, g2]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


class Table:
    def __init__(self, ends, gids):
        self.nseg = len(ends)
        self.host_ends = (ctypes.c_int64 * len(ends))(*[int(e) for e in ends])
        self.host_gids = (ctypes.c_uint8 * len(gids))(*[int(k) for k in gids])
        self.ends = torch.tensor([int(e) for e in ends], dtype=torch.int64).cuda()
        self.gids = torch.tensor([int(k) for k in gids], dtype=torch.uint8).cuda()


def _hp(groups, step, grad_scale, n_groups=None):
    from efgh_amd import _C
    hp = _C.AdamGroups()
    hp.n_groups = len(groups) if n_groups is None else n_groups
    hp.step, hp.grad_scale, hp.beta1, hp.beta2, hp.eps = step, grad_scale, BETAS[0], BETAS[1], EPS
    for k, g in enumerate(groups[:16]):
        hp.lr[k], hp.weight_decay[k], hp.decoupled[k] = g['lr'], g['weight_decay'], 1 if g['decoupled'] else 0
        hp.decay[k] = 1.0 - g['lr'] * g['weight_decay']
    return hp


def _launch(w, g, m, v, n, table, hp, state=None, grid=0, w_ptr=None):
    from efgh_amd import _C
    return _C.lib().efgh_adam_step_groups(w.data_ptr() if w_ptr is None else w_ptr, g.data_ptr(), m.data_ptr(), v.data_ptr(), n,
                                          table.ends.data_ptr(), table.gids.data_ptr(), table.nseg, table.host_ends, table.host_gids,
                                          ctypes.byref(hp), state.data_ptr() if state is not None else None, grid, _C.stream_ptr())


class Guard:
    """the guard's state block over the whole gradient, as train.FusedAdam drives it"""

    def __init__(self, n, max_norm, skip_nonfinite=False):
        from efgh_amd import _C
        self.n, self.max_norm, self.skip = n, max_norm, int(skip_nonfinite)
        self.bounds = (ctypes.c_int64 * 2)(0, n)
        self.state = torch.zeros(ctypes.sizeof(_C.GuardState), dtype=torch.uint8, device='cuda')
        self.ws = torch.empty(_C.lib().efgh_grad_guard_workspace(n), dtype=torch.uint8, device='cuda')

    def measure(self, g, step, grad_scale):
        from efgh_amd import _C
        _C.check(_C.lib().efgh_grad_guard_measure(g.data_ptr(), self.n, self.bounds, 1, self.max_norm, grad_scale, self.skip,
                                                  BETAS[0], BETAS[1], step, self.ws.data_ptr(), self.state.data_ptr(), 0,
                                                  _C.stream_ptr()))

    def read(self):
        from efgh_amd import _C
        return _C.GuardState.from_buffer_copy(self.state.cpu().numpy().tobytes())


def _parent_segment(w, g, m, v, a, e, group, step, grad_scale, state):
    """the ungrouped kernel on fresh aligned copies of [a, e) -> (w, m, v) of the segment"""
    from efgh_amd import _C
    ws, gs, ms, vs = (t[a:e].clone() for t in (w, g, m, v))
    assert all(t.data_ptr() % 16 == 0 for t in (ws, gs, ms, vs))
    wd = group['weight_decay']
    if group['decoupled']:
        ws.mul_(float(np.float32(1.0 - group['lr'] * group['weight_decay'])))
        wd = 0.0
    lib = _C.lib()
    if state is None:
        _C.check(lib.efgh_adam_step(_C.ptr(ws), _C.ptr(gs), _C.ptr(ms), _C.ptr(vs), _C.c_int64(e - a), _C.c_float(group['lr']),
                                    _C.c_float(BETAS[0]), _C.c_float(BETAS[1]), _C.c_float(EPS), _C.c_float(wd),
                                    _C.c_int32(step), _C.c_float(grad_scale), _C.stream_ptr()))
    else:
        _C.check(lib.efgh_adam_step_guarded(ws.data_ptr(), gs.data_ptr(), ms.data_ptr(), vs.data_ptr(), e - a, group['lr'], BETAS[0],
                                            BETAS[1], EPS, wd, state.data_ptr(), _C.stream_ptr()))
    return ws, ms, vs


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('layout', sorted(LAYOUTS))
def test_every_segment_holds_the_ungrouped_kernels_bits(layout, mode):
    n, ends, gids, groups, grid = LAYOUTS[layout]
    groups = [dict(g) for g in groups]
    table = Table(ends, gids)
    w0, m0, v0, grads = _buffers(n, 7 + len(ends))
    w, m, v = _dev(w0), _dev(m0), _dev(v0)                    # the grouped launch's buffers
    we, me, ve = w.clone(), m.clone(), v.clone()              # the yardstick's: every segment through the ungrouped kernel
    guard = None if mode == 'plain' else Guard(n, float('inf') if mode == 'measure' else 1.0)
    grad_scale = 0.5
    starts = [0] + list(ends[:-1])
    for step in (1, 2, 3):
        if step == 3:                                         # a learning rate written between two steps
            groups[len(groups) // 2]['lr'] *= 0.3
        g = _dev(grads[step - 1])
        state = None
        if guard is not None:
            guard.measure(g, step, grad_scale)
            state = guard.state
        assert _launch(w, g, m, v, n, table, _hp(groups, step, grad_scale), state, grid) == 0
        for a, e, k in zip(starts, ends, gids):
            a, e = int(a), int(e)
            ws, ms, vs = _parent_segment(we, g, me, ve, a, e, groups[k], step, grad_scale, state)
            we[a:e], me[a:e], ve[a:e] = ws, ms, vs
        torch.cuda.synchronize()
        for name, got, want in (('w', w, we), ('m', m, me), ('v', v, ve)):
            bad = np.nonzero(_bits(got) != _bits(want))[0]
            print('%s %s step %d %s: %d of %d elements differ' % (layout, mode, step, name, bad.size, n))
            assert bad.size == 0, (name, step, bad[:8].tolist())
    if mode == 'clip':                                        # the clip was a real one wherever the last gradient's norm exceeds 1
        norm = float(np.sqrt((grads[2].astype(np.float64) ** 2).sum())) * grad_scale
        assert (guard.read().coef < 1.0) == (norm + 1e-6 > 1.0)
        assert norm > 1.0 or n < 1000                         # (magnitudes up to 1e18: every layout but the tiny ones clips)


def test_a_skipped_step_leaves_every_group_untouched():
    n, ends, gids, groups, grid = LAYOUTS['n4099']
    table = Table(ends, gids)
    w0, m0, v0, grads = _buffers(n, 3)
    w, m, v = _dev(w0), _dev(m0), _dev(v0)
    guard = Guard(n, float('inf'), skip_nonfinite=True)
    good = _dev(grads[0])
    guard.measure(good, 0, 1.0)
    assert _launch(w, good, m, v, n, table, _hp(groups, 0, 1.0), guard.state) == 0
    torch.cuda.synchronize()
    st = guard.read()
    assert st.applied == 1 and st.skip == 0 and (_bits(w) != w0.view(np.int32)).any()
    before = [_bits(t).copy() for t in (w, m, v)]
    bad = grads[1].copy()
    bad[2048] = np.nan
    bad = _dev(bad)
    guard.measure(bad, 0, 1.0)
    assert _launch(w, bad, m, v, n, table, _hp(groups, 0, 1.0), guard.state) == 0
    torch.cuda.synchronize()
    st = guard.read()
    assert st.skip == 1 and st.applied == 1 and st.skipped == 1
    for t, b in zip((w, m, v), before):
        assert (_bits(t) == b).all()


def test_argument_errors_launch_nothing():
    n, ends, gids, groups, grid = LAYOUTS['n4099']
    w0, m0, v0, grads = _buffers(n + 4, 5)
    w, m, v, g = _dev(w0), _dev(m0), _dev(v0), _dev(grads[0])
    before = [_bits(t).copy() for t in (w, m, v)]
    good = Table(ends, gids)
    unsorted = list(ends)
    unsorted[2], unsorted[3] = unsorted[3], unsorted[2]
    cases = {
        'unsorted ends': (Table(unsorted, gids), _hp(groups, 1, 1.0), None),
        'last end != n': (Table(ends[:-1] + [n - 1], gids), _hp(groups, 1, 1.0), None),
        'group id out of range': (Table(ends, gids[:-1] + [len(groups)]), _hp(groups, 1, 1.0), None),
        '17 groups': (good, _hp(groups, 1, 1.0, n_groups=17), None),
        'misaligned buffer': (good, _hp(groups, 1, 1.0), w.data_ptr() + 4),
    }
    for name, (table, hp, w_ptr) in cases.items():
        assert _launch(w, g, m, v, n, table, hp, None, 0, w_ptr) == -1, name
    torch.cuda.synchronize()
    for t, b in zip((w, m, v), before):
        assert (_bits(t) == b).all()
    assert _launch(w, g, m, v, n, good, _hp(groups, 1, 1.0)) == 0           # the same call with a valid table goes through
    torch.cuda.synchronize()
    assert (_bits(w)[:n] != before[0][:n]).any()
