"""Transactional BatchNorm state on the GPU: the three efgh_txn_* launches against the numpy contract (tests/txn_contract.py), and
Trainer(skip_nonfinite=True, transactional=True) on the small configuration of tests/test_gpu_grad_guard.py - a skipped step is all
or nothing, a non-finite forward is seen and undone, accumulation, no side effects on clean steps, census, checkpoint."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from efgh_amd import _C, synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import txn_contract as contract  # noqa: E402
from train_harness import (INF, NAN, RAW, SpoilOnCall as _SpoilOnCall, batch, census, eval_forward, make_world, step as _step,  # noqa: E402
                           trainer as _trainer, waits_for_nothing)

pytestmark = pytest.mark.gpu
GS, TS = ctypes.sizeof(_C.GuardState), ctypes.sizeof(_C.TxnState)


# ---------------------------------------------------------------- 1. kernels against the contract
def _starts(n):
    """[0, n) cut into buffers of lengths 3, 32, 61, 3, ...: the starts are not 16-byte aligned"""
    s, i = [0], 0
    while s[-1] < n:
        s.append(min(n, s[-1] + (3, 32, 61)[i % 3]))
        i += 1
    return s


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _block(cls, t):
    return cls.from_buffer_copy(t.cpu().numpy().tobytes())


def _i32(t):
    return t.detach().clone().view(torch.int32)


def _snapshot(live, shadow, lc, sc, txn):
    _C.check(_C.lib().efgh_txn_snapshot(live.data_ptr(), shadow.data_ptr(), live.numel(), lc.data_ptr(), sc.data_ptr(), lc.numel(),
                                        txn.data_ptr(), _C.stream_ptr()))


def _probe(live, shadow, starts, txn, losses=None, k=0, stride=1):
    _C.check(_C.lib().efgh_txn_probe(live.data_ptr(), shadow.data_ptr(), live.numel(), starts.data_ptr(), starts.numel() - 1,
                                     losses.data_ptr() if k else 0, k, stride, txn.data_ptr(), _C.stream_ptr()))


def _resolve(live, shadow, lc, sc, guard, txn):
    _C.check(_C.lib().efgh_txn_resolve(live.data_ptr(), shadow.data_ptr(), live.numel(), lc.data_ptr(), sc.data_ptr(), lc.numel(),
                                       guard.data_ptr(), txn.data_ptr(), 0.9, 0.999, _C.stream_ptr()))


def _measure(g, state, skip=1):
    lib = _C.lib()
    n = g.numel()
    ws = torch.full((lib.efgh_grad_guard_workspace(n),), 255, dtype=torch.uint8, device='cuda')
    arr = (ctypes.c_int64 * 2)(0, n)
    _C.check(lib.efgh_grad_guard_measure(g.data_ptr(), n, arr, 1, INF, 1.0, skip, 0.9, 0.999, 0, ws.data_ptr(), state.data_ptr(), 0,
                                         _C.stream_ptr()))


def _guard_state(applied, skipped):
    st = torch.zeros(GS, dtype=torch.uint8, device='cuda')
    for field, v in ((_C.GuardState.applied, applied), (_C.GuardState.skipped, skipped)):
        st[field.offset:field.offset + 8].view(torch.int64).fill_(v)
    return st


def _planted(n, starts, seed):
    """-> (live, shadow): shadow finite except ONE element that is NaN in both (must not count); live = shadow with +inf, -inf and
    NaN at the first element, the last element and both sides of a buffer boundary (where n has room for them)"""
    rs = np.random.RandomState(seed)
    shadow = rs.standard_normal(n).astype(np.float32)
    live = (shadow + np.float32(0.25)).astype(np.float32)
    spots = {0, n - 1}
    if len(starts) > 2:
        b = starts[len(starts) // 2]
        spots |= {b - 1, b}
    for j, i in enumerate(sorted(spots)):
        live[i] = (INF, -INF, NAN)[j % 3]
    if n >= 5:
        old = min(i for i in range(n) if i not in spots)
        shadow[old] = live[old] = NAN
        if n > 40:
            live[33], shadow[33] = 1.0, INF                  # non-finite -> finite: not an event
    return live, shadow


@pytest.mark.parametrize('n', [1, 3, 4, 5, 255, 256, 257, 4099])
def test_kernels_follow_the_contract(n):
    starts = _starts(n)
    live_h, shadow_h = _planted(n, starts, n)
    want_count, want_first = contract.probe(live_h, shadow_h, starts)
    assert want_count == len({0, n - 1} | ({starts[len(starts) // 2] - 1, starts[len(starts) // 2]} if len(starts) > 2 else set()))
    # vectors inside larger allocations with canaries on both sides: nothing outside [0, n) may be touched
    pad = 8
    def boxed(a, dtype):
        t = torch.full((pad + len(a) + pad,), -7777, dtype=dtype, device='cuda')
        t[pad:pad + len(a)] = _dev(a)
        return t, t[pad:pad + len(a)]
    box_l, live = boxed(live_h, torch.float32)
    box_s, shadow = boxed(shadow_h, torch.float32)
    nc = 1 + n % 7
    box_lc, lc = boxed(np.arange(nc, dtype=np.int64) * 1000003 + (1 << 40), torch.int64)
    box_sc, sc = boxed(np.arange(nc, dtype=np.int64) + 5, torch.int64)
    st = _dev(np.asarray(starts, np.int64))
    txn = torch.zeros(TS, dtype=torch.uint8, device='cuda')
    keep = [t.clone() for t in (box_l, box_s, box_lc, box_sc)]

    def untouched():
        return all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(keep, (box_l, box_s, box_lc, box_sc)))

    # probe: exact count and first_bad, with two non-finite ones among four strided loss scalars; nothing else is written
    txn[_C.TxnState.first_bad.offset:_C.TxnState.first_bad.offset + 4].view(torch.int32).fill_(-1)
    losses = _dev(np.array([1.0, NAN, INF, NAN, 2.0, NAN, -INF, NAN], np.float32))      # stride 2: 1, inf, 2, -inf
    _probe(live, shadow, st, txn, losses, 4, 2)
    t = _block(_C.TxnState, txn)
    assert (t.forward_nonfinite, t.first_bad) == (want_count + 2, want_first), (n, t.forward_nonfinite, t.first_bad)
    assert (t.vetoed, t.rolled_back, t.vetoed_total) == (0, 0, 0) and untouched()
    _probe(live, shadow, st, txn)                            # the count accumulates, the minimum stays
    t = _block(_C.TxnState, txn)
    assert (t.forward_nonfinite, t.first_bad) == (2 * want_count + 2, want_first)
    if n > 1:                                                # the first element finite: first_bad names a later buffer (or none)
        live2_h = live_h.copy()
        live2_h[0] = 1.0
        if n > 40:
            live2_h[1:40] = shadow_h[1:40]                   # (nothing new in buffers 0 and 1 and the head of 2)
        c2, f2 = contract.probe(live2_h, shadow_h, starts)
        assert c2 == want_count - 1 and (f2 > 1 or n <= 40)
        txn2 = torch.zeros(TS, dtype=torch.uint8, device='cuda')
        _snapshot(live, shadow.clone(), lc, sc.clone(), txn2)                # (clears first_bad to -1)
        _probe(_dev(live2_h), shadow, st, txn2)
        t = _block(_C.TxnState, txn2)
        assert (t.forward_nonfinite, t.first_bad) == (c2, f2), (n, t.forward_nonfinite, t.first_bad, c2, f2)

    # resolve, guard applied and forward clean: nothing is written at all
    g = _dev(np.ones(7, np.float32))
    guard = _guard_state(4, 2)
    _measure(g, guard)
    txn.zero_()
    raw_guard = guard.clone()
    _resolve(live, shadow, lc, sc, guard, txn)
    assert torch.equal(guard, raw_guard) and untouched() and _block(_C.TxnState, txn).rolled_back == 0

    # resolve, the guard skipped (NaN gradient): live and the counters get the bits of shadow; the guard block stays
    guard = _guard_state(4, 2)
    _measure(_dev(np.array([1.0, NAN, 1.0], np.float32)), guard)
    raw_guard = guard.clone()
    _resolve(live, shadow, lc, sc, guard, txn)
    assert torch.equal(guard, raw_guard)
    assert torch.equal(_i32(live), _i32(shadow)) and torch.equal(lc, sc)
    assert torch.equal(_i32(shadow), _i32(_dev(shadow_h)))
    for a, b in zip(keep, (box_l, box_s, box_lc, box_sc)):   # canaries
        assert torch.equal(a[:pad], b[:pad]) and torch.equal(a[-pad:], b[-pad:])
    t = _block(_C.TxnState, txn)
    assert (t.rolled_back, t.vetoed, t.vetoed_total) == (1, 0, 0)

    # snapshot: shadow = live bit for bit, per-step fields cleared, totals kept
    live.copy_(_dev(live_h))
    lc.add_(3)
    txn[_C.TxnState.forward_nonfinite.offset:_C.TxnState.forward_nonfinite.offset + 8].view(torch.int64).fill_(9)
    _snapshot(live, shadow, lc, sc, txn)
    assert torch.equal(_i32(shadow), _i32(_dev(live_h))) and torch.equal(sc, lc) and torch.equal(_i32(live), _i32(_dev(live_h)))
    t = _block(_C.TxnState, txn)
    assert (t.forward_nonfinite, t.first_bad, t.vetoed, t.rolled_back) == (0, -1, 0, 1)
    _probe(live, shadow, st, txn)                            # nothing became non-finite since
    assert _block(_C.TxnState, txn).forward_nonfinite == 0 and _block(_C.TxnState, txn).first_bad == -1


def _bias_corrections_ok(st, t):
    """the tolerance tests/test_gpu_grad_guard.py holds the guard's bias corrections to (the power may be off by one fp32 rounding)"""
    ref1, ref2 = contract.bias_corrections(t)
    return abs(st.bc1 - ref1) <= 2.0 ** -23 and abs(st.bc2_sqrt - ref2) <= 2.0 ** -23 / (2 * float(ref2)) + 2.0 ** -24


def test_veto_rewrites_the_guard_block_as_a_skip_would():
    n = 1000
    rs = np.random.RandomState(5)
    g = _dev(rs.standard_normal(n).astype(np.float32))
    live_h, shadow_h = rs.standard_normal(300).astype(np.float32), rs.standard_normal(300).astype(np.float32)
    live, shadow = _dev(live_h), _dev(shadow_h)
    lc, sc = _dev(np.arange(9, dtype=np.int64) + 100), _dev(np.arange(9, dtype=np.int64))
    guard = _guard_state(4, 2)
    _measure(g, guard)
    before = _block(_C.GuardState, guard)
    assert (before.skip, before.applied, before.skipped, before.nonfinite_total) == (0, 5, 2, 0)
    txn = torch.zeros(TS, dtype=torch.uint8, device='cuda')
    txn[_C.TxnState.forward_nonfinite.offset:_C.TxnState.forward_nonfinite.offset + 8].view(torch.int64).fill_(3)
    _resolve(live, shadow, lc, sc, guard, txn)
    got, t = _block(_C.GuardState, guard), _block(_C.TxnState, txn)
    mirror = {k: getattr(before, k) for k in ('skip', 'applied', 'skipped', 'bc1', 'bc2_sqrt')}
    want, want_t, restore = contract.resolve(mirror, 3)
    assert restore and (got.skip, got.applied, got.skipped) == (want['skip'], want['applied'], want['skipped']) == (1, 4, 3)
    assert _bias_corrections_ok(got, 4), (got.bc1, got.bc2_sqrt)
    assert (t.vetoed, t.vetoed_total, t.rolled_back, t.forward_nonfinite) == (1, 1, 1, 3)
    assert (want_t['vetoed'], want_t['vetoed_total'], want_t['rolled_back']) == (1, 1, 1)
    for k in ('sumsq_total', 'norm', 'nonfinite_total', 'coef', 'scale', 'nseg'):                 # untouched
        assert getattr(got, k) == getattr(before, k), k
    assert list(got.sumsq) == list(before.sumsq) and list(got.nonfinite) == list(before.nonfinite)
    # ... and exactly what the decide launch leaves when it skips from the same counters
    skipped = _guard_state(4, 2)
    bad = g.clone()
    bad[17] = NAN
    _measure(bad, skipped)
    ref = _block(_C.GuardState, skipped)
    for k in ('skip', 'applied', 'skipped', 'bc1', 'bc2_sqrt'):
        assert getattr(got, k) == getattr(ref, k), (k, getattr(got, k), getattr(ref, k))
    assert torch.equal(_i32(live), _i32(shadow)) and torch.equal(lc, sc)                            # restored
    # the guarded Adam sees the veto through state->skip
    w, m, v = (_dev(rs.standard_normal(n).astype(np.float32)) for _ in range(3))
    v.abs_()
    keep = [_i32(x) for x in (w, m, v)]
    _C.check(_C.lib().efgh_adam_step_guarded(w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 0.0,
                                             guard.data_ptr(), _C.stream_ptr()))
    assert all(torch.equal(a, _i32(b)) for a, b in zip(keep, (w, m, v)))
    # a second vetoed step from applied = 0: the bias corrections of step 0, as a skip at step 0 leaves them
    guard0, ref0 = _guard_state(0, 0), _guard_state(0, 0)
    _measure(g, guard0)
    _measure(bad, ref0)
    _resolve(live, shadow, lc, sc, guard0, txn)
    got0, r0, t = _block(_C.GuardState, guard0), _block(_C.GuardState, ref0), _block(_C.TxnState, txn)
    assert [getattr(got0, k) for k in ('skip', 'applied', 'skipped', 'bc1', 'bc2_sqrt')] == \
        [getattr(r0, k) for k in ('skip', 'applied', 'skipped', 'bc1', 'bc2_sqrt')]
    assert (t.vetoed_total, t.rolled_back) == (2, 2)


# ---------------------------------------------------------------- Trainer, small configuration of tests/test_gpu_grad_guard.py
@pytest.fixture(scope='module')
def world(manifest):
    w = make_world(manifest)
    inp, gt = batch(2)
    inp[1][1, 0, 40, 100] = NAN                              # ONE NaN pixel in the second image
    w['nan'] = (inp, gt)
    return w


def _entries(tr):
    """all state_dict entries (637 for the full net) and both moments, cloned"""
    out = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    out['<m>'], out['<v>'] = tr.opt.m.clone(), tr.opt.v.clone()
    return out


def _differing(a, b):
    """keys whose bits differ"""
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    return [k for k in a if not torch.equal(bits(a[k]), bits(b[k]))]


def _counters(tr):
    return tr.flat.nbt.clone()


@pytest.fixture(scope='module')
def skip_run(world, tmp_path_factory):
    """transactional over batches 0, 1, 2 with the loss of the second step multiplied by inf; a checkpoint after the skipped step"""
    from efgh_amd.io import checkpoint as ck
    tr = _trainer(world, bad_calls=(2,), skip_nonfinite=True, transactional=True)
    c0 = _counters(tr)
    _step(tr, world, 0)
    before = _entries(tr)
    _step(tr, world, 1)
    after, stats2 = _entries(tr), tr.guard_stats()
    path = ck.save_checkpoint(str(tmp_path_factory.mktemp('txn_ckpt')), tr.model, tr.opt, tr.it, 0.0)
    _step(tr, world, 2)
    return {'tr': tr, 'before': before, 'after': after, 'stats2': stats2, 'stats3': tr.guard_stats(), 'ckpt': path, 'c0': c0,
            'c3': _counters(tr)}


@pytest.fixture(scope='module')
def clean_runs(world):
    """two clean steps (batches 0 and 2): skip_nonfinite alone, and with transactional"""
    out = {}
    for name, kw in (('guard', {}), ('txn', {'transactional': True})):
        tr = _trainer(world, skip_nonfinite=True, **kw)
        _step(tr, world, 0)
        _step(tr, world, 2)
        out[name] = {'tr': tr, 'entries': _entries(tr), 'w': tr.flat.w.clone(), 'stats': tr.guard_stats()}
    return out


def test_a_skipped_step_is_all_or_nothing(world, skip_run):
    r = skip_run
    assert len(r['before']) == 637 + 2
    assert _differing(r['before'], r['after']) == []                        # parameters, running statistics, counters, m, v
    s = r['stats2']
    assert (s['skipped'], s['applied'], s['rolled_back'], s['vetoed']) == (1, 1, 1, 0) and s['nonfinite'] > 0
    assert s['forward_nonfinite'] == 1 and s['first_bad_buffer'] is None     # the one infinite loss; no buffer was spoiled
    s = r['stats3']
    assert (s['skipped'], s['applied'], s['rolled_back'], s['forward_nonfinite']) == (1, 2, 1, 0)
    assert torch.equal(r['c3'], r['c0'] + 2)                                 # two applied forwards, 93 counters
    assert len(r['tr'].txn.names) == 186 and r['tr'].flat.nbt.numel() == 93


def test_without_the_option_the_skipped_step_leaves_its_mark(world):
    """the same run with skip_nonfinite alone: weights and moments are kept, running statistics and counters are not - what the
    option is for"""
    tr = _trainer(world, bad_calls=(2,), skip_nonfinite=True)
    _step(tr, world, 0)
    before = _entries(tr)
    _step(tr, world, 1)
    diff = _differing(before, _entries(tr))
    assert tr.guard_stats()['skipped'] == 1 and 'rolled_back' not in tr.guard_stats()
    assert diff and all(k.endswith(('running_mean', 'running_var', 'num_batches_tracked')) for k in diff)
    assert sum(k.endswith('num_batches_tracked') for k in diff) == 93
    assert any(k.endswith('running_mean') for k in diff) and any(k.endswith('running_var') for k in diff)


def test_a_nonfinite_forward_is_seen_and_undone(world, clean_runs):
    """One NaN pixel in the second image of a batch.  Measured on an MI355X when this test was written: 16 205 running statistics
    became non-finite, the first in `H.vgg.features.1.running_mean`; the gradient came out non-finite as well (37 215 058 elements),
    so the guard skipped by itself and the forward did not have to veto (test_a_finite_gradient_is_vetoed_by_a_spoiled_buffer covers
    that branch); after the following clean step 0 of the 639 entries differed in bits from the run that never saw the bad batch."""
    tr = _trainer(world, skip_nonfinite=True, transactional=True)
    _step(tr, world, 0)
    before = _entries(tr)
    e0, e1 = eval_forward(tr.model, world), eval_forward(tr.model, world)
    assert _differing(e0, e1) == []                                          # (the eval forward repeats itself bit for bit)
    _step(tr, world, 'nan')
    s = tr.guard_stats()
    print('nan step:', {k: s[k] for k in ('forward_nonfinite', 'first_bad_buffer', 'vetoed', 'nonfinite', 'skipped', 'applied')})
    assert s['forward_nonfinite'] > 0
    assert s['first_bad_buffer'] in tr.model.state_dict() and s['first_bad_buffer'].endswith(('running_mean', 'running_var'))
    assert (s['skipped'], s['applied'], s['rolled_back']) == (1, 1, 1)        # skipped, whether or not the gradient came out finite
    assert s['vetoed'] == (1 if s['nonfinite'] == 0 else 0)
    assert _differing(before, _entries(tr)) == []
    assert _differing(e0, eval_forward(tr.model, world)) == []               # the folded eval affine was rebuilt from restored values
    _step(tr, world, 2)
    assert tr.guard_stats()['applied'] == 2 and tr.guard_stats()['forward_nonfinite'] == 0
    # against the run that never saw the bad batch: the yardstick of test_trainer_skips_a_nonfinite_step, per parameter and buffer
    mine, clean = _entries(tr), clean_runs['txn']['entries']
    worst = 0.0
    for k, b in clean.items():
        if b.dtype.is_floating_point:
            d, tol = float((mine[k] - b).abs().max()), 2e-6 + 1e-5 * float(b.abs().max())
            worst = max(worst, d / tol)
            assert d <= tol, (k, d, tol)
        else:
            assert torch.equal(mine[k], b), k
    print('after the following clean step: %d of %d entries differ in bits from the clean run, worst |d| / bound = %.3g'
          % (len(_differing(mine, clean)), len(clean), worst))
    assert bool(torch.isfinite(tr.txn.live).all())


def test_a_finite_gradient_is_vetoed_by_a_spoiled_buffer(world):
    tr = _trainer(world, skip_nonfinite=True, transactional=True)
    key = tr.txn.names[77]
    tr.criterion = _SpoilOnCall(tr.criterion, tr.model, key, 2)
    _step(tr, world, 0)
    before = _entries(tr)
    w = tr.flat.w.clone().view(torch.int32)
    _step(tr, world, 1)
    s = tr.guard_stats()
    assert (s['nonfinite'], s['forward_nonfinite'], s['first_bad_buffer'], s['vetoed']) == (0, 1, key, 1)
    assert (s['skipped'], s['applied'], s['rolled_back']) == (1, 1, 1) and s['norm'] > 0 and s['coef'] == 1.0
    assert _differing(before, _entries(tr)) == [] and torch.equal(w, tr.flat.w.view(torch.int32))
    assert tr.opt.t == 1
    _step(tr, world, 2)
    s = tr.guard_stats()
    assert (s['skipped'], s['applied'], s['rolled_back'], s['vetoed'], s['forward_nonfinite']) == (1, 2, 1, 0, 0)
    assert not torch.equal(w, tr.flat.w.view(torch.int32)) and bool(torch.isfinite(tr.flat.w).all())


def test_accumulated_step_rolls_back_every_micro_batch(world):
    tr = _trainer(world, skip_nonfinite=True, transactional=True)
    before, c0 = _entries(tr), _counters(tr)
    _step(tr, world, 'nan', micro_batches=2)                                 # the NaN pixel is in the second micro-batch
    s = tr.guard_stats()
    assert s['forward_nonfinite'] > 0 and (s['skipped'], s['applied'], s['rolled_back']) == (1, 0, 1)
    assert _differing(before, _entries(tr)) == []
    assert torch.equal(c0, _counters(tr))                                    # no tick from either micro-batch
    _step(tr, world, 0, micro_batches=2)
    s = tr.guard_stats()
    assert (s['skipped'], s['applied'], s['rolled_back'], s['forward_nonfinite'], s['vetoed']) == (1, 1, 1, 0, 0)
    assert torch.equal(_counters(tr), c0 + 2)
    assert bool(torch.isfinite(tr.txn.live).all()) and bool(torch.isfinite(tr.flat.w).all())


def test_no_side_effects_when_nothing_is_wrong(clean_runs):
    a, b = clean_runs['guard'], clean_runs['txn']
    assert _differing(a['entries'], b['entries']) == []                      # 637 entries and both moments
    assert torch.equal(a['w'].view(torch.int32), b['w'].view(torch.int32))
    s = b['stats']
    assert (s['rolled_back'], s['vetoed'], s['forward_nonfinite'], s['first_bad_buffer']) == (0, 0, 0, None)
    assert (s['applied'], s['skipped']) == (2, 0) and b['tr'].txn.block.data_ptr() == b['tr'].opt.state.data_ptr() + GS
    assert a['tr'].txn is None and 'rolled_back' not in a['stats']


def test_transactional_step_adds_no_aten_ops_and_no_host_sync(world, clean_runs):
    guarded, txn = clean_runs['guard']['tr'], clean_runs['txn']['tr']
    n_guarded = sum(census(lambda: _step(guarded, world, 0)).values())
    n_txn = sum(census(lambda: _step(txn, world, 0)).values())
    assert n_txn <= n_guarded, (n_txn, n_guarded)
    t = txn.txn
    loss = torch.ones(1, device='cuda')

    def three():
        t.snapshot()
        t.probe(loss, 1, 1)
        t.resolve(txn.opt.state, txn.opt.betas)
    assert sum(census(three).values()) == 0
    waits_for_nothing(three)


def test_checkpoint_after_a_skipped_step(world, skip_run):
    from efgh_amd.io import checkpoint as ck
    from efgh_amd.nets import EFGHBackbone
    saved = torch.load(skip_run['ckpt'], map_location='cpu', weights_only=False)['state_dict']
    assert len(saved) == 637
    for k, v in saved.items():                               # the views save with their own storage, not the whole vector's
        assert v.untyped_storage().nbytes() == v.numel() * v.element_size(), k
    fresh = EFGHBackbone(syn.default_args(RAW, 'cuda'))
    ck.load_model_state(fresh, skip_run['ckpt'])
    want = {k: v.cpu() for k, v in skip_run['after'].items() if not k.startswith('<')}
    got = {k: v.detach().clone() for k, v in fresh.state_dict().items()}
    assert list(got) == list(want) and _differing(want, got) == []
    # one applied forward (the skipped step's tick was rolled back)
    nbt = torch.stack([v for k, v in saved.items() if k.endswith('num_batches_tracked')])
    assert torch.equal(nbt, skip_run['c0'].cpu() + 1)
    # ... and loading into the live, re-homed model copies in place: the transaction's views survive
    tr = skip_run['tr']
    ck.load_model_state(tr.model, skip_run['ckpt'])
    tr.txn.check()
    assert torch.equal(tr.flat.nbt, skip_run['c0'] + 1)
