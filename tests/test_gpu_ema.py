"""Weight average on the GPU: efgh_ema_update against the float64 recipe (tests/ema_contract.py) within the one-step bound derived
there, efgh_ema_swap bit for bit, the refusals, and Trainer(ema_decay=) on the small configuration of tests/test_gpu_train.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from efgh_amd import _C, ops, synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_contract as contract  # noqa: E402
from train_harness import (NAN, RAW, SpoilOnCall as _SpoilOnCall, bits as _bits, census, eval_forward, mb as _mb, step as _step,  # noqa: E402,F401
                           trainer, waits_for_nothing, world)

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1000003]
SETTINGS = [(0.999, 1), (0.999, 5), (0.999, 10 ** 5), (0.5, 10 ** 3), (0.9999, 10 ** 6)]
GUARD = 8


def _boxed(x):
    """x (numpy fp32) on the device with GUARD elements of a fixed bit pattern behind it -> (whole buffer, its first len(x))"""
    buf = torch.empty(len(x) + GUARD, dtype=torch.float32, device='cuda')
    buf[:len(x)].copy_(torch.from_numpy(x))
    buf[len(x):].view(torch.int32).fill_(0x7fc0beef)
    return buf, buf[:len(x)]


def _guard_ok(buf, n):
    return bool((buf[n:].view(torch.int32) == 0x7fc0beef).all())


def _raw_update(ema, w, n, decay=0.999, warmup=1, step=1, state=None):
    return _C.lib().efgh_ema_update(ema.data_ptr(), w.data_ptr(), n, decay, warmup, step,
                                    state.data_ptr() if state is not None else 0, _C.stream_ptr())


def _raw_swap(a, b, n):
    return _C.lib().efgh_ema_swap(a.data_ptr(), b.data_ptr(), n, _C.stream_ptr())


def _state(applied, skip):
    st = _C.GuardState()
    st.applied, st.skip = applied, skip
    return torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8).cuda()


def _within(got, e, w, d, tag):
    """every element of `got` (numpy fp32) within the one-step bound of the float64 recipe from (e, w)"""
    want, tol = contract.update(e, w, d), contract.bound(e, w, d)
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / tol).max())
    print(tag, 'worst |err| / bound = %.5f' % ratio)
    assert np.isfinite(got).all() and ratio <= 1.0, (tag, ratio, int(np.argmax(err / tol)))


@pytest.mark.parametrize('n', SIZES)
def test_update_follows_the_recipe(n):
    e, w = contract.inputs(n, seed=n % 997)
    assert np.isfinite(e).all() and np.isfinite(w).all()
    wd = torch.from_numpy(w).cuda()
    for decay, t in SETTINGS:
        buf, ema = _boxed(e)
        assert _raw_update(ema, wd, n, decay, 1, t) == 0
        got = ema.cpu().numpy()
        _within(got, e, w, contract.decay_at(decay, True, t), 'n=%d decay=%g t=%d' % (n, decay, t))
        assert _guard_ok(buf, n)
        buf2, ema2 = _boxed(e)                                                   # the same launch again: the same bits
        assert _raw_update(ema2, wd, n, decay, 1, t) == 0
        assert torch.equal(_bits(buf), _bits(buf2))
    # a NaN in w at one index: a NaN in ema there and nowhere else; every other element as without it
    k = n // 2
    wn = w.copy()
    wn[k] = np.nan
    buf3, ema3 = _boxed(e)
    assert _raw_update(ema3, torch.from_numpy(wn).cuda(), n, *SETTINGS[-1][:1], 1, SETTINGS[-1][1]) == 0
    got3 = ema3.cpu().numpy()
    assert np.isnan(got3[k]) and int(np.isnan(got3).sum()) == 1 and _guard_ok(buf3, n)
    keep = np.arange(n) != k
    assert np.array_equal(got3[keep].view(np.int32), got[keep].view(np.int32))


@pytest.mark.parametrize('n', [257, 1025, 1000003])
def test_equal_buffers_are_a_fixed_point(n):
    e, _ = contract.inputs(n, seed=3)
    buf, ema = _boxed(e)
    assert _raw_update(ema, torch.from_numpy(e).cuda(), n, 0.999, 1, 7) == 0
    got = ema.cpu().numpy()
    assert np.array_equal(got, e)                                                # values (-0 == +0)
    not_negzero = e.view(np.int32) != np.int32(-2 ** 31)
    assert (~not_negzero).any() and np.array_equal(got.view(np.int32)[not_negzero], e.view(np.int32)[not_negzero])
    assert _guard_ok(buf, n)


def test_state_block_decides_the_count_and_the_skip():
    n = 1025
    e, w = contract.inputs(n, seed=11)
    wd = torch.from_numpy(w).cuda()
    wn = w.copy()
    wn[[0, 500, n - 1]] = np.nan
    # skip = 1: bit-unchanged, also with NaN in w
    for src in (w, wn):
        buf, ema = _boxed(e)
        before = _bits(buf)
        assert _raw_update(ema, torch.from_numpy(src).cuda(), n, 0.999, 1, 1000, _state(3, 1)) == 0
        assert torch.equal(before, _bits(buf))
    # skip = 0, applied = 3, host step 1000: the device count is the one used, d = 4 / 13
    buf, ema = _boxed(e)
    assert _raw_update(ema, wd, n, 0.999, 1, 1000, _state(3, 0)) == 0
    got = ema.cpu().numpy()
    assert contract.decay_at(0.999, True, 3) == np.float32(4.0 / 13.0)
    _within(got, e, w, np.float32(4.0 / 13.0), 'state applied=3')
    far = contract.update(e, w, contract.decay_at(0.999, True, 1000))            # ... and not the host's 1000
    assert float((np.abs(got - far) / contract.bound(e, w, np.float32(4.0 / 13.0))).max()) > 1e3
    # state = NULL, step = 3: the same bits
    buf2, ema2 = _boxed(e)
    assert _raw_update(ema2, wd, n, 0.999, 1, 3) == 0
    assert torch.equal(_bits(buf), _bits(buf2))
    # warmup = 0: d = decay at t = 1
    buf3, ema3 = _boxed(e)
    assert _raw_update(ema3, wd, n, 0.999, 0, 1) == 0
    _within(ema3.cpu().numpy(), e, w, contract.decay_at(0.999, False, 1), 'no warm-up')
    assert not torch.equal(_bits(buf3), _bits(buf))
    # through the wrapper, with the state tensor
    buf4, ema4 = _boxed(e)
    ops.ema_update(ema4, wd, 0.999, True, 0, _state(3, 0))
    assert torch.equal(_bits(buf4), _bits(buf))


def test_refusals_launch_nothing():
    n = 1024
    e, w = contract.inputs(n + 8, seed=5)
    x, y = torch.from_numpy(e).cuda(), torch.from_numpy(w).cuda()
    bx, by = _bits(x), _bits(y)
    lib = _C.lib()

    def refused(rc):
        torch.cuda.synchronize()
        assert rc == -1 and b'invalid argument' in lib.efgh_last_error()
        assert torch.equal(bx, _bits(x)) and torch.equal(by, _bits(y))

    refused(_raw_update(x, x, n))                                                # ema == w
    refused(_raw_update(x[:n], x[4:], n))                                        # overlapping slices (both 16-byte aligned)
    refused(_raw_update(x[4:], x[:n], n))
    refused(_raw_update(x[1:], y, n))                                            # misaligned pointers
    refused(_raw_update(x, y[2:], n))
    for decay in (0.0, 1.0, NAN, -0.5, 1.5):
        refused(_raw_update(x, y, n, decay))
    refused(_raw_update(x, y, 0))                                                # n = 0
    refused(_raw_update(x, y, -4))
    refused(_raw_update(x, y, n, 0.999, 1, 0))                                   # state = NULL with step = 0
    refused(lib.efgh_ema_update(0, y.data_ptr(), n, 0.999, 1, 1, 0, _C.stream_ptr()))
    refused(lib.efgh_ema_update(x.data_ptr(), 0, n, 0.999, 1, 1, 0, _C.stream_ptr()))
    st = torch.zeros(ctypes.sizeof(_C.GuardState) + 8, dtype=torch.uint8, device='cuda')
    refused(_raw_update(x, y, n, 0.999, 1, 1, st[4:]))                           # state not 8-byte aligned
    refused(_raw_swap(x, x, n))
    refused(_raw_swap(x[:n], x[4:], n))
    refused(_raw_swap(x[1:], y, n))
    refused(_raw_swap(x, y[3:], n))
    refused(_raw_swap(x, y, 0))
    refused(lib.efgh_ema_swap(0, y.data_ptr(), n, _C.stream_ptr()))
    refused(lib.efgh_ema_swap(x.data_ptr(), 0, n, _C.stream_ptr()))
    # the wrappers raise instead of passing a bad pointer down
    for call in (lambda: ops.ema_update(x, x, 0.999, True, 1), lambda: ops.ema_update(x[:n], x[4:], 0.999, True, 1),
                 lambda: ops.ema_update(x[1:], y[1:], 0.999, True, 1), lambda: ops.ema_update(x, y, 1.0, True, 1),
                 lambda: ops.ema_update(x, y, NAN, True, 1), lambda: ops.ema_update(x, y, 0.999, True, 0),
                 lambda: ops.ema_update(x, y[:n], 0.999, True, 1), lambda: ops.ema_update(x, y.double(), 0.999, True, 1),
                 lambda: ops.ema_update(x, y.cpu(), 0.999, True, 1), lambda: ops.ema_update(x, y, 0.999, True, 1, st.cpu()),
                 lambda: ops.ema_update(x.view(2, -1)[:, :8], y.view(2, -1)[:, :8], 0.999, True, 1),
                 lambda: ops.ema_swap(x, x), lambda: ops.ema_swap(x[:n], x[4:]), lambda: ops.ema_swap(x[1:], y[1:]),
                 lambda: ops.ema_swap(x, y[:n]), lambda: ops.ema_swap(x, y.cpu()), lambda: ops.ema_swap(x, y.half())):
        with pytest.raises(_C.EfghError):
            call()
    torch.cuda.synchronize()
    assert torch.equal(bx, _bits(x)) and torch.equal(by, _bits(y))


@pytest.mark.parametrize('n', SIZES)
def test_swap_exchanges_bits(n):
    rs = np.random.RandomState(n % 991)
    a = rs.randint(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)        # any bit pattern: NaN payloads, denormals, ...
    b = rs.randint(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    special = np.array([0x7fc00001, 0x7f800000, -0x00800000, -2 ** 31, 0x7fa12345, -0x00345678], dtype=np.int64).astype(np.int32)
    a[:min(n, 6)] = special[:min(n, 6)]                                          # quiet / signalling NaN payloads, +-inf, -0
    b[max(0, n - 6):] = special[:n - max(0, n - 6)]
    bufa, da = _boxed(a.view(np.float32))
    bufb, db = _boxed(b.view(np.float32))
    assert _raw_swap(da, db, n) == 0
    assert np.array_equal(da.cpu().numpy().view(np.int32), b) and np.array_equal(db.cpu().numpy().view(np.int32), a)
    assert _guard_ok(bufa, n) and _guard_ok(bufb, n)
    ops.ema_swap(da, db)                                                         # twice is the identity
    assert np.array_equal(da.cpu().numpy().view(np.int32), a) and np.array_equal(db.cpu().numpy().view(np.int32), b)
    assert _guard_ok(bufa, n) and _guard_ok(bufb, n)


# ---- Trainer, small configuration of tests/test_gpu_train.py (tests/train_harness.py) ----
def _trainer(world, bad_calls=(), **kw):
    return trainer(world, bad_calls, forward_names=True, **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _three_steps(tr, world):
    """three steps; per step the returned losses and (average before, weights after, average after, Adam's count) from the device"""
    out = {'tr': tr, 'losses': [], 'trace': []}
    for i in range(3):
        prev = _np(tr.ema.buf) if tr.ema is not None else None
        losses, _ = _step(tr, world, i)
        out['losses'].append({k: v.detach().clone() for k, v in losses.items() if torch.is_tensor(v)})
        if tr.ema is not None:
            out['trace'].append((prev, _np(tr.flat.w), _np(tr.ema.buf), tr.opt.t))
    out.update(w=tr.flat.w.clone(), m=tr.opt.m.clone(), v=tr.opt.v.clone())
    return out


@pytest.fixture(scope='module')
def plain_run(world):
    return _three_steps(_trainer(world), world)


@pytest.fixture(scope='module')
def ema_run(world):
    tr = _trainer(world, ema_decay=0.999)
    start_equal = torch.equal(_bits(tr.ema.buf), _bits(tr.flat.w)) and tr.ema.buf.data_ptr() != tr.flat.w.data_ptr()
    out = _three_steps(tr, world)
    out['start_equal'] = start_equal
    return out


def test_the_average_does_not_disturb_training(plain_run, ema_run):
    p, e = plain_run, ema_run
    assert p['tr'].ema is None and not hasattr(p['tr'].ema, 'buf')
    assert e['start_equal'] and e['tr'].ema.buf.numel() == e['tr'].flat.n
    for k in ('w', 'm', 'v'):
        assert torch.equal(_bits(p[k]), _bits(e[k])), k
    for lp, le in zip(p['losses'], e['losses']):
        assert list(lp) == list(le) and 'total' in lp
        for k in lp:
            assert torch.equal(lp[k].view(torch.int32), le[k].view(torch.int32)), k


def test_every_step_follows_the_recipe(ema_run):
    assert [t for _, _, _, t in ema_run['trace']] == [1, 2, 3]
    for prev, w, now, t in ema_run['trace']:
        d = contract.decay_at(0.999, True, t)
        _within(now, prev, w, d, 'trainer step %d (d = %.6f)' % (t, float(d)))
        assert float(np.abs(now - prev).max()) > 0 and float(np.abs(now - w).max()) > 0


def test_update_adds_no_aten_op_and_no_host_wait(world, plain_run, ema_run):
    # (placed ahead of the tests that take the averaging trainer through accumulated steps, eval forwards and checkpoints: here both
    # trainers have the same history, three plain steps, so the two counts compare like with like)
    plain, avg = plain_run['tr'], ema_run['tr']
    for tr in (plain, avg):
        _step(tr, world, 0)
    c_plain, c_avg = census(lambda: _step(plain, world, 0)), census(lambda: _step(avg, world, 0))
    n_plain, n_avg = sum(c_plain.values()), sum(c_avg.values())
    print('aten ops per step: %d without the average, %d with it; more with it: %s' % (n_plain, n_avg, dict(c_avg - c_plain)))
    assert n_avg <= n_plain, (n_avg, n_plain, dict(c_avg - c_plain))
    assert sum(census(lambda: avg.ema.update(avg.opt)).values()) == 0
    waits_for_nothing(lambda: avg.ema.update(avg.opt))


@pytest.mark.parametrize('route', ['gradient', 'forward_veto'])
def test_a_skipped_step_is_not_averaged(world, route):
    if route == 'gradient':
        tr = _trainer(world, bad_calls=(2,), skip_nonfinite=True, ema_decay=0.999)
    else:
        tr = _trainer(world, skip_nonfinite=True, transactional=True, ema_decay=0.999)
        tr.criterion = _SpoilOnCall(tr.criterion, tr.model, tr.txn.names[77], 2)
    _step(tr, world, 0)
    before, w1 = _bits(tr.ema.buf), _bits(tr.flat.w)
    _step(tr, world, 1)
    s = tr.guard_stats()
    assert (s['skipped'], s['applied']) == (1, 1)
    if route == 'forward_veto':
        assert (s['nonfinite'], s['vetoed'], s['rolled_back']) == (0, 1, 1)      # a finite gradient, vetoed by the forward alone
    else:
        assert s['nonfinite'] > 0
    assert torch.equal(before, _bits(tr.ema.buf)) and torch.equal(w1, _bits(tr.flat.w))
    prev = _np(tr.ema.buf)
    _step(tr, world, 2)
    assert tr.guard_stats()['applied'] == 2 and tr.opt.t == 2
    # the un-advanced count: d = 3 / 12, not 4 / 13
    _within(_np(tr.ema.buf), prev, _np(tr.flat.w), contract.decay_at(0.999, True, 2), route + ': the step after the skipped one')
    assert contract.decay_at(0.999, True, 2) == np.float32(0.25)


def test_an_accumulated_step_moves_the_average_once(world, ema_run):
    tr = ema_run['tr']
    t0 = tr.opt.t
    prev = _np(tr.ema.buf)
    tr.step_accumulated([_mb(world, i) for i in range(3)])
    assert tr.opt.t == t0 + 1
    _within(_np(tr.ema.buf), prev, _np(tr.flat.w), contract.decay_at(0.999, True, t0 + 1), 'accumulated step, t = %d' % (t0 + 1))
    assert float(np.abs(_np(tr.ema.buf) - prev).max()) > 0


def _same_outputs(a, b):
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    return list(a) == list(b) and all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


def test_the_scope_puts_the_averaged_weights_under_the_model(world, ema_run):
    from efgh_amd.nets import EFGHBackbone
    tr = ema_run['tr']
    live = eval_forward(tr.model, world)                                        # (packs and folds the LIVE weights)
    w, e = _bits(tr.flat.w), _bits(tr.ema.buf)
    sd = tr.ema_state_dict()
    now = tr.model.state_dict()
    assert len(sd) == 637 and list(sd) == list(now) and all(sd[k].shape == now[k].shape for k in now)
    trainable = {k for k, p in tr.model.named_parameters() if p.requires_grad}
    assert len(trainable) == 353
    for k in now:
        if k in trainable:
            assert sd[k].data_ptr() != now[k].data_ptr()
        else:
            assert torch.equal(sd[k], now[k]), k
    assert torch.equal(torch.cat([sd[k].reshape(-1) for k, p in tr.model.named_parameters() if p.requires_grad]), tr.ema.buf)
    fresh = EFGHBackbone(syn.default_args(RAW, 'cuda'))
    fresh.load_state_dict(sd, strict=True)
    want = eval_forward(fresh.cuda(), world)
    assert not _same_outputs(live, want)                                         # the average is a different model
    with tr.ema_weights():
        assert torch.equal(_bits(tr.flat.w), e) and torch.equal(_bits(tr.ema.buf), w)
        inside = eval_forward(tr.model, world)                                  # a missed epoch bump would leave stale packed weights
        with pytest.raises(_C.EfghError):
            _step(tr, world, 0)
        with pytest.raises(_C.EfghError):
            tr.step_accumulated([_mb(world, 0)])
        with pytest.raises(_C.EfghError):
            with tr.ema_weights():
                pass
    assert _same_outputs(inside, want)
    assert torch.equal(_bits(tr.flat.w), w) and torch.equal(_bits(tr.ema.buf), e)
    assert _same_outputs(eval_forward(tr.model, world), live)
    with pytest.raises(KeyError):                                                # an exception inside the scope still swaps back
        with tr.ema_weights():
            raise KeyError('x')
    assert torch.equal(_bits(tr.flat.w), w) and torch.equal(_bits(tr.ema.buf), e)
    assert _same_outputs(eval_forward(tr.model, world), live)
    tr.model.train()


def test_checkpoint_round_trip(world, ema_run, plain_run, tmp_path):
    from efgh_amd.io import checkpoint as ck
    from efgh_amd.nets import EFGHBackbone
    tr = ema_run['tr']
    with pytest.raises(_C.EfghError, match='ema_decay='):
        plain_run['tr'].ema_state_dict()
    with pytest.raises(_C.EfghError, match='ema_decay='):
        with plain_run['tr'].ema_weights():
            pass
    with_avg = ck.save_checkpoint(str(tmp_path / 'a'), tr.model, tr.opt, tr.it - 1, 0.0, ema=tr.ema)
    without = ck.save_checkpoint(str(tmp_path / 'b'), tr.model, tr.opt, tr.it - 1, 0.0)
    saved = torch.load(with_avg, map_location='cpu', weights_only=False)
    assert sorted(saved) == ['ema', 'iter', 'min_loss', 'optimizer', 'state_dict'] and len(saved['ema']['state_dict']) == 353
    assert sorted(torch.load(without, map_location='cpu', weights_only=False)) == ['iter', 'min_loss', 'optimizer', 'state_dict']
    new = _trainer(world, ema_decay=0.999)
    assert new.load_checkpoint(with_avg) == tr.it
    for a, b in ((new.ema.buf, tr.ema.buf), (new.flat.w, tr.flat.w), (new.opt.m, tr.opt.m), (new.opt.v, tr.opt.v)):
        assert torch.equal(_bits(a), _bits(b))
    assert new.it == tr.it and new.opt.t == tr.opt.t
    assert not torch.equal(_bits(new.ema.buf), _bits(new.flat.w))
    new.load_checkpoint(without)                                                 # no average in the file: a copy of the loaded weights
    assert torch.equal(_bits(new.ema.buf), _bits(new.flat.w)) and torch.equal(_bits(new.flat.w), _bits(tr.flat.w))
    # the reference's layout with the averaged parameters: a strict load into a fresh backbone
    ref = ck.ema_checkpoint(saved)
    assert sorted(ref) == ['iter', 'min_loss', 'optimizer', 'state_dict'] and len(ref['state_dict']) == 637
    fresh = EFGHBackbone(syn.default_args(RAW, 'cuda'))
    ck.load_model_state(fresh, ref, strict=True)
    want = tr.ema_state_dict()
    got = fresh.state_dict()
    assert list(got) == list(want)
    for k in want:
        a, b = got[k], want[k].cpu()
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k


def test_example_loop_validates_both_sets_of_weights():
    """examples/train_synthetic.py --ema 0.9: the error meter on the live weights and inside ema_weights()"""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'train_synthetic.py')
    spec = importlib.util.spec_from_file_location('train_synthetic_ema', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hist, live, averaged = mod.main(['--iters', '2', '--batch', '2', '--ema', '0.9', '--raw', '128', '256', '--points', '2048'])
    assert len(hist) == 2 and all(np.isfinite(h) for h in hist)
    assert live and list(live) == list(averaged) and all(np.isfinite(float(v)) for v in list(live.values()) + list(averaged.values()))
