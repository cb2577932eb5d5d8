"""Weight average, host side: the float64 recipe (tests/ema_contract.py) against torch's AveragedModel, the warm-up schedule, the
argument checks of Trainer / WeightEma / the ops wrappers, and the checkpoint dictionaries - on a FlatParams over a toy module on
the CPU (the plain-torch route of ops.ema_update / ops.ema_swap)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from efgh_amd import _C, ops
from efgh_amd.io import checkpoint as ck
from efgh_amd.train import FlatParams, FusedAdam, Trainer, WeightEma, check_ema_decay

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_contract as contract  # noqa: E402


def test_recipe_agrees_with_torch_averaged_model():
    """AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d)): the first update_parameters copies (the trainer's copy at construction),
    every later one is lerp(avg, p, 1 - d).  torch's lerp is not the fused form and takes 1 - d in float64: per update the two differ
    by a few fp32 roundings of values of size max|w|, bounded here by 4 * 2^-24 * max|w| per update."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    torch.manual_seed(5)
    d = 0.999
    m = torch.nn.Linear(7, 5)
    avg = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(d))
    avg.update_parameters(m)
    e64 = {k: p.detach().numpy().astype(np.float64) for k, p in m.named_parameters()}
    wmax = 0.0
    for k in range(1, 7):
        with torch.no_grad():
            for p in m.parameters():
                p.add_(torch.randn_like(p) * 0.05)
        avg.update_parameters(m)
        for name, p in m.named_parameters():
            e64[name] = contract.update(e64[name], p.detach().numpy(), contract.decay_at(d, False, k))
            wmax = max(wmax, float(p.detach().abs().max()))
        for name, p in avg.module.named_parameters():
            gap = float(np.abs(p.detach().numpy().astype(np.float64) - e64[name]).max())
            print('update', k, name, 'gap', gap, 'bound', k * 4 * 2.0 ** -24 * wmax)
            assert gap <= k * 4 * 2.0 ** -24 * wmax, (k, name, gap)
    # ... and the average did move away from both the start and the live weights
    assert all(float((p - q).detach().abs().max()) > 1e-3 for p, q in zip(avg.module.parameters(), m.parameters()))


def test_warmup_schedule():
    assert contract.decay_at(0.999, True, 1) == np.float32(2.0 / 11.0)
    assert contract.decay_at(0.999, False, 1) == np.float32(0.999)
    for decay in (0.5, 0.9, 0.999, 0.9999):
        ds = [float(contract.decay_at(decay, True, t)) for t in range(1, 200000 if decay > 0.999 else 20000)]
        assert all(a <= b for a, b in zip(ds, ds[1:]))                           # monotone
        first = next(t for t in range(1, 10 ** 6) if (1.0 + t) / (10.0 + t) >= float(np.float32(decay)))
        # (the value just before may already round to it in fp32, never beyond it)
        assert ds[first - 1] == np.float32(decay) and (first == 1 or ds[0] < ds[first - 2] <= np.float32(decay)), (decay, first)
        assert all(x == np.float32(decay) for x in ds[first - 1:])
    assert ops.ema_decay_at(0.999, True, 5) == float(contract.decay_at(0.999, True, 5))
    assert ops.ema_decay_at(0.999, True, 10 ** 5) == float(np.float32(0.999))


def _toy():
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4), torch.nn.Linear(4, 2))
    m[2].bias.requires_grad = False                                              # one frozen parameter
    return m


@pytest.mark.parametrize('bad', [True, False, float('nan'), 0, 1, 0.0, 1.0, -0.1, 1.5, '0.9', float('inf')])
def test_ema_decay_must_lie_inside_the_unit_interval(bad):
    m = _toy()
    before = [p.data_ptr() for p in m.parameters()]
    with pytest.raises(_C.EfghError, match='ema_decay'):
        Trainer(m, None, ema_decay=bad)
    assert [p.data_ptr() for p in m.parameters()] == before                      # nothing was re-homed
    with pytest.raises(_C.EfghError):
        check_ema_decay(bad)


def test_trainer_arguments_and_state_dict_on_the_cpu():
    assert check_ema_decay(None) is None and check_ema_decay(0.5) == 0.5
    off = Trainer(_toy(), None)
    assert off.ema is None
    with pytest.raises(_C.EfghError, match='ema_decay='):
        off.ema_state_dict()
    with pytest.raises(_C.EfghError, match='ema_decay='):
        with off.ema_weights():
            pass
    m = _toy()
    tr = Trainer(m, None, ema_decay=0.9, ema_warmup=False)
    assert tr.ema.decay == 0.9 and tr.ema.warmup is False and torch.equal(tr.ema.buf, tr.flat.w)
    assert tr.ema.buf.data_ptr() != tr.flat.w.data_ptr()
    live = {k: v.clone() for k, v in m.state_dict().items()}
    tr.flat.w.add_(1.0)
    tr.opt._t = 1
    tr.ema.update(tr.opt)                                                        # CPU route: lerp_
    assert torch.allclose(tr.ema.buf - (tr.flat.w - 1.0), torch.full_like(tr.flat.w, 0.1), atol=1e-6)
    sd = tr.ema_state_dict()
    now = m.state_dict()
    assert list(sd) == list(now) and all(sd[k].shape == now[k].shape for k in now)
    for k in now:
        if k == '2.bias' or 'running' in k or 'num_batches' in k:                # frozen parameter and buffers: the live values
            assert torch.equal(sd[k], now[k]) and torch.equal(now[k], live[k])
        else:
            assert torch.allclose(sd[k], live[k] + 0.1, atol=1e-6) and sd[k].data_ptr() != now[k].data_ptr()
    # the scope: in place, exchanged back after an exception, refused when nested
    w, e, n0 = tr.flat.w.clone(), tr.ema.buf.clone(), tr.flat.epoch.n
    with pytest.raises(ZeroDivisionError):
        with tr.ema_weights():
            assert torch.equal(tr.flat.w, e) and torch.equal(tr.ema.buf, w) and tr.flat.epoch.n == n0 + 1
            assert torch.equal(m[0].weight.detach().reshape(-1), e[:12])
            with pytest.raises(_C.EfghError):
                with tr.ema_weights():
                    pass
            with pytest.raises(_C.EfghError):
                tr.step(None, None, None, None, None)
            with pytest.raises(_C.EfghError):
                tr.step_accumulated([])
            1 / 0
    assert torch.equal(tr.flat.w, w) and torch.equal(tr.ema.buf, e) and tr.flat.epoch.n == n0 + 2
    tr.ema.reset()
    assert torch.equal(tr.ema.buf, tr.flat.w)


def test_ops_wrappers_check_their_arguments():
    a, b, x = torch.zeros(8), torch.ones(8), torch.ones(16)
    for bad in ((a, b.double()), (a, b[:7]), (a, x[::2]), (a, a), (a[:0], b[:0]), (x[:8], x[4:12])):
        with pytest.raises(_C.EfghError):
            ops.ema_swap(*bad)
    with pytest.raises(_C.EfghError):
        ops.ema_update(x[:8], x[4:12], 0.9, True, 1)
    for decay in (0, 1, float('nan'), True):
        with pytest.raises(_C.EfghError):
            ops.ema_update(a, b, decay, True, 1)
    for step in (0, -1, 1.0, True):
        with pytest.raises(_C.EfghError):
            ops.ema_update(a, b, 0.9, True, step)
    assert float(a.abs().max()) == 0.0 and float(b.min()) == 1.0
    ops.ema_swap(a, b)
    assert float(a.min()) == 1.0 and float(b.abs().max()) == 0.0
    ops.ema_update(b, a, 0.9, True, 1)                                           # d = 2/11
    assert torch.allclose(b, torch.full_like(b, 9.0 / 11.0), atol=1e-6)


def test_checkpoint_dictionaries(tmp_path):
    m = _toy()
    flat = FlatParams(m)
    opt = FusedAdam(flat)
    ema = WeightEma(flat, 0.75, warmup=False)
    flat.w.add_(1.0)
    opt._t = 1
    ema.update(opt)
    trainable = ['0.weight', '0.bias', '1.weight', '1.bias', '2.weight']
    plain = torch.load(ck.save_checkpoint(str(tmp_path / 'a'), m, opt, 7, 0.5), weights_only=False)
    assert sorted(plain) == ['iter', 'min_loss', 'optimizer', 'state_dict']     # exactly the reference's keys
    with pytest.raises(_C.EfghError):
        ck.ema_checkpoint(plain)
    saved = torch.load(ck.save_checkpoint(str(tmp_path / 'b'), m, opt, 7, 0.5, ema=ema), weights_only=False)
    assert sorted(saved) == ['ema', 'iter', 'min_loss', 'optimizer', 'state_dict']
    assert sorted(saved['ema']) == ['decay', 'state_dict', 'warmup']
    assert saved['ema']['decay'] == 0.75 and saved['ema']['warmup'] is False
    assert list(saved['ema']['state_dict']) == ['module.' + k for k in trainable]
    for k, v in saved['ema']['state_dict'].items():
        assert v.untyped_storage().nbytes() == v.numel() * 4 and v.shape == saved['state_dict'][k].shape
        assert torch.allclose(v, saved['state_dict'][k] - 0.75, atol=1e-6)      # w moved by 1, the average by a quarter of it
    ref = ck.ema_checkpoint(saved)
    assert sorted(ref) == ['iter', 'min_loss', 'optimizer', 'state_dict'] and ref['iter'] == 7
    assert list(ref['state_dict']) == list(saved['state_dict'])
    for k, v in ref['state_dict'].items():
        want = saved['ema']['state_dict'].get(k, saved['state_dict'][k])
        assert torch.equal(v, want), k
    assert 'ema' in saved and torch.equal(saved['state_dict']['module.0.weight'], m[0].weight.detach())      # the input is untouched
    fresh = _toy()
    ck.load_model_state(fresh, ref, strict=True)
    assert torch.equal(fresh[0].weight.detach(), ema.buf[:12].view(4, 3))
    # restoring: a round trip, then a name and a shape mismatch
    ema2 = WeightEma(flat, 0.75)
    assert not torch.equal(ema2.buf, ema.buf)
    ck.load_ema_state(ema2, m, saved['ema'])
    assert torch.equal(ema2.buf, ema.buf)
    renamed = dict(saved['ema'], state_dict={k.replace('0.weight', '0.kernel'): v for k, v in saved['ema']['state_dict'].items()})
    with pytest.raises(_C.EfghError, match='0.kernel'):
        ck.load_ema_state(ema2, m, renamed)
    reshaped = dict(saved['ema'], state_dict={k: (v.reshape(-1) if k == 'module.0.weight' else v)
                                              for k, v in saved['ema']['state_dict'].items()})
    with pytest.raises(_C.EfghError, match='shape'):
        ck.load_ema_state(ema2, m, reshaped)
    assert torch.equal(ema2.buf, ema.buf)                                        # a refused load writes nothing


def test_trainer_load_checkpoint_restores_or_resets_the_average(tmp_path):
    m = _toy()
    tr = Trainer(m, None, ema_decay=0.75, ema_warmup=False)
    tr.flat.w.add_(1.0)
    tr.opt._t = 1
    tr.ema.update(tr.opt)
    with_avg = ck.save_checkpoint(str(tmp_path / 'a'), m, tr.opt, 3, 0.0, ema=tr.ema)
    without = ck.save_checkpoint(str(tmp_path / 'b'), m, tr.opt, 3, 0.0)
    tr2 = Trainer(_toy(), None, ema_decay=0.5)
    assert tr2.load_checkpoint(with_avg) == 4
    assert torch.equal(tr2.flat.w, tr.flat.w) and torch.equal(tr2.ema.buf, tr.ema.buf) and tr2.ema.decay == 0.5
    tr3 = Trainer(_toy(), None, ema_decay=0.5)
    tr3.load_checkpoint(without)
    assert torch.equal(tr3.flat.w, tr.flat.w) and torch.equal(tr3.ema.buf, tr3.flat.w)
    bad = torch.load(with_avg, weights_only=False)
    bad['ema']['state_dict'].pop('module.1.bias')
    w = tr3.flat.w.clone()
    tr3.flat.w.zero_()
    with pytest.raises(_C.EfghError):
        tr3.load_checkpoint(bad)
    assert float(tr3.flat.w.abs().max()) == 0.0                                  # refused before the weights were written
    tr3.flat.w.copy_(w)
    off = Trainer(_toy(), None)
    off.load_checkpoint(with_avg)                                                # a trainer without an average ignores the file's
    assert off.ema is None and math.isclose(float(off.flat.w[0]), float(tr.flat.w[0]))


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """the argument checks of both entry points run before any device work, so they can be exercised on host arrays (nothing here
    is ever launched: every call below is one that must be refused)"""
    import ctypes
    lib = _C.lib()
    n = 64
    raw = (ctypes.c_float * (2 * n + 16))(*range(2 * n + 16))
    base = (ctypes.addressof(raw) + 15) // 16 * 16
    a, b = base, base + 4 * n + 16                                               # two 16-byte aligned, disjoint ranges
    before = list(raw)
    upd = lambda *args: lib.efgh_ema_update(*args, None)
    swp = lambda *args: lib.efgh_ema_swap(*args, None)
    calls = [upd(0, b, n, 0.9, 1, 1, 0), upd(a, 0, n, 0.9, 1, 1, 0), upd(a, b, 0, 0.9, 1, 1, 0), upd(a, b, -1, 0.9, 1, 1, 0),
             upd(a + 4, b, n, 0.9, 1, 1, 0), upd(a, b + 8, n, 0.9, 1, 1, 0), upd(a, a, n, 0.9, 1, 1, 0),
             upd(a, a + 16, n, 0.9, 1, 1, 0), upd(a + 16, a, n, 0.9, 1, 1, 0), upd(a, b, n, 0.0, 1, 1, 0),
             upd(a, b, n, 1.0, 1, 1, 0), upd(a, b, n, float('nan'), 1, 1, 0), upd(a, b, n, 0.9, 1, 0, 0),
             upd(a, b, n, 0.9, 1, 1, b + 4),
             swp(0, b, n), swp(a, 0, n), swp(a, b, 0), swp(a + 4, b, n), swp(a, b + 12, n), swp(a, a, n), swp(a, a + 16, n)]
    assert calls == [-1] * len(calls)
    assert b'invalid argument' in lib.efgh_last_error() and b'ema.hip' in lib.efgh_last_error()
    assert list(raw) == before
