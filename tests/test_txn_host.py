"""Transactional BatchNorm state on the host: the numpy contract's own rules (tests/txn_contract.py), the option's validation, and
train.BnTransaction on CPU tensors - re-homing, snapshot / probe / resolve, the aliasing check, the buffer names."""
import os
import sys

import numpy as np
import pytest
import torch

from efgh_amd import _C

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import txn_contract as contract  # noqa: E402

INF, NAN = float('inf'), float('nan')


def test_contract_count_and_first_bad_rules():
    starts = [0, 3, 35, 96]
    shadow = np.arange(96, dtype=np.float32)
    live = shadow.copy()
    assert contract.probe(live, shadow, starts) == (0, -1)
    live[[2, 3, 95]] = [INF, -INF, NAN]                     # last of buffer 0, first of buffer 1, last of buffer 2
    assert contract.probe(live, shadow, starts) == (3, 0)
    live[2] = 2.0
    assert contract.probe(live, shadow, starts) == (2, 1)
    shadow[3] = NAN                                         # was non-finite before the step: counts nothing
    assert contract.probe(live, shadow, starts) == (1, 2)
    assert contract.probe(live, shadow, starts, losses=[1.0, INF, NAN]) == (3, 2)
    live[95] = 0.0
    assert contract.probe(live, shadow, starts, losses=[NAN]) == (1, -1)      # a loss names no buffer
    shadow[7], live[7] = INF, 1.0                           # non-finite -> finite is not an event either
    assert contract.probe(live, shadow, starts) == (0, -1)


def test_contract_veto_rule_mirrors_a_skip_of_the_guard():
    import grad_guard_contract as guard
    applied = guard.decide([4.0], [0], INF, 1.0, True, 4, 2)
    skipped = guard.decide([4.0], [1], INF, 1.0, True, 4, 2)
    assert (applied['applied'], applied['skipped'], applied['skip']) == (5, 2, False)
    block = dict(applied, skip=0, bc1=contract.bias_corrections(5)[0], bc2_sqrt=contract.bias_corrections(5)[1])
    same, t, restore = contract.resolve(block, 0)
    assert same == block and not restore and t == {'vetoed': 0, 'vetoed_total': 0, 'rolled_back': 0}
    g, t, restore = contract.resolve(block, 3)
    assert restore and t == {'vetoed': 1, 'vetoed_total': 1, 'rolled_back': 1}
    assert (g['applied'], g['skipped'], g['skip']) == (skipped['applied'], skipped['skipped'], 1) == (4, 3, 1)
    assert (g['bc1'], g['bc2_sqrt']) == contract.bias_corrections(4)
    for k in ('norm', 'coef', 'scale', 'nonfinite'):        # untouched
        assert g[k] == block[k]
    # a step the guard skipped itself: no veto, but restored
    own = dict(block, skip=1, applied=4, skipped=3)
    g, t, restore = contract.resolve(own, 0)
    assert g == own and restore and t == {'vetoed': 0, 'vetoed_total': 0, 'rolled_back': 1}
    g, t, restore = contract.resolve(own, 2)
    assert g == own and restore and t['vetoed'] == 0
    bc1, bc2 = contract.bias_corrections(1)
    assert abs(bc1 - 0.1) < 1e-6 and abs(bc2 - 0.001 ** 0.5) < 1e-6 and contract.bias_corrections(0) == (0.0, 0.0)


def test_transactional_needs_skip_nonfinite():
    from efgh_amd.train import BnTransaction, FlatParams, FusedAdam, Trainer
    m = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.BatchNorm1d(4))
    before = {k: v.data_ptr() for k, v in m.state_dict().items()}
    with pytest.raises(_C.EfghError, match='skip_nonfinite'):
        Trainer(m, None, transactional=True)
    with pytest.raises(_C.EfghError, match='skip_nonfinite'):
        Trainer(m, None, max_grad_norm=1.0, transactional=True)
    assert {k: v.data_ptr() for k, v in m.state_dict().items()} == before     # refused before anything was re-homed
    flat = FlatParams(m)
    with pytest.raises(_C.EfghError, match='skip_nonfinite'):
        FusedAdam(flat, max_grad_norm=1.0, txn=BnTransaction(m, flat))
    with pytest.raises(_C.EfghError, match='no BatchNorm'):
        lin = torch.nn.Linear(2, 2)
        BnTransaction(lin, FlatParams(lin))


def test_defaults_build_no_transaction():
    from efgh_amd.train import FlatParams, Trainer
    m = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.BatchNorm1d(4), torch.nn.BatchNorm1d(4))
    ptrs = {k: v.data_ptr() for k, v in m.state_dict().items() if 'running' in k}
    flat = FlatParams(m)
    assert not any(hasattr(flat, a) for a in ('txn', 'live', 'shadow_f'))
    for kw in ({}, {'skip_nonfinite': True}, {'max_grad_norm': 1.0}):
        m2 = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.BatchNorm1d(4), torch.nn.BatchNorm1d(4))
        p2 = {k: v.data_ptr() for k, v in m2.state_dict().items() if 'running' in k}
        tr = Trainer(m2, None, **kw)
        assert tr.txn is None and tr.opt.txn is None
        assert {k: v.data_ptr() for k, v in m2.state_dict().items() if 'running' in k} == p2      # the float buffers stay where they were
        if tr.opt.state is not None:
            assert tr.opt.state.numel() == _C.ctypes.sizeof(_C.GuardState)
    assert {k: v.data_ptr() for k, v in m.state_dict().items() if 'running' in k} == ptrs
    tr = Trainer(torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.BatchNorm1d(4)), None, skip_nonfinite=True, transactional=True)
    assert tr.txn is not None and tr.opt.txn is tr.txn
    assert tr.opt.state.numel() == _C.ctypes.sizeof(_C.GuardState) + _C.ctypes.sizeof(_C.TxnState)


def _bits(t):
    return t.detach().clone().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _model():
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.BatchNorm1d(7), torch.nn.BatchNorm1d(7))
    with torch.no_grad():
        for bn in (m[1], m[2]):
            bn.running_mean.copy_(torch.randn(7))
            bn.running_var.copy_(torch.rand(7) + 0.5)
        m[1].running_mean[0] = -0.0
        # a NaN with a payload and a sign: a restore must copy bits, not values
        m[2].running_var.view(torch.int32)[3] = int(np.array([0xffc12345], np.uint32).view(np.int32)[0])
        m[2].num_batches_tracked += 41
    return m


def test_bn_transaction_on_cpu_tensors():
    from efgh_amd.train import BnTransaction, FlatParams
    m = _model()
    keys = [(k, tuple(v.shape), v.dtype) for k, v in m.state_dict().items()]
    before = {k: _bits(v) for k, v in m.state_dict().items()}
    flat = FlatParams(m)
    txn = BnTransaction(m, flat)
    assert [(k, tuple(v.shape), v.dtype) for k, v in m.state_dict().items()] == keys        # names, shapes, order
    for k, v in m.state_dict().items():
        assert torch.equal(_bits(v), before[k]), k                                           # bit for bit
    assert txn.names == ['1.running_mean', '1.running_var', '2.running_mean', '2.running_var']
    assert txn.nf % 4 == 0 and txn.live.data_ptr() == m[1].running_mean.data_ptr() and txn.host is not None and txn.block is None
    assert all(getattr(mod, attr).data_ptr() == txn.live.data_ptr() + 4 * a for mod, attr, a, _ in txn.slots)
    assert [a % BnTransaction.ALIGN for a in txn._starts] == [0] * 5 and txn.starts.tolist() == txn._starts

    def mutate():
        m.train()
        m(torch.randn(6, 5))                                # torch's own BatchNorm: running statistics and counters move
        with torch.no_grad():
            m[2].running_mean[2] = INF

    # a skipped step is restored, bits and all
    txn.snapshot()
    mutate()
    assert int(m[1].num_batches_tracked) == 1 and int(m[2].num_batches_tracked) == 42
    txn.probe()
    assert txn.stats()['forward_nonfinite'] == 1 and txn.stats()['first_bad_buffer'] == '2.running_mean'
    assert txn.resolve(skip=True) is True
    for k, v in m.state_dict().items():
        assert torch.equal(_bits(v), before[k]), k
    s = txn.stats()
    assert (s['rolled_back'], s['vetoed']) == (1, 0)

    # an applied step keeps what the forward did
    txn.snapshot()
    assert txn.stats()['forward_nonfinite'] == 0 and txn.stats()['first_bad_buffer'] is None
    m.train()
    m(torch.randn(6, 5))
    moved = {k: _bits(v) for k, v in m.state_dict().items()}
    txn.probe(torch.tensor([1.0, 2.0]), 2, 1)
    assert txn.stats()['forward_nonfinite'] == 0            # (the NaN of 2.running_var was there before the step)
    assert txn.resolve(skip=False) is False
    for k, v in m.state_dict().items():
        assert torch.equal(_bits(v), moved[k]), k
    assert not torch.equal(moved['1.running_mean'], before['1.running_mean']) and int(m[1].num_batches_tracked) == 1
    assert txn.stats()['rolled_back'] == 1

    # a non-finite forward vetoes a step the guard would have applied; a non-finite loss alone names no buffer
    txn.snapshot()
    mutate()
    txn.probe(torch.tensor([0.5, NAN, 1.0, INF]), 2, 2, 1)  # elements 1 and 3
    s = txn.stats()
    assert s['forward_nonfinite'] == 3 and s['first_bad_buffer'] == '2.running_mean'
    assert txn.resolve(skip=False) is True
    for k, v in m.state_dict().items():
        assert torch.equal(_bits(v), moved[k]), k
    s = txn.stats()
    assert (s['rolled_back'], s['vetoed']) == (2, 1) and txn.host.vetoed_total == 1
    txn.snapshot()
    txn.probe(torch.tensor([NAN]), 1, 1)
    s = txn.stats()
    assert s['forward_nonfinite'] == 1 and s['first_bad_buffer'] is None and s['vetoed'] == 0

    # load_state_dict copies in place: the views survive it
    m.load_state_dict({k: torch.zeros_like(v) for k, v in m.state_dict().items()})
    txn.snapshot()
    assert float(txn.live.abs().sum()) == 0 and int(flat.nbt.sum()) == 0


def test_bn_transaction_refuses_a_rebound_buffer_by_name():
    from efgh_amd.train import BnTransaction, FlatParams
    m = _model()
    flat = FlatParams(m)
    txn = BnTransaction(m, flat)
    txn.snapshot()
    m[2].running_var = m[2].running_var.clone()
    with pytest.raises(_C.EfghError, match=r'2\.running_var'):
        txn.snapshot()
    m = _model()
    flat = FlatParams(m)
    txn = BnTransaction(m, flat)
    m[1].num_batches_tracked = m[1].num_batches_tracked.clone()
    with pytest.raises(_C.EfghError, match=r'1\.num_batches_tracked'):
        txn.snapshot()
    m = _model()
    txn = BnTransaction(m, FlatParams(m))
    m.double()
    with pytest.raises(_C.EfghError, match=r'1\.running_mean'):
        txn.snapshot()


def test_txn_state_mirror_matches_the_header():
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = ['forward_nonfinite', 'rolled_back', 'vetoed_total', 'first_bad', 'vetoed']
    src = '#include <stdio.h>\n#include "efgh_hip.h"\nint main(){printf("%zu %zu"' + ' " %zu"' * len(fields) + \
          ',sizeof(efgh_txn_state),sizeof(efgh_guard_state)' + ''.join(',__builtin_offsetof(efgh_txn_state,%s)' % f for f in fields) + \
          ');return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'p.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(root, 'include'), os.path.join(d, 'p.c'), '-o', os.path.join(d, 'p')])
        got = list(map(int, subprocess.check_output([os.path.join(d, 'p')]).split()))
    assert got[0] == _C.ctypes.sizeof(_C.TxnState) and got[1] == _C.ctypes.sizeof(_C.GuardState) and got[1] % 8 == 0
    assert got[2:] == [getattr(_C.TxnState, f).offset for f in fields]
