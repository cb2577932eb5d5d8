"""Two data-parallel ranks sharing one GPU (gloo, as tests/test_gpu_txn_dp.py): every rank keeps its own weight average of
bit-identical weights, so the averages are bit-identical too - without a collective of their own."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_harness as H  # noqa: E402

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, q):
    dist = H.rank_setup(rank, world, port)
    from efgh_amd import train
    calls = {'all_reduce': 0, 'broadcast': 0, 'other': 0}

    def counted(name, key):
        inner = getattr(dist, name)

        def fn(*a, **kw):
            calls[key] += 1
            return inner(*a, **kw)
        setattr(dist, name, fn)
    counted('all_reduce', 'all_reduce')
    counted('broadcast', 'broadcast')
    for name in ('all_gather', 'reduce', 'all_gather_into_tensor', 'reduce_scatter', 'all_to_all', 'gather', 'scatter', 'barrier'):
        counted(name, 'other')
    # collectives issued while the average is built or updated (the constructor's copy and every update, wrapped), and their number
    inside = {'collectives': 0, 'init': 0, 'update': 0}

    def watched(name):
        inner = getattr(train.WeightEma, name)

        def fn(*a, **kw):
            n0 = sum(calls.values())
            try:
                return inner(*a, **kw)
            finally:
                inside['collectives'] += sum(calls.values()) - n0
                inside[name.strip('_')] += 1
        setattr(train.WeightEma, name, fn)
    watched('__init__')
    watched('update')
    tr, inp, gt = H.rank_trainer(rank, sd_seed=1 + rank, ema_decay=0.999)                 # different starts: rank 0's is broadcast
    start_equal = torch.equal(tr.ema.buf.view(torch.int32), tr.flat.w.view(torch.int32))
    for _ in range(3):
        tr.step(*inp, dict(gt))
    seen = dict(calls)
    same = H.gathered_equal(dist, world, tr.ema.buf)
    moved = float((tr.ema.buf - tr.flat.w).abs().max()) > 0 and bool(torch.isfinite(tr.ema.buf).all())
    q.put({'rank': rank, 'same': bool(same), 'moved': bool(moved), 'start_equal': bool(start_equal), 'seen': seen,
           'inside': dict(inside), 'buckets': len(tr.comm.buckets), 't': tr.opt.t})
    dist.destroy_process_group()


def test_both_ranks_hold_the_same_average_without_a_collective():
    res = H.run_ranks(_worker)
    for r in res:
        assert r['start_equal'] and r['same'] and r['moved'] and r['t'] == 3, res
        # the run did communicate (the constructor's broadcasts, every step's gradient buckets) - none of it from the average
        assert r['seen']['broadcast'] >= 1 and r['seen']['all_reduce'] >= 3 * r['buckets'] and r['seen']['other'] == 0, res
        assert r['inside'] == {'collectives': 0, 'init': 1, 'update': 3}, res
