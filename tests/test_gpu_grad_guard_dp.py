"""Two data-parallel ranks sharing one GPU (gloo, as tests/test_gpu_dp.py): a non-finite gradient on ONE rank is skipped by BOTH -
the guard decides from the all-reduced gradient, which holds the same bits everywhere - and the replicas stay identical."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_harness as H  # noqa: E402

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, q):
    dist = H.rank_setup(rank, world, port)
    tr, inp, gt = H.rank_trainer(rank, bad_calls=(2,) if rank == 1 else (), skip_nonfinite=True)    # only rank 1's second loss is infinite
    w0 = tr.flat.w.clone()
    unchanged, totals = None, []
    for step in range(3):
        before = tr.flat.w.clone().view(torch.int32)
        losses, _ = tr.step(*inp, dict(gt))
        totals.append(float(losses['total'].detach()))
        if step == 1:
            unchanged = bool(torch.equal(before, tr.flat.w.view(torch.int32)))
            stats2 = tr.guard_stats()
    stats = tr.guard_stats()
    same = H.gathered_equal(dist, world, tr.flat.w)
    moved = float((tr.flat.w - w0).abs().max()) > 0 and bool(torch.isfinite(tr.flat.w).all())
    q.put({'rank': rank, 'same': bool(same), 'moved': bool(moved), 'unchanged': unchanged, 'skipped': stats['skipped'],
           'applied': stats['applied'], 'nonfinite2': stats2['nonfinite'], 'totals': totals, 't': tr.opt.t})
    dist.destroy_process_group()


def test_both_ranks_skip_the_step_one_rank_spoiled():
    res = H.run_ranks(_worker)
    for r in res:
        assert r['skipped'] == 1 and r['applied'] == 2 and r['t'] == 2, res
        assert r['unchanged'] and r['same'] and r['moved'] and r['nonfinite2'] > 0, res
    assert math.isfinite(res[0]['totals'][1]) and not math.isfinite(res[1]['totals'][1])      # rank 0 itself saw nothing wrong
