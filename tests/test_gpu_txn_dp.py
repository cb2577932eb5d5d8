"""Two data-parallel ranks sharing one GPU (gloo, as tests/test_gpu_grad_guard_dp.py): a NaN pixel in ONE rank's batch spoils only
that rank's BatchNorm statistics, yet BOTH ranks skip the step - the probe's count is summed over the ranks before the resolve launch -
each restores its own buffers, and the replicas stay identical."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_harness as H  # noqa: E402

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, q):
    dist = H.rank_setup(rank, world, port)
    tr, inp, gt = H.rank_trainer(rank, skip_nonfinite=True, transactional=True)
    bad = list(inp)
    if rank == 1:                                            # only rank 1's second batch has the NaN pixel
        bad[1] = inp[1].clone()
        bad[1][0, 0, 40, 100] = float('nan')
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    w0 = tr.flat.w.clone()
    unchanged, stats2 = None, None
    for step in range(3):
        before = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
        tr.step(*(bad if step == 1 else inp), dict(gt))
        if step == 1:
            after = tr.model.state_dict()
            unchanged = len(before) == 637 and all(torch.equal(bits(before[k]), bits(after[k])) for k in before)
            stats2 = tr.guard_stats()
    stats = tr.guard_stats()
    same = H.gathered_equal(dist, world, tr.flat.w)
    moved = float((tr.flat.w - w0).abs().max()) > 0 and bool(torch.isfinite(tr.flat.w).all())
    q.put({'rank': rank, 'same': bool(same), 'moved': bool(moved), 'unchanged': bool(unchanged), 'skipped': stats['skipped'],
           'applied': stats['applied'], 'rolled_back': stats['rolled_back'], 'forward2': stats2['forward_nonfinite'],
           'first2': stats2['first_bad_buffer'], 'skipped2': stats2['skipped'], 'finite': bool(torch.isfinite(tr.txn.live).all())})
    dist.destroy_process_group()


def test_both_ranks_roll_back_the_step_one_rank_spoiled():
    res = H.run_ranks(_worker)
    for r in res:
        assert r['skipped'] == 1 and r['skipped2'] == 1 and r['applied'] == 2 and r['rolled_back'] == 1, res
        assert r['unchanged'] and r['same'] and r['moved'] and r['finite'], res
    # the count is the sum over the ranks: the same on both; the buffer's name is known only where it was spoiled
    assert res[0]['forward2'] == res[1]['forward2'] > 0, res
    assert res[0]['first2'] is None and res[1]['first2'].endswith(('running_mean', 'running_var')), res
