"""Two data-parallel ranks sharing one GPU (gloo, as tests/test_gpu_grad_guard_dp.py): a NaN pixel in ONE rank's batch spoils only
that rank's BatchNorm statistics, yet BOTH ranks skip the step - the probe's count is summed over the ranks before the resolve launch -
each restores its own buffers, and the replicas stay identical."""
import json
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, manifest_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from efgh_amd import synthetic as syn
    from efgh_amd.losses import EFGHCriterion
    from efgh_amd.nets import EFGHBackbone
    from efgh_amd.train import Trainer
    raw, npts = (128, 256), 2048
    manifest = json.load(open(manifest_path))
    args = syn.default_args(raw, 'cuda')
    m = EFGHBackbone(args)
    m.load_state_dict(syn.synthetic_state_dict(manifest['state_dict'], 1))
    tr = Trainer(m.cuda(), EFGHCriterion(args), lr=1e-3, skip_nonfinite=True, transactional=True)
    b = syn.make_batch(raw, npts, 1, first_seed=rank)
    inp = [torch.from_numpy(b[k]).cuda() for k in ('pc', 'img', 'calib', 'A')]
    gt = {k: torch.from_numpy(v) for k, v in b['gt'].items()}
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
    ws = [torch.zeros_like(tr.flat.w) for _ in range(world)]
    dist.all_gather(ws, tr.flat.w)
    same = all(torch.equal(ws[0].view(torch.int32), w.view(torch.int32)) for w in ws[1:])
    moved = float((tr.flat.w - w0).abs().max()) > 0 and bool(torch.isfinite(tr.flat.w).all())
    q.put({'rank': rank, 'same': bool(same), 'moved': bool(moved), 'unchanged': bool(unchanged), 'skipped': stats['skipped'],
           'applied': stats['applied'], 'rolled_back': stats['rolled_back'], 'forward2': stats2['forward_nonfinite'],
           'first2': stats2['first_bad_buffer'], 'skipped2': stats2['skipped'], 'finite': bool(torch.isfinite(tr.txn.live).all())})
    dist.destroy_process_group()


def test_both_ranks_roll_back_the_step_one_rank_spoiled():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    mpath = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'state_dict_manifest.json')
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q, mpath)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=600) for _ in ps), key=lambda r: r['rank'])
    for p in ps:
        p.join(120)
    for r in res:
        assert r['skipped'] == 1 and r['skipped2'] == 1 and r['applied'] == 2 and r['rolled_back'] == 1, res
        assert r['unchanged'] and r['same'] and r['moved'] and r['finite'], res
    # the count is the sum over the ranks: the same on both; the buffer's name is known only where it was spoiled
    assert res[0]['forward2'] == res[1]['forward2'] > 0, res
    assert res[0]['first2'] is None and res[1]['first2'].endswith(('running_mean', 'running_var')), res
