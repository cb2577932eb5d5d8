"""Two data-parallel ranks sharing one GPU (gloo, as tests/test_gpu_dp.py): a non-finite gradient on ONE rank is skipped by BOTH -
the guard decides from the all-reduced gradient, which holds the same bits everywhere - and the replicas stay identical."""
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


class _InfOnCall:
    def __init__(self, inner, bad_calls):
        self.inner, self.bad, self.calls = inner, set(bad_calls), 0

    def compute_loss(self, *a):
        losses, gt = self.inner.compute_loss(*a)
        self.calls += 1
        if self.calls in self.bad:
            losses = dict(losses)
            losses['total'] = losses['total'] * float('inf')
        return losses, gt


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
    crit = _InfOnCall(EFGHCriterion(args), (2,) if rank == 1 else ())                    # only rank 1's second loss is infinite
    tr = Trainer(m.cuda(), crit, lr=1e-3, skip_nonfinite=True)
    b = syn.make_batch(raw, npts, 1, first_seed=rank)
    inp = [torch.from_numpy(b[k]).cuda() for k in ('pc', 'img', 'calib', 'A')]
    gt = {k: torch.from_numpy(v) for k, v in b['gt'].items()}
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
    ws = [torch.zeros_like(tr.flat.w) for _ in range(world)]
    dist.all_gather(ws, tr.flat.w)
    same = all(torch.equal(ws[0].view(torch.int32), w.view(torch.int32)) for w in ws[1:])
    moved = float((tr.flat.w - w0).abs().max()) > 0 and bool(torch.isfinite(tr.flat.w).all())
    q.put({'rank': rank, 'same': bool(same), 'moved': bool(moved), 'unchanged': unchanged, 'skipped': stats['skipped'],
           'applied': stats['applied'], 'nonfinite2': stats2['nonfinite'], 'totals': totals, 't': tr.opt.t})
    dist.destroy_process_group()


def test_both_ranks_skip_the_step_one_rank_spoiled():
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
        assert r['skipped'] == 1 and r['applied'] == 2 and r['t'] == 2, res
        assert r['unchanged'] and r['same'] and r['moved'] and r['nonfinite2'] > 0, res
    import math
    assert math.isfinite(res[0]['totals'][1]) and not math.isfinite(res[1]['totals'][1])      # rank 0 itself saw nothing wrong
