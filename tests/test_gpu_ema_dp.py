"""Two data-parallel ranks sharing one GPU (gloo, as tests/test_gpu_txn_dp.py): every rank keeps its own weight average of
bit-identical weights, so the averages are bit-identical too - without a collective of their own."""
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
    from efgh_amd import train
    from efgh_amd.train import Trainer
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
    raw, npts = (128, 256), 2048
    manifest = json.load(open(manifest_path))
    args = syn.default_args(raw, 'cuda')
    m = EFGHBackbone(args)
    m.load_state_dict(syn.synthetic_state_dict(manifest['state_dict'], 1 + rank))         # different starts: rank 0's is broadcast
    tr = Trainer(m.cuda(), EFGHCriterion(args), lr=1e-3, ema_decay=0.999)
    start_equal = torch.equal(tr.ema.buf.view(torch.int32), tr.flat.w.view(torch.int32))
    b = syn.make_batch(raw, npts, 1, first_seed=rank)
    inp = [torch.from_numpy(b[k]).cuda() for k in ('pc', 'img', 'calib', 'A')]
    gt = {k: torch.from_numpy(v) for k, v in b['gt'].items()}
    for _ in range(3):
        tr.step(*inp, dict(gt))
    seen = dict(calls)
    bufs = [torch.zeros_like(tr.ema.buf) for _ in range(world)]
    dist.all_gather(bufs, tr.ema.buf)
    same = all(torch.equal(bufs[0].view(torch.int32), x.view(torch.int32)) for x in bufs[1:])
    moved = float((tr.ema.buf - tr.flat.w).abs().max()) > 0 and bool(torch.isfinite(tr.ema.buf).all())
    q.put({'rank': rank, 'same': bool(same), 'moved': bool(moved), 'start_equal': bool(start_equal), 'seen': seen,
           'inside': dict(inside), 'buckets': len(tr.comm.buckets), 't': tr.opt.t})
    dist.destroy_process_group()


def test_both_ranks_hold_the_same_average_without_a_collective():
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
        assert r['start_equal'] and r['same'] and r['moved'] and r['t'] == 3, res
        # the run did communicate (the constructor's broadcasts, every step's gradient buckets) - none of it from the average
        assert r['seen']['broadcast'] >= 1 and r['seen']['all_reduce'] >= 3 * r['buckets'] and r['seen']['other'] == 0, res
        assert r['inside'] == {'collectives': 0, 'init': 1, 'update': 3}, res
