"""Gradient accumulation over micro-batches: everything that can be checked without a GPU - the numpy contract
(tests/grad_accum_contract.py) against torch's own `(loss_i / k).backward()` + Adam, GradAccumulator on a CPU FlatParams, two gloo
ranks with a paused OverlappedAllReduce, the C-ABI surface and the `micro_batches=` splitter."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_accum_contract as contract  # noqa: E402

SYMBOLS = ('efgh_grad_drain', 'efgh_gimg_valid_count')


def _bits(t):
    return t.detach().clone().view(torch.int32)


def _model(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Tanh(), torch.nn.Linear(19, 5))


def _loss(model, x):
    return model(x).pow(2).mean()


def test_contract_rules():
    g = [np.array([1.0, -0.0, 1e-30, 3e38], np.float32), np.array([1e-8, 0.0, 1e-30, 3e38], np.float32),
         np.array([-1.0, 0.0, -2e-30, -3e38], np.float32)]
    s = contract.sequential_sum(g)
    assert s[0] == np.float32(np.float32(1.0) + np.float32(1e-8)) - np.float32(1.0) and s[3] == np.inf    # (inf - 3e38: the ORDER shows)
    assert np.signbit(contract.sequential_sum(g[:1])[1]) and not np.signbit(s[1])                        # a copy first, then -0 + 0 = +0
    w = contract.depth_weights([100, 300, 200])
    assert w.dtype == np.float32 and w.tolist() == [0.5, 1.5, 1.0]
    assert contract.depth_weights([0, 0, 0]).tolist() == [1.0, 1.0, 1.0]                                # the zero-mean rule
    assert contract.depth_weights([0, 6]).tolist() == [0.0, 2.0]
    w = contract.depth_weights([1, 2, 4])
    assert w[0] == np.float32(1.0 / (7.0 / 3.0))                                                        # float64, ONE rounding
    assert contract.depth_weights([10, 30, 20, 60], own=[10, 30]).tolist() == [np.float32(10 / 30.), 1.0]      # two ranks x two
    assert contract.grad_scale(3) == 1.0 / 3 and contract.grad_scale(3, 2) == 1.0 / 6 and contract.grad_scale(1) == 1.0


def test_contract_matches_torch_accumulation_and_adam():
    """k = 3 micro-batches, `(loss_i / k).backward()` into .grad, torch.optim.Adam - against the sequential fp32 SUM of the three
    unscaled gradients fed to the Adam recipe with grad_scale = 1 / k, within the FusedAdam yardstick 2e-6 + 1e-5 max|w|, over
    three optimizer steps (the contract's gradients are taken at torch's own weights each step)"""
    k, lr = 3, 1e-2
    model = _model(1)
    params = list(model.parameters())
    opt = torch.optim.Adam(params, lr=lr)
    flatten = lambda ts: torch.cat([t.reshape(-1) for t in ts]).detach().numpy()
    w = flatten(params).astype(np.float64)
    m, v = np.zeros_like(w), np.zeros_like(w)
    torch.manual_seed(7)
    for t in range(1, 4):
        xs = [torch.randn(8, 37) * (1 + i) for i in range(k)]
        grads = [flatten(torch.autograd.grad(_loss(model, x), params)) for x in xs]
        acc = contract.sequential_sum(grads)
        assert acc.dtype == np.float32
        opt.zero_grad()
        for x in xs:
            (_loss(model, x) / k).backward()
        opt.step()
        w, m, v = contract.adam_on_sum(w, m, v, acc, k, 1, t, lr)
        got = flatten(params).astype(np.float64)
        d, tol = float(np.abs(got - w).max()), 2e-6 + 1e-5 * float(np.abs(w).max())
        print('step', t, 'max |torch - contract|', d, 'bound', tol)
        assert d <= tol
        assert float(np.abs(got - flatten(_model(1).parameters())).max()) > 1e-3           # (it trained)


def test_grad_accumulator_on_cpu_flat_params():
    from efgh_amd.train import FlatParams, GradAccumulator
    model = _model(2)
    flat = FlatParams(model)
    acc = GradAccumulator(flat)
    assert acc.acc is None and acc.count == 0                       # allocated on first use
    torch.manual_seed(3)
    for step in range(2):
        clones = []
        flat.zero_grad()
        for i in range(3):
            _loss(model, torch.randn(8, 37) * 10.0 ** i).backward()
            if i == 0:
                flat.g[5] = -0.0
            clones.append(flat.g.clone())
            assert acc.drain() == i + 1
            assert torch.equal(_bits(flat.g), torch.zeros(flat.n, dtype=torch.int32))                    # all +0
            assert all(p.grad.data_ptr() == flat.g.data_ptr() + 4 * off for p, (off, _) in zip(flat.params, flat.offsets))
            assert flat.arrived == [False] * len(flat.params)
            if i == 0:
                assert torch.equal(_bits(acc.acc), _bits(clones[0]))                                     # -0 included
        want = contract.sequential_sum([c.numpy() for c in clones])
        assert np.array_equal(acc.acc.numpy().view(np.int32), want.view(np.int32))
        assert float(np.abs(want).max()) > 0
        acc.reset()
        assert acc.count == 0
        acc.acc.fill_(float('nan'))                                  # the next first drain does not read it


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from efgh_amd.train import FlatParams, GradAccumulator, OverlappedAllReduce, allreduce_mean_
    k = 3
    model = _model(0)
    flat = FlatParams(model)
    comm = OverlappedAllReduce(flat, world, bucket_elems=300)
    assert len(comm.buckets) >= 2 and comm._arrived in flat.listeners
    acc = GradAccumulator(flat)
    torch.manual_seed(100 + rank)                       # each rank: its own samples
    comm.start_step()
    comm.paused = True
    local = []
    flat.zero_grad()
    for i in range(k):
        _loss(model, torch.randn(8, 37)).backward()
        local.append(flat.g.clone())
        acc.drain()
    comm.finish()
    issued = list(comm.order) + list(comm.works)        # nothing may have gone on the wire while paused
    comm.paused = False
    allreduce_mean_(acc.acc, world, bucket_elems=100)
    mean = acc.acc * contract.grad_scale(k, world)
    gathered = [torch.zeros(k, flat.n) for _ in range(world)]
    dist.all_gather(gathered, torch.stack(local))
    want = torch.cat(gathered).double().mean(0)
    ok = not issued and float((mean.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    ok = ok and all(p.grad.data_ptr() == flat.g.data_ptr() + 4 * off for p, (off, _) in zip(flat.params, flat.offsets))
    ok = ok and not bool(flat.g.any())
    # un-paused, the same listeners work as before
    comm.start_step()
    _loss(model, torch.randn(8, 37)).backward()
    comm.finish()
    ok = ok and len(comm.order) == len(comm.buckets)
    q.put((rank, bool(ok), len(issued), float(mean.sum())))
    dist.destroy_process_group()


def test_two_gloo_ranks_accumulate_to_the_mean_of_six_gradients():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=120) for _ in ps]
    for p in ps:
        p.join(60)
    assert all(ok and issued == 0 for _, ok, issued, _ in res), res
    assert res[0][3] == res[1][3]                       # both ranks hold the same mean gradient


def test_entry_points_are_in_header_and_library():
    from efgh_amd import _C
    hdr = open(os.path.join(ROOT, 'include', 'efgh_hip.h')).read()
    lib = _C.lib()
    for s in SYMBOLS:
        assert 'int %s(' % s in hdr
        assert getattr(lib, s) is not None
    assert lib.efgh_version() == 4 and '#define EFGH_ABI_VERSION 4' in hdr          # additive: the ABI number did not move


@pytest.mark.parametrize('kw', [dict(acc=None), dict(g=None), dict(g=0x1000), dict(n=0), dict(n=-3), dict(acc=0x1004),
                                dict(g=0x1100)],           # (the last: overlapping ranges)
                         ids=lambda kw: ','.join('%s=%s' % kv for kv in kw.items()))
def test_drain_refuses_bad_arguments_before_any_device_work(kw):
    """the pointers are fake: a call that passed validation would fault, so every one of these must be refused first"""
    from efgh_amd import _C
    lib = _C.lib()
    a = dict(acc=0x1000, g=0x2000, n=100)
    a.update(kw)
    for first in (0, 1):
        assert lib.efgh_grad_drain(a['acc'], a['g'], a['n'], first, None) == -1
        msg = lib.efgh_last_error().decode()
        assert 'invalid argument' in msg and 'accum.hip' in msg


@pytest.mark.parametrize('kw', [dict(gdep=None), dict(mask=None), dict(count=None), dict(B=0), dict(HW=0), dict(count=0x3004)],
                         ids=lambda kw: ','.join('%s=%s' % kv for kv in kw.items()))
def test_valid_count_refuses_bad_arguments_before_any_device_work(kw):
    from efgh_amd import _C
    lib = _C.lib()
    a = dict(gdep=0x1000, mask=0x2000, B=1, HW=16, count=0x3000)
    a.update(kw)
    assert lib.efgh_gimg_valid_count(a['gdep'], a['mask'], a['B'], a['HW'], a['count'], None) == -1
    assert 'invalid argument' in lib.efgh_last_error().decode()


def test_splitter():
    from efgh_amd import _C
    from efgh_amd.train import split_micro_batches
    B = 6
    pc, img, calib, A = torch.arange(B * 3 * 4.).view(B, 3, 4), torch.zeros(B, 3, 2, 2), torch.zeros(B, 3, 4), torch.zeros(B, 3, 3)
    gt = {'cam_T_velo': np.arange(B * 16.).reshape(B, 4, 4), 'img_mask': torch.ones(B, 1, 2, 2, dtype=torch.uint8)}
    mbs = split_micro_batches(pc, img, calib, A, gt, 3)
    assert len(mbs) == 3 and all(len(mb) == 5 for mb in mbs)
    assert torch.equal(torch.cat([mb[0] for mb in mbs]), pc) and mbs[1][0].data_ptr() == pc[2:4].data_ptr()      # slices, no copies
    assert all(mb[1].shape[0] == 2 and mb[4]['img_mask'].shape[0] == 2 for mb in mbs)
    assert np.array_equal(np.concatenate([mb[4]['cam_T_velo'] for mb in mbs]), gt['cam_T_velo'])
    assert len(split_micro_batches(pc, img, calib, A, gt, 1)) == 1
    with pytest.raises(_C.EfghError, match='4.*6|6.*4'):
        split_micro_batches(pc, img, calib, A, gt, 4)                              # B % k != 0
    for bad in (dict(gt, scale=1.0), dict(gt, intr=np.eye(3)), dict(gt, name='kitti')):
        key = [k for k in bad if k not in gt][0]
        with pytest.raises(_C.EfghError, match=key):
            split_micro_batches(pc, img, calib, A, bad, 2)                         # a gt entry without the batch dimension
    for k in (0, -1, 1.5, True):
        with pytest.raises(_C.EfghError, match='micro_batches'):
            split_micro_batches(pc, img, calib, A, gt, k)


class _Crit:
    loss_name = ['total']


def test_step_accumulated_refuses_unequal_micro_batches():
    """refused before anything runs (a CPU model: reaching the forward would raise another error)"""
    from efgh_amd import _C
    from efgh_amd.train import Trainer
    tr = Trainer(_model(0), _Crit())
    mb = lambda b: (torch.zeros(b, 3, 4), torch.zeros(b, 3, 2, 2), torch.zeros(b, 3, 4), torch.zeros(b, 3, 3), {})
    with pytest.raises(_C.EfghError, match=r'\[2, 3, 2\]'):
        tr.step_accumulated([mb(2), mb(3), mb(2)])
    with pytest.raises(_C.EfghError, match='k >= 1'):
        tr.step_accumulated([])
    assert tr.it == 0 and tr.accum is None
