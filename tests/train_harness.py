"""What the trainer-level GPU tests share (test_gpu_grad_guard / _grad_accum / _txn / _ema and their two-rank _dp files): the small
configuration of tests/test_gpu_train.py, the criterion wrappers that spoil a step, Trainer builders, and the spawn scaffold of the
data-parallel tests.  A plain module, imported like the *_contract modules; the `world` fixture is imported by name."""
import json
import os
import socket
import sys

import pytest
import torch

from efgh_amd import synthetic as syn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'tools'))
from glue_census import census  # noqa: E402,F401

RAW, NPTS = (128, 256), 2048
INF, NAN = float('inf'), float('nan')
MANIFEST = os.path.join(HERE, 'golden', 'state_dict_manifest.json')


class InfOnCall:
    """criterion whose `total` is multiplied by inf on the given calls (1-based): the forward stays finite, the gradient does not.
    `forward_names`: also offer the inner criterion's `loss_name`.  step_accumulated returns its losses in that order when it is
    there and in the order of compute_loss's dict otherwise, and the two differ (`total` leads loss_name and ends the dict), so
    the forwarding stays a choice of the caller."""

    def __init__(self, inner, bad_calls, forward_names=False):
        self.inner, self.bad, self.calls = inner, set(bad_calls), 0
        if forward_names:
            self.loss_name = getattr(inner, 'loss_name', None)

    def compute_loss(self, *a):
        losses, gt = self.inner.compute_loss(*a)
        self.calls += 1
        if self.calls in self.bad:
            losses = dict(losses)
            losses['total'] = losses['total'] * INF
        return losses, gt


class SpoilOnCall:
    """criterion that writes +inf into one running statistic on the given call (1-based), after the forward: loss and gradient stay
    finite - the case the deferred activations can produce, which only the transaction's probe sees"""

    def __init__(self, inner, model, key, call):
        self.inner, self.model, self.key, self.call, self.calls = inner, model, key, call, 0

    def compute_loss(self, *a):
        self.calls += 1
        if self.calls == self.call:
            with torch.no_grad():
                self.model.state_dict()[self.key].view(-1)[0] = INF
        return self.inner.compute_loss(*a)


def bits(t):
    return t.detach().clone().view(torch.int32)


def batch(seed, size=2):
    """-> ([pc, img, calib, A] on the device, gt on the host)"""
    b = syn.make_batch(RAW, NPTS, size, first_seed=seed)
    return ([torch.from_numpy(b[k]).cuda() for k in ('pc', 'img', 'calib', 'A')],
            {k: torch.from_numpy(v) for k, v in b['gt'].items()})


def make_world(manifest):
    return {'sd': syn.synthetic_state_dict(manifest['state_dict'], 1), 'batches': [batch(0), batch(2), batch(4)]}


@pytest.fixture(scope='module')
def world(manifest):
    return make_world(manifest)


def model(sd):
    from efgh_amd.nets import EFGHBackbone
    m = EFGHBackbone(syn.default_args(RAW, 'cuda'))
    m.load_state_dict(sd)
    return m.cuda()


def trainer(world, bad_calls=(), lr=1e-3, forward_names=False, **kw):
    from efgh_amd.losses import EFGHCriterion
    from efgh_amd.train import Trainer
    crit = EFGHCriterion(syn.default_args(RAW, 'cuda'))
    return Trainer(model(world['sd']), InfOnCall(crit, bad_calls, forward_names) if bad_calls else crit, lr=lr, **kw)


def mb(world, i):
    """batch i (or the entry named i) as one micro-batch (pc, img, calib, A, gt) with a gt dict of its own"""
    inp, gt = world[i] if isinstance(i, str) else world['batches'][i]
    return tuple(inp) + (dict(gt),)


def step(tr, world, i, **kw):
    return tr.step(*mb(world, i), **kw)


def eval_forward(m, world):
    m.eval()
    with torch.no_grad():
        out = m(*world['batches'][2][0])
    return {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}


def waits_for_nothing(fn):
    """runs fn with synchronising calls flagged as errors, where this build can flag them (else there is nothing to check)"""
    try:
        torch.cuda.set_sync_debug_mode('error')
    except (RuntimeError, AttributeError):
        return
    try:
        fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')


# ---- two data-parallel ranks sharing one GPU over gloo
def run_ranks(worker, world=2):
    """spawns worker(rank, world, port, queue) per rank -> what each put on the queue, in rank order"""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ps = [ctx.Process(target=worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=600) for _ in ps), key=lambda r: r['rank'])
    for p in ps:
        p.join(120)
    return res


def rank_setup(rank, world, port):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    return dist


def rank_trainer(rank, sd_seed=1, bad_calls=(), **kw):
    """-> (Trainer on the weights of `sd_seed`, this rank's one-sample batch: inp, gt)"""
    tr = trainer({'sd': syn.synthetic_state_dict(json.load(open(MANIFEST))['state_dict'], sd_seed)}, bad_calls, **kw)
    return (tr,) + batch(rank, 1)


def gathered_equal(dist, world, t):
    """every rank holds the bits of `t`"""
    ts = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(ts, t)
    return all(torch.equal(ts[0].view(torch.int32), x.view(torch.int32)) for x in ts[1:])
