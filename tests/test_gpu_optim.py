"""efgh_amd.optim.Adam / AdamW (the torch.optim drop-ins on the fused step) and Trainer(param_groups=) on the GPU: bit equality
with train.FusedAdam, agreement with torch's optimizers, checkpoint interchange in both directions, the reference's own loop
against Trainer.step, and parameter groups by name."""
import os
import sys

import pytest
import torch

from efgh_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_harness import RAW, NPTS, bits, mb, model, step, trainer, world  # noqa: E402,F401

pytestmark = pytest.mark.gpu
SHAPES = [(1,), (3,), (1025,), (4, 5), (7, 3, 3)]
STOCK_ADAM = torch.optim.Adam


def _params(seed, shapes=SHAPES):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(s, generator=gen) * 0.1).cuda().requires_grad_(True) for s in shapes]


def _grads(seed, shapes=SHAPES):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(s, generator=gen) * 0.01).cuda() for s in shapes]


def _feed(params, grads):
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)


def _close(ours, theirs):
    """the bound tests/test_gpu_train.py holds the fused step to against torch.optim.Adam"""
    for p, q in zip(ours, theirs):
        d = float((p.detach() - q.detach()).abs().max())
        assert d <= 2e-6 + 1e-5 * float(q.detach().abs().max()), d


def test_one_group_is_fused_adam_bit_for_bit():
    from efgh_amd.optim import Adam
    from efgh_amd.train import FlatParams, FusedAdam
    ours, twin = _params(0), _params(0)
    opt = Adam(ours, lr=1e-3, weight_decay=1e-2)
    assert opt.fused.param_groups is None                      # one coupled group: the launches FusedAdam always made
    flat = FlatParams.from_params(twin)
    ref = FusedAdam(flat, lr=1e-3, weight_decay=1e-2)
    for it in range(3):
        grads = _grads(10 + it)
        opt.zero_grad()
        flat.zero_grad()
        _feed(ours, grads)
        _feed(twin, grads)
        opt.step()
        ref.step()
        assert torch.equal(bits(opt.flat.w), bits(flat.w))
        assert torch.equal(bits(opt.fused.m), bits(ref.m)) and torch.equal(bits(opt.fused.v), bits(ref.v))
    assert opt.fused.t == ref.t == 3 and all(p.data_ptr() >= opt.flat.w.data_ptr() for p in ours)


def _two_groups(params):
    return [{'params': params[:3], 'lr': 1e-3, 'weight_decay': 1e-2},
            {'params': params[3:], 'lr': 3e-4, 'weight_decay': 5e-2, 'decoupled_weight_decay': True}]


def test_two_groups_agree_with_torch_adam_and_adamw():
    from efgh_amd.optim import Adam
    ours, theirs = _params(1), _params(1)
    opt = Adam(_two_groups(ours))
    stock = STOCK_ADAM(_two_groups(theirs))
    assert [g['decoupled'] for g in opt.fused.param_groups] == [False, True]
    for it in range(2):
        grads = _grads(20 + it)
        opt.zero_grad()
        _feed(ours, grads)
        _feed(theirs, grads)
        opt.step()
        stock.step()
        _close(ours, theirs)
    # the same through the AdamW class, one decoupled group
    from efgh_amd.optim import AdamW
    a, b = _params(2), _params(2)
    opt, stock = AdamW(a, lr=2e-3), torch.optim.AdamW(b, lr=2e-3)
    for it in range(2):
        grads = _grads(30 + it)
        opt.zero_grad()
        _feed(a, grads)
        _feed(b, grads)
        opt.step()
        stock.step()
        _close(a, b)


def test_state_dict_round_trip_with_torch_both_ways():
    from efgh_amd.optim import Adam
    ours, theirs = _params(3), _params(3)
    opt, stock = Adam(_two_groups(ours)), STOCK_ADAM(_two_groups(theirs))
    for it in range(2):                                        # two steps of ours; torch's twin follows through the state_dict
        opt.zero_grad()
        _feed(ours, _grads(40 + it))
        opt.step()
    sd = opt.state_dict()
    assert [g['params'] for g in sd['param_groups']] == [[0, 1, 2], [3, 4]] and sorted(sd['state']) == [0, 1, 2, 3, 4]
    stock.load_state_dict(sd)
    with torch.no_grad():
        for p, q in zip(ours, theirs):
            q.copy_(p)
    grads = _grads(42)
    opt.zero_grad()
    _feed(ours, grads)
    _feed(theirs, grads)
    opt.step()
    stock.step()
    _close(ours, theirs)
    # the other way round: torch's state after its third step into a fresh optimizer of ours
    fresh = _params(3)
    opt2 = Adam(_two_groups(fresh))
    opt2.load_state_dict(stock.state_dict())
    assert opt2.fused.t == 3
    with torch.no_grad():
        for p, q in zip(fresh, theirs):
            p.copy_(q)
    grads = _grads(43)
    opt2.zero_grad()
    _feed(fresh, grads)
    _feed(theirs, grads)
    opt2.step()
    stock.step()
    _close(fresh, theirs)
    # a stock single-group dict (the reference's optimizer entry) loads into the one-group form
    a, b = _params(4), _params(4)
    one, stock1 = Adam(a, lr=1e-3), STOCK_ADAM(b, lr=1e-3)
    _feed(b, _grads(44))
    stock1.step()
    one.load_state_dict(stock1.state_dict())
    assert one.fused.t == 1 and one.fused.param_groups is None
    with torch.no_grad():
        for p, q in zip(a, b):
            p.copy_(q)
    grads = _grads(45)
    one.zero_grad()
    _feed(a, grads)
    _feed(b, grads)
    one.step()
    stock1.step()
    _close(a, b)
    with pytest.raises(Exception, match='group'):
        one.load_state_dict(stock.state_dict())                # two groups into one


def test_reference_loop_follows_trainer_step_bit_for_bit(manifest):
    """the loop of test_reference_training_loop_with_stock_torch_adam with efgh_amd.optim.Adam in place of torch's: the gradient,
    the losses and the weights are those of Trainer.step on a twin model, bit for bit"""
    from efgh_amd import ops
    from efgh_amd.losses import EFGHCriterion
    from efgh_amd.nets import EFGHBackbone
    from efgh_amd.optim import Adam
    from efgh_amd.train import Trainer
    args = syn.default_args(RAW, 'cuda')
    sd = syn.synthetic_state_dict(manifest['state_dict'], 1)
    m_ref, m_tr = EFGHBackbone(args), EFGHBackbone(args)
    m_ref.load_state_dict(sd); m_tr.load_state_dict(sd)
    m_ref, m_tr = m_ref.cuda(), m_tr.cuda()
    criterion = EFGHCriterion(args)
    optimizer = Adam((p for p in m_ref.parameters() if p.requires_grad), lr=1e-3, weight_decay=0.0)
    tr = Trainer(m_tr, EFGHCriterion(args), lr=1e-3)
    b = syn.make_batch(RAW, NPTS, 2)
    pcd, img, calib, A = [torch.from_numpy(b[k]).cuda().float() for k in ('pc', 'img', 'calib', 'A')]
    gt = {k: torch.from_numpy(v) for k, v in b['gt'].items()}
    flat = optimizer.flat
    m_ref.train()

    def forward_backward(zero):
        pred = m_ref(pcd, img, calib, A)
        losses, _ = criterion.compute_loss(pcd, img, calib, A, dict(gt), pred)
        if zero:
            optimizer.zero_grad()
        losses['total'].backward()
        ops.join_side_streams(flat.g)
        return losses

    for it in range(2):
        losses = forward_backward(True)
        g_ref = flat.g.clone()
        optimizer.step()
        l_tr, _ = tr.step(pcd, img, calib, A, dict(gt))
        if it == 0:
            assert torch.equal(bits(g_ref), bits(tr.flat.g)), int((bits(g_ref) != bits(tr.flat.g)).sum())
        assert torch.equal(bits(losses['total'].detach().reshape(1)), bits(l_tr['total'].detach().reshape(1))), it
    assert torch.equal(bits(flat.w), bits(tr.flat.w))
    for p, q in zip(m_ref.parameters(), m_tr.parameters()):
        assert torch.equal(bits(p), bits(q))
    # a second backward without zero_grad accumulates, as under torch: g + g
    forward_backward(True)
    once = flat.g.double()
    forward_backward(False)
    err = (flat.g.double() - 2.0 * once).abs()
    tol = 2.0 ** -24 * (2.0 * once).abs() * (1.0 + 2.0 ** -20) + 2.0 ** -149        # one fp32 rounding of the sum
    assert bool((err <= tol).all()), float((err - tol).max())
    assert float(once.abs().max()) > 0.0


def _g_slice(tr):
    names = [k for k, p in tr.model.named_parameters() if p.requires_grad]
    idx = [i for i, k in enumerate(names) if k.startswith('G.')]
    assert idx == list(range(idx[0], idx[-1] + 1)) and 0 < len(idx) < len(names)
    return tr.flat.offsets[idx[0]][0], sum(tr.flat.offsets[idx[-1]])


def test_trainer_param_groups_by_name(world):
    grouped = trainer(world, lr=1e-3, skip_nonfinite=True, param_groups=[{'names': ['G.'], 'lr': 1e-4}])
    twin = trainer(world, lr=1e-4, skip_nonfinite=True)
    assert [g['name'] for g in grouped.opt.param_groups] == ['G.', 'default']
    assert [g['lr'] for g in grouped.opt.param_groups] == [1e-4, 1e-3]
    w0 = grouped.flat.w.clone()
    # the twin runs the ungrouped kernel over the WHOLE buffer, the grouped launch holds G to that kernel run on G alone: the two
    # differ in which (at most 3) elements take the kernel's twice-rounded tail form of m and v.  From zero moments the forms
    # coincide (b * 0 is exact), which is what makes this first step comparable bit for bit whatever G's length and position
    assert not bool(grouped.opt.m.any()) and not bool(grouped.opt.v.any()) and not bool(twin.opt.m.any()) and not bool(twin.opt.v.any())
    step(grouped, world, 0)
    step(twin, world, 0)
    a, e = _g_slice(grouped)
    assert torch.equal(bits(grouped.flat.w[a:e]), bits(twin.flat.w[a:e]))              # G moved with its own rate
    assert not torch.equal(bits(grouped.flat.w[a:e]), bits(w0[a:e]))
    rest = torch.cat([grouped.flat.w[:a], grouped.flat.w[e:]]), torch.cat([twin.flat.w[:a], twin.flat.w[e:]])
    assert float((bits(rest[0]) != bits(rest[1])).float().mean()) > 0.5                # the rest with the global one
    assert grouped.guard_stats()['applied'] == 1
    # an accumulated step over two micro-batches runs through the same launch
    w1 = grouped.flat.w.clone()
    grouped.step_accumulated([mb(world, 1), mb(world, 2)])
    st = grouped.guard_stats()
    assert st['applied'] == 2 and st['skipped'] == 0 and not torch.equal(bits(w1), bits(grouped.flat.w))


def test_trainer_param_groups_skip_a_nonfinite_step_in_every_group(world):
    tr = trainer(world, bad_calls=(2,), lr=1e-3, skip_nonfinite=True, param_groups=[{'names': ['G.'], 'lr': 1e-4}])
    step(tr, world, 0)
    before = [bits(t) for t in (tr.flat.w, tr.opt.m, tr.opt.v)]
    step(tr, world, 1)                                         # the criterion multiplies `total` by inf: a NaN / inf gradient
    st = tr.guard_stats()
    assert st['skipped'] == 1 and st['applied'] == 1 and st['nonfinite'] > 0
    for t, b in zip((tr.flat.w, tr.opt.m, tr.opt.v), before):
        assert torch.equal(bits(t), b)
