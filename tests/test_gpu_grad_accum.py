"""Gradient accumulation over micro-batches on the GPU: the drain and valid-count kernels bit for bit / count for count, and
Trainer.step_accumulated on the small configuration of tests/test_gpu_train.py - one micro-batch is a plain step, the accumulator
holds the sequential fp32 sum, k micro-batches mean what k DataParallel replicas mean, the guard sees the sum, the bookkeeping,
the memory of ONE micro-batch, and no host synchronisation in the new pieces."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from efgh_amd import _C, ops, synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_accum_contract as contract  # noqa: E402
from train_harness import INF, RAW, batch, bits as _bits, census, make_world, mb as _mb, model as _model, trainer as _trainer, waits_for_nothing  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1000003]        # the float4 and tail edges
SPECIALS = [0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-40, 1.1754942e-38]    # +-0, +-inf, denormals


# ---- efgh_grad_drain ----
def _gradient(n, seed):
    """normals times 10^U(-20, 18) with +0, -0, +-inf and denormals scattered in (at other places for every seed)"""
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal(n) * 10.0 ** rs.uniform(-20, 18, n)).astype(np.float32)
    reps = max(1, min(50, n // 40))
    where = rs.permutation(n)[:min(n, len(SPECIALS) * reps)]
    for j, i in enumerate(where):
        x[i] = np.float32(SPECIALS[(j + seed) % len(SPECIALS)])
    return x


@pytest.mark.parametrize('n', SIZES)
def test_drain_holds_the_bits_of_the_sequential_sum(n):
    gs = [torch.from_numpy(_gradient(n, 10 * (n % 1000) + j)).cuda() for j in range(3)]
    want = (gs[0] + gs[1]) + gs[2]                                 # torch's own fp32 adds on the device
    zeros = torch.zeros(n, dtype=torch.int32, device='cuda')
    acc = torch.full((n,), float('nan'), device='cuda')            # a first drain never reads it
    g = torch.empty(n, device='cuda')
    for j in range(3):
        g.copy_(gs[j])
        ops.grad_drain(acc, g, j == 0)
        assert torch.equal(_bits(g), zeros)                        # all +0
        if j == 0:
            assert torch.equal(_bits(acc), _bits(gs[0]))           # a copy: -0 stays -0, the NaN fill is gone
    assert torch.equal(_bits(acc), _bits(want))
    host = contract.sequential_sum([t.cpu().numpy() for t in gs])
    got = acc.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(host)) and np.array_equal(got[~np.isnan(got)], host[~np.isnan(host)])
    if n >= 255:
        assert np.isinf(got).any() and np.isnan(got).sum() < n // 8 and np.isfinite(got).sum() > n // 2


@pytest.mark.parametrize('n', [5, 1025])
def test_drain_keeps_a_nan_of_any_one_gradient(n):
    for which in range(3):
        gs = [torch.from_numpy(np.random.RandomState(n + j).standard_normal(n).astype(np.float32)).cuda() for j in range(3)]
        at = [0, n - 1, n // 2][which]
        gs[which][at] = float('nan')
        acc, g = torch.empty(n, device='cuda'), torch.empty(n, device='cuda')
        for j in range(3):
            g.copy_(gs[j])
            ops.grad_drain(acc, g, j == 0)
        bad = torch.isnan(acc).nonzero().flatten().tolist()
        assert bad == [at], (which, bad)


def test_drain_refuses_acc_equal_g_and_launches_nothing():
    x = torch.from_numpy(_gradient(1025, 1)).cuda()
    before = _bits(x)
    for first in (0, 1):
        assert _C.lib().efgh_grad_drain(x.data_ptr(), x.data_ptr(), x.numel(), first, _C.stream_ptr()) == -1
        assert 'invalid argument' in _C.lib().efgh_last_error().decode()
    assert _C.lib().efgh_grad_drain(x.data_ptr(), x[4:].data_ptr(), 100, 0, _C.stream_ptr()) == -1      # overlapping
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), before)
    with pytest.raises(_C.EfghError):
        ops.grad_drain(x, x, True)


# ---- efgh_gimg_valid_count ----
def _depth_image(B, H, W, seed):
    rs = np.random.RandomState(seed)
    img = rs.standard_normal((B, H, W, 4)).astype(np.float32)
    d = (rs.rand(B, H, W) * 80).astype(np.float32)
    kind = rs.randint(0, 8, (B, H, W))
    d[kind == 0] = 0.0
    d[kind == 1] = -d[kind == 1] - 1
    d[kind == 2] = np.nan
    d[kind == 3] = np.inf
    img[..., 3] = d
    return torch.from_numpy(img).cuda()


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('hw', [(1, 1), (3, 5), (37, 61), (128, 256)], ids=lambda hw: '%dx%d' % hw)
def test_valid_count_is_exact_and_is_the_loss_kernels_count(hw, B):
    from efgh_amd.nets import fn as FN
    H, W = hw
    gdep = _depth_image(B, H, W, seed=H + B)
    rs = np.random.RandomState(5)
    masks = {'zeros': np.zeros((B, 1, H, W), np.uint8), 'full': np.full((B, 1, H, W), 255, np.uint8),
             'random': (rs.randint(0, 3, (B, 1, H, W)) * rs.randint(1, 128, (B, 1, H, W))).astype(np.uint8)}
    pd = torch.rand(B, 1, H, W, device='cuda')
    pm = torch.rand(B, 1, H, W, device='cuda') * 0.98 + 0.01
    for name, m in masks.items():
        mask = torch.from_numpy(m).cuda()
        want = int(((gdep[..., 3] > 0) & (mask.view(B, H, W) > 0)).sum())
        count = torch.zeros(3, dtype=torch.int64, device='cuda')
        ops.gimg_valid_count(gdep, mask, count[1:2])
        assert count.tolist() == [0, want, 0], (name, count.tolist(), want)
        ops.gimg_valid_count(gdep, mask, count[1:2])               # two calls add up
        assert count.tolist() == [0, 2 * want, 0]
        n_valid = FN.GImageLossFn.apply(pd, pm, gdep, mask)[4]
        assert int(n_valid) == want, (name, float(n_valid), want)
        if name == 'zeros':
            assert want == 0
        elif H * W > 100:
            assert 0 < want < B * H * W


# ---- Trainer, small configuration of tests/test_gpu_train.py (tests/train_harness.py) ----
@pytest.fixture(scope='module')
def world(manifest):
    return dict(make_world(manifest), singles=[batch(i, 1) for i in range(3)])


def _state(tr):
    """the bits of weights and moments - and of the average, the BatchNorm statistics and the counters where the options keep them"""
    extra = ([tr.ema.buf] if tr.ema is not None else []) + ([tr.txn.live, tr.flat.nbt] if tr.txn is not None else [])
    return [_bits(t) if t.dtype == torch.float32 else t.clone() for t in [tr.flat.w, tr.opt.m, tr.opt.v] + extra]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


ROUTES = {'plain': {}, 'skip_nonfinite': {'skip_nonfinite': True}, 'measure_only': {'max_grad_norm': INF},
          'all_options': {'max_grad_norm': 1.0, 'skip_nonfinite': True, 'transactional': True, 'ema_decay': 0.999}}


@pytest.mark.parametrize('route', list(ROUTES))
def test_one_micro_batch_is_a_plain_step(world, route):
    """what holds the two entry points of the step core together: the same kernels on the same bits, so equality is exact - with
    every option on (all_options) also for the average, the BatchNorm statistics and counters, and the guard's whole report"""
    kw = ROUTES[route]
    a, b = _trainer(world, **kw), _trainer(world, **kw)
    assert _same(_state(a), _state(b))
    assert len(_state(a)) == (6 if route == 'all_options' else 3)
    w0 = a.flat.w.clone()
    for i in (0, 2):
        la, _ = a.step(*_mb(world, i))
        lb, preds = b.step_accumulated([_mb(world, i)])
        assert _same(_state(a), _state(b)), (route, i)
        assert len(preds) == 1 and set(lb) == set(a.criterion.loss_name)
        assert all(torch.equal(la[k].detach(), lb[k]) for k in lb)
    assert a.it == b.it == 2 and a.opt.t == b.opt.t == 2
    assert float((a.flat.w - w0).abs().max()) > 0
    if route != 'plain':
        sa, sb = a.guard_stats(), b.guard_stats()
        assert sa == sb and sa['applied'] == 2
        if route == 'all_options':                                 # a finite clip: the coefficient is below 1 on this net
            assert sa['coef'] < 1.0 and sa['coef'] == sb['coef']
            assert (sa['rolled_back'], sa['forward_nonfinite']) == (0, 0) and float((a.ema.buf - a.flat.w).abs().max()) > 0
        else:
            assert sa['coef'] == 1.0


def _micro_gradient(tr, mb):
    """Trainer.step's path up to the optimizer, by hand: the flat gradient of one micro-batch"""
    pc, img, calib, A, gt = mb
    tr.flat.uses = [0] * len(tr.flat.params)
    tr.model.train()
    tr.flat.collect_ticks = True
    try:
        pred = tr.model(pc, img, calib, A)
    finally:
        tr.flat.flush_ticks()
    losses, _ = tr.criterion.compute_loss(pc, img, calib, A, gt, pred)
    tr.flat.zero_grad()
    losses['total'].backward()
    for s in ops.side_streams():
        torch.cuda.current_stream().wait_stream(s)
    return tr.flat.g.clone()


def test_accumulator_holds_the_sequential_sum_on_the_real_net(world):
    """three micro-batches of 2, plain mean: `acc` (which the optimizer kernel only reads) against the fp32 sum ((g1 + g2) + g3) of
    the three gradients a second Trainer with the same weights computes one at a time - exact because all 353 gradients are
    bit-reproducible from run to run"""
    a, b = _trainer(world), _trainer(world)
    a.step_accumulated([_mb(world, i) for i in range(3)], exact_depth_mean=False)
    clones = [_micro_gradient(b, _mb(world, i)) for i in range(3)]
    want = (clones[0] + clones[1]) + clones[2]
    assert a.accum.acc.shape == a.flat.g.shape and a.accum.acc.data_ptr() != a.flat.g.data_ptr()
    assert torch.equal(_bits(a.accum.acc), _bits(want))
    assert float(want.abs().max()) > 0 and not torch.equal(_bits(want), _bits(clones[0] + (clones[1] + clones[2])))
    assert not bool(a.flat.g.any())                                # drained
    assert a.accum.count == 0                                      # the optimizer step ended the sum


def test_three_micro_batches_equal_dataparallel_on_the_real_net(world):
    """The comparison of tests/test_gpu_dp.py::_dp_semantics_worker in one process: micro-batches = samples 0, 1, 2 at batch 1;
    reference = what `torch.nn.DataParallel` computes - three train-mode forwards (BatchNorm statistics per replica), outputs
    concatenated, ONE efghloss over the batch of three, one backward.  Bounds of tests/test_gpu_dp.py: every loss term within
    2e-5 |ref| + 1e-7, acc / k within 1e-5 relative 2-norm per sub-network; without the valid-pixel weights G deviates by more than
    10 times as much.  (lr = 0: the optimizer leaves the weights alone, both forms run on one Trainer.)
    Measured: terms within 2.3e-7 (g_depth; 7.1e-2 unweighted); gradients E 5.6e-7, H 7.1e-6, F 5.3e-6, G 8.0e-6 (5.3e-3 unweighted).
    E, H and F do not see g_depth and read the same with and without the weights: their deviation is the fp32 rounding of a
    backward pass whose upstream gradient is scaled by 1/3 in one form and not in the other (the two-rank test's 2.7e-8 scales by
    an exact 1/2 on both sides)."""
    from efgh_amd.losses import EFGHCriterion
    k = 3
    mbs = lambda: [tuple(inp) + (dict(gt),) for inp, gt in world['singles']]
    tr = _trainer(world, lr=0.0)
    w0 = _bits(tr.flat.w)
    weights = tr.depth_weights(mbs()).cpu().numpy()
    print('\nvalid-pixel weights of samples 0, 1, 2:', weights.tolist())
    assert weights.dtype == np.float32 and weights.max() / weights.min() - 1 >= 0.01      # otherwise this test shows nothing
    got = {}
    for exact in (True, False):
        losses, preds = tr.step_accumulated(mbs(), exact_depth_mean=exact)
        assert torch.equal(_bits(tr.flat.w), w0) and len(preds) == k
        got[exact] = (tr.accum.acc.double() / k, {n: float(v) for n, v in losses.items()})
    # the reference
    m = _model(world['sd']).train()
    crit = EFGHCriterion(syn.default_args(RAW, 'cuda'))
    ps = [m(*inp) for inp, _ in world['singles']]
    pred = {n: (torch.cat([p[n] for p in ps], 0) if torch.is_tensor(ps[0][n]) else ps[0][n]) for n in ps[0]}
    inp = [torch.cat([s[0][j] for s in world['singles']], 0) for j in range(4)]
    gt = {n: torch.cat([s[1][n] for s in world['singles']], 0) for n in world['singles'][0][1]}
    L, _ = crit.compute_loss(*inp, gt, pred)
    L['total'].backward()
    torch.cuda.synchronize()
    named = list(m.named_parameters())
    g_ref = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1).double() for _, p in named])
    offs = np.concatenate([[0], np.cumsum([p.numel() for _, p in named])])
    assert g_ref.numel() == tr.flat.n and [n for n, _ in named] == [n for n, _ in tr.model.named_parameters()]
    dev = {}
    for exact in (True, False):
        g, terms = got[exact]
        dev[exact] = {}
        for net in 'EHFG':
            idx = [i for i, (n, _) in enumerate(named) if n.startswith(net + '.')]
            lo, hi = int(offs[idx[0]]), int(offs[idx[-1] + 1])
            assert idx == list(range(idx[0], idx[-1] + 1))
            dev[exact][net] = float((g[lo:hi] - g_ref[lo:hi]).norm() / (g_ref[lo:hi].norm() + 1e-300))
        term_dev = {n: abs(terms[n] - float(L[n])) / (abs(float(L[n])) + 1e-12) for n in crit.loss_name}
        print('  count-weighted=%s: worst term deviation %.2e (%s); g_depth %.3e; gradient deviation per sub-net %s' % (
            exact, max(term_dev.values()), max(term_dev, key=term_dev.get), term_dev['g_depth'],
            {n: '%.1e' % v for n, v in dev[exact].items()}))
    terms = got[True][1]
    for n in crit.loss_name:
        ref = float(L[n])
        assert abs(terms[n] - ref) <= 2e-5 * abs(ref) + 1e-7, (n, terms[n], ref)
    assert all(v < 1e-5 for v in dev[True].values()), dev[True]
    assert dev[False]['G'] > 10 * dev[True]['G'], (dev[False], dev[True])


def test_a_nonfinite_micro_batch_skips_the_whole_accumulated_step(world):
    tr = _trainer(world, bad_calls=(2,), skip_nonfinite=True)
    before = _state(tr)
    losses, _ = tr.step_accumulated([_mb(world, i) for i in range(3)])     # criterion calls 1, 2, 3: the second is bad
    s = tr.guard_stats()
    assert _same(before, _state(tr))                                        # w, m, v bit-unchanged
    assert s['applied'] == 0 and s['skipped'] == 1 and s['nonfinite'] > 0 and tr.opt.t == 0
    assert not math.isfinite(float(losses['total'])) and math.isfinite(float(losses['g_depth']))
    assert tr.it == 1                                                       # (as `step`: the iteration counter counts calls)
    tr.step_accumulated([_mb(world, i) for i in range(3)])                  # calls 4, 5, 6: clean
    s = tr.guard_stats()
    assert s['applied'] == 1 and s['skipped'] == 1 and s['nonfinite'] == 0 and tr.opt.t == 1
    assert not _same(before, _state(tr)) and bool(torch.isfinite(tr.flat.w).all())


def test_the_guard_measures_the_accumulated_mean_gradient(world):
    """max_grad_norm = inf: `norm` is the 2-norm of acc / k in float64, to 1e-12 (k = 2: 1 / k is an exact fp32 number).  For k = 3
    the kernels take grad_scale as an fp32 argument: the norm is that of acc * fp32(1 / 3) to 1e-12, hence of acc / 3 to the
    2^-24 of that one rounding."""
    tr = _trainer(world, max_grad_norm=INF)
    for k in (2, 3):
        tr.step_accumulated([_mb(world, i) for i in range(k)])
        s = tr.guard_stats()
        raw = float(tr.accum.acc.double().pow(2).sum().sqrt())
        print('k', k, 'norm', s['norm'], 'float64 |acc| / k', raw / k)
        assert s['coef'] == 1.0 and s['nonfinite'] == 0 and raw > 0
        if k == 2:
            assert abs(s['norm'] - raw / k) <= 1e-12 * (raw / k)
        else:
            applied = raw * float(np.float32(1.0 / k))
            assert abs(s['norm'] - applied) <= 1e-12 * applied
            assert abs(s['norm'] - raw / k) <= (2.0 ** -24 + 1e-12) * (raw / k)
        assert abs(sum(v * v for v in s['norms'].values()) - s['norm'] ** 2) <= 1e-9 * s['norm'] ** 2
    assert tr.guard_stats()['applied'] == 2


def test_bookkeeping_and_the_micro_batches_argument(world):
    """one accumulated step of k = 3 through `step(..., micro_batches=3)` on the concatenated batch of 6: one iteration, one Adam
    step, three BatchNorm ticks; then a plain step() - against a Trainer that took the same two updates through
    step_accumulated([..]) on the explicit micro-batches and step_accumulated([b])"""
    a, b = _trainer(world), _trainer(world)
    cat = [torch.cat([world['batches'][i][0][j] for i in range(3)], 0) for j in range(4)]
    gt = {n: torch.cat([world['batches'][i][1][n] for i in range(3)], 0) for n in world['batches'][0][1]}
    nbt0 = a.flat.nbt.clone()
    assert nbt0.numel() > 50
    losses, preds = a.step(*cat, gt, micro_batches=3)
    assert a.it == 1 and a.opt.t == 1 and len(preds) == 3 and set(losses) == set(a.criterion.loss_name)
    assert torch.equal(a.flat.nbt, nbt0 + 3)
    assert all(int(m.num_batches_tracked) == int(nbt0[j]) + 3 for j, m in enumerate(a.flat._bns))
    assert all(p.grad.data_ptr() == a.flat.g.data_ptr() + 4 * off for p, (off, _) in zip(a.flat.params, a.flat.offsets))
    assert a.opt.lr == 1e-3
    b.step_accumulated([_mb(world, i) for i in range(3)])
    assert _same(_state(a), _state(b))                             # the slices of the concatenated batch are the micro-batches
    a.step(*_mb(world, 1))
    b.step_accumulated([_mb(world, 1)])
    assert _same(_state(a), _state(b))
    assert a.it == b.it == 2 and a.opt.t == b.opt.t == 2 and torch.equal(a.flat.nbt, b.flat.nbt) and torch.equal(a.flat.nbt, nbt0 + 4)
    assert all(p.grad.data_ptr() == a.flat.g.data_ptr() + 4 * off for p, (off, _) in zip(a.flat.params, a.flat.offsets))
    for bf_a, bf_b in zip(a.model.buffers(), b.model.buffers()):   # BatchNorm running statistics: per micro-batch, the same
        assert torch.equal(bf_a, bf_b)
    with pytest.raises(_C.EfghError, match='4'):
        a.step(*cat, gt, micro_batches=4)
    assert a.it == 2


def _storage_bytes(objs):
    seen = {}
    for t in objs:
        if torch.is_tensor(t) and t.is_cuda:
            st = t.untyped_storage()
            seen[st.data_ptr()] = st.nbytes()
    return sum(seen.values())


def test_activation_memory_is_that_of_one_micro_batch(world):
    tr = _trainer(world)
    mbs = [_mb(world, i) for i in range(3)]
    tr.step_accumulated(mbs)                                       # warm-up: the accumulator, caches and workspaces exist
    torch.cuda.synchronize()

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(), out

    p3, (_, preds) = peak(lambda: tr.step_accumulated(mbs))
    retained = _storage_bytes(list(mbs[2][:4]) + list(mbs[2][4].values()) + list(preds[2].values()))
    del preds
    p2, out = peak(lambda: tr.step_accumulated(mbs[:2]))
    del out
    cat = [torch.cat([mb[j] for mb in mbs], 0) for j in range(4)]
    gt = {n: torch.cat([mb[4][n] for mb in mbs], 0) for n in mbs[0][4]}
    p6, out = peak(lambda: tr.step(*cat, gt))
    del out
    print('\npeak bytes: 3 micro-batches of 2: %d, 2 micro-batches of 2: %d (difference %d, one micro-batch retains %d), '
          'step at batch 6: %d' % (p3, p2, p3 - p2, retained, p6))
    assert p3 - p2 <= retained + (1 << 20)
    assert p3 < p6


def test_no_host_sync_and_no_aten_op_in_the_new_pieces(world):
    tr = _trainer(world)
    mbs = [mb[:4] + ({n: v.cuda() for n, v in mb[4].items()},) for mb in (_mb(world, i) for i in range(3))]
    tr.step_accumulated(mbs)
    tr.flat.g.normal_()
    assert sum(census(lambda: tr.accum.drain()).values()) == 0
    assert not bool(tr.flat.g.any()) and bool(tr.accum.acc.any())
    want = contract.depth_weights([int(((ops.depth_image(mb[0], mb[4]['cam_T_velo'].float(), *RAW)[0][..., 3] > 0)
                                        & (mb[4]['img_mask'].view(-1, *RAW) > 0)).sum()) for mb in mbs])
    assert np.array_equal(tr.depth_weights(mbs).cpu().numpy(), want)      # the weight rule of the contract, bit for bit
    waits_for_nothing(lambda: (tr.accum.drain(), tr.depth_weights(mbs)))


def test_example_loop_accumulates():
    """examples/train_synthetic.py --accumulate 2: GPU sample preparation -> Trainer.step(micro_batches=2) -> error meter"""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'train_synthetic.py')
    spec = importlib.util.spec_from_file_location('train_synthetic_accum', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hist = mod.main(['--iters', '2', '--batch', '2', '--accumulate', '2', '--raw', '128', '256', '--points', '2048'])
    assert len(hist) == 2 and all(np.isfinite(h) for h in hist)
