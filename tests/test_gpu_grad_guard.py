"""Gradient guard on the GPU: the measure pass against exact float64 sums, the decide rule, the guarded fused Adam against the
float64 contract (tests/grad_guard_contract.py) and torch's clip_grad_norm_ + Adam, and Trainer with clipping / skipping."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from efgh_amd import _C, synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_guard_contract as contract  # noqa: E402
from train_harness import INF, RAW, bits as _bits, census, step as _step, trainer as _trainer, waits_for_nothing, world  # noqa: E402,F401

pytestmark = pytest.mark.gpu
L = _C.GUARD_RUN
SIZES = [1, 2, 3, 4, 5, 255, 256, 257, L - 1, L, L + 1, 3 * L + 5, 1000003]


def _measure(g, bounds, max_norm=INF, grad_scale=1.0, skip=0, step=1, grid=0, state=None):
    """one efgh_grad_guard_measure call on a device tensor -> (GuardState, its raw bytes).  The workspace starts as NaN / -1 words:
    a run the kernels failed to write would show."""
    lib = _C.lib()
    n = g.numel()
    ws = torch.full((lib.efgh_grad_guard_workspace(n),), 255, dtype=torch.uint8, device='cuda')
    if state is None:
        state = torch.zeros(ctypes.sizeof(_C.GuardState), dtype=torch.uint8, device='cuda')
    arr = (ctypes.c_int64 * len(bounds))(*bounds)
    _C.check(lib.efgh_grad_guard_measure(g.data_ptr(), n, arr, len(bounds) - 1, max_norm, grad_scale, skip, 0.9, 0.999, step,
                                         ws.data_ptr(), state.data_ptr(), grid, _C.stream_ptr()))
    raw = state.cpu().numpy().tobytes()
    return _C.GuardState.from_buffer_copy(raw), raw


def _segment_sets(n):
    """one segment; (0, 3, 3+L+1, n) where it fits; eight segments with odd boundaries (as many one-element segments as fit, n < 8)"""
    sets = [(0, n)]
    if 3 + L + 1 < n:
        sets.append((0, 3, 3 + L + 1, n))
    if 1 < n <= 16:
        sets.append(tuple(range(min(8, n))) + (n,))
    elif n > 16:
        inner = [int(n * f) | 1 for f in (0.07, 0.19, 0.33, 0.5, 0.61, 0.78, 0.93)]
        assert all(a < b for a, b in zip([0] + inner, inner + [n]))
        sets.append((0,) + tuple(inner) + (n,))
    return sets


def _values(kind, n, seed):
    rs = np.random.RandomState(seed)
    if kind == 'mixed':                      # normal times 10^U(-20, 18)
        return (rs.standard_normal(n) * 10.0 ** rs.uniform(-20, 18, n)).astype(np.float32)
    if kind == 'huge':                       # +-3e38: every fp32 square overflows
        return (np.float32(3e38) * rs.choice([-1.0, 1.0], n)).astype(np.float32)
    return np.zeros(n, np.float32)


@pytest.mark.parametrize('n', SIZES)
def test_measure_matches_exact_sums_and_is_reproducible(n):
    """per-segment sum of squares against math.fsum of the exact double products: relative error <= (n_s + 1) * 2^-53, the worst
    case of ANY order of float64 additions of non-negative terms (an fp32 accumulation misses it by orders of magnitude from a few
    hundred elements on); two runs and a run on a different launch grid give the same bits"""
    for kind in ('mixed', 'huge', 'zeros'):
        x = _values(kind, n, seed=n % 1000)
        p = x.astype(np.float64) ** 2            # exact: 48-bit products
        g = torch.from_numpy(x).cuda()
        for bounds in _segment_sets(n):
            st, raw = _measure(g, bounds)
            assert st.nseg == len(bounds) - 1 and st.nonfinite_total == 0 and st.skip == 0
            total = 0.0
            for s, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
                want = math.fsum(p[a:b])
                err = abs(st.sumsq[s] - want)
                print(kind, n, bounds, s, 'rel err', err / want if want else err)
                assert err <= (b - a + 1) * 2.0 ** -53 * want, (kind, bounds, s, st.sumsq[s], want)
                assert st.nonfinite[s] == 0
                total += st.sumsq[s]
            assert st.sumsq_total == total                                   # the segment values added in index order
            assert all(st.sumsq[s] == 0.0 and st.nonfinite[s] == 0 for s in range(len(bounds) - 1, _C.GUARD_MAX_SEGMENTS))
            assert _measure(g, bounds)[1] == raw
            assert _measure(g, bounds, grid=3)[1] == raw and _measure(g, bounds, grid=1)[1] == raw


def test_measure_counts_nonfinite_elements_exactly():
    """inf, -inf and NaN at the first element, the last element, a segment's last element and on both sides of a run boundary"""
    n = 3 * L + 5
    bounds = (0, 3, 3 + L + 1, n)
    base = _values('mixed', n, 11)
    run_edge = bounds[2] + L                      # first element of the second run of the third segment
    placements = {'first': [0], 'last': [n - 1], 'segment_end': [2, bounds[2] - 1], 'run_boundary': [run_edge - 1, run_edge],
                  'all': [0, n - 1, 2, bounds[2] - 1, run_edge - 1, run_edge]}
    for name, idx in placements.items():
        for j, bad in enumerate((np.inf, -np.inf, np.nan)):
            x = base.copy()
            x[idx] = bad
            if name == 'all':
                x[idx] = [(np.inf, -np.inf, np.nan)[(i + j) % 3] for i in range(len(idx))]
            want = [int((~np.isfinite(x[a:b])).sum()) for a, b in zip(bounds[:-1], bounds[1:])]
            st, raw = _measure(torch.from_numpy(x).cuda(), bounds)
            assert [st.nonfinite[s] for s in range(3)] == want and st.nonfinite_total == sum(want), (name, bad, want)
            for s in range(3):                    # a clean segment keeps a finite sum
                assert math.isfinite(st.sumsq[s]) == (want[s] == 0)
            assert st.skip == 0 and st.applied == 1                           # not asked to skip: the step counts
            st2, _ = _measure(torch.from_numpy(x).cuda(), bounds, skip=1)
            assert st2.skip == 1 and st2.applied == 0 and st2.skipped == 1


def _bias_corrections_ok(st, t):
    """bc1 = 1 - beta1^t and bc2_sqrt = sqrt(1 - beta2^t) in fp32 arithmetic on the fp32 betas, as efgh_adam_step forms them (the
    cancellation in 1 - 0.999f^t is part of that recipe); the power may be off by one fp32 rounding (2^-24 below 1), which the
    subtraction passes on unchanged and the square root divides by 2 sqrt(bc2)"""
    b1, b2 = np.float64(np.float32(0.9)), np.float64(np.float32(0.999))
    ref1 = np.float32(1) - np.float32(b1 ** t)
    ref2 = np.sqrt(np.float32(1) - np.float32(b2 ** t), dtype=np.float32)
    return abs(st.bc1 - ref1) <= 2.0 ** -23 and abs(st.bc2_sqrt - ref2) <= 2.0 ** -23 / (2 * float(ref2)) + 2.0 ** -24


def _one_ulp32(got, want):
    want = np.float32(want)
    return abs(np.float32(got) - want) <= np.spacing(want)


@pytest.mark.parametrize('case', ['generic', 'tiny', 'measure_only', 'zeros', 'half_scale'])
def test_decide_rule(case):
    n = 5000
    x = np.random.RandomState(3).standard_normal(n).astype(np.float32) * 3
    max_norm, gs = 1.0, 1.0
    if case == 'tiny':                            # norm ~1e-7 with max_norm 1e-7: torch's + 1e-6 decides, 0.09 and not 1
        x = np.zeros(n, np.float32)
        x[17] = 1e-7
        max_norm = 1e-7
    elif case == 'measure_only':
        max_norm = INF
    elif case == 'zeros':
        x = np.zeros(n, np.float32)
    elif case == 'half_scale':
        gs = 0.5
    bounds = (0, 1001, 2048, n)
    st, _ = _measure(torch.from_numpy(x).cuda(), bounds, max_norm=max_norm, grad_scale=gs, step=5)
    sums = [st.sumsq[s] for s in range(3)]
    want = contract.decide(sums, [0, 0, 0], max_norm, gs, False, 4, 0)
    assert abs(st.norm - want['norm']) <= 4e-16 * want['norm']
    assert _one_ulp32(st.coef, want['coef']), (st.coef, want['coef'])
    assert st.scale == np.float32(gs) * np.float32(st.coef)
    assert st.applied == 5 and st.skipped == 0 and st.skip == 0
    assert _bias_corrections_ok(st, 5), (st.bc1, st.bc2_sqrt)
    if case == 'tiny':
        assert 0.0908 < st.coef < 0.0910
    if case in ('measure_only', 'zeros'):
        assert st.coef == 1.0 and st.scale == gs
    if case == 'half_scale':
        full, _ = _measure(torch.from_numpy(x).cuda(), bounds, max_norm=max_norm, grad_scale=1.0)
        assert abs(st.norm - 0.5 * full.norm) <= 4e-16 * st.norm and st.coef > full.coef


def test_decide_counts_steps_on_the_device_when_skipping():
    """skip_nonfinite: applied / skipped are carried in the state block from call to call, the bias corrections follow `applied`"""
    x = np.random.RandomState(4).standard_normal(777).astype(np.float32)
    bad = x.copy()
    bad[500] = np.nan
    state = torch.zeros(ctypes.sizeof(_C.GuardState), dtype=torch.uint8, device='cuda')
    seen = []
    for arr in (x, bad, x, bad, bad, x):
        st, _ = _measure(torch.from_numpy(arr).cuda(), (0, 777), max_norm=1.0, skip=1, step=0, state=state)
        seen.append((st.applied, st.skipped, st.skip))
        assert st.applied == 0 or _bias_corrections_ok(st, st.applied), (st.applied, st.bc1, st.bc2_sqrt)
    assert seen == [(1, 0, 0), (1, 1, 1), (2, 1, 0), (2, 2, 1), (2, 3, 1), (3, 3, 0)]


# ---- guarded FusedAdam on a flat buffer of three fake parameters, n = 20 003 ----
class _Three(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(7)
        self.p0 = torch.nn.Parameter(torch.randn(100, 100, generator=g))
        self.p1 = torch.nn.Parameter(torch.randn(7000, generator=g))
        self.p2 = torch.nn.Parameter(torch.randn(3, 1001, generator=g) * 0.01)


SEG3 = [('p0', 0, 10000), ('p1', 10000, 17000), ('p2', 17000, 20003)]


def _flat3():
    from efgh_amd.train import FlatParams
    flat = FlatParams(_Three().cuda())
    assert flat.n == 20003
    return flat


def _yardstick(w, w64):
    """the project's FusedAdam-vs-torch bound (tests/test_gpu_train.py): |w - w64| <= 2e-6 + 1e-5 max|w64|"""
    d = float(np.abs(w.astype(np.float64) - w64).max())
    return d, 2e-6 + 1e-5 * float(np.abs(w64).max())


def test_guarded_adam_five_steps_clip_and_skip():
    """gradient scales 1e-3, 1e2, a NaN step, 1e-1, 3e4 with max_norm 1, grad_scale 0.5, lr 1e-3, skipping on: the weights follow
    the float64 contract (which follows torch, test_grad_guard_host.py) within the FusedAdam yardstick after every applied step;
    the NaN step leaves w, m, v bit-unchanged and does not count"""
    from efgh_amd.train import FusedAdam
    flat = _flat3()
    opt = FusedAdam(flat, lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True, segments=SEG3)
    grads = contract.gradients(flat.n, seed=2)
    ref = contract.run(flat.w.cpu().numpy(), grads, 1.0, 0.5, 1e-3, skip_nonfinite=True)
    for k, (g, (w64, m64, v64, d)) in enumerate(zip(grads, ref)):
        before = [_bits(t) for t in (flat.w, opt.m, opt.v)]
        flat.g.copy_(torch.from_numpy(g))
        opt.step(grad_scale=0.5)
        stats = opt.guard_stats()
        assert (stats['applied'], stats['skipped']) == (d['applied'], d['skipped']), (k, stats)
        if d['skip']:
            assert k == 2 and stats['nonfinite'] == 1 and stats['skipped'] == 1 and stats['applied'] == 2
            for b, t in zip(before, (flat.w, opt.m, opt.v)):
                assert torch.equal(b, _bits(t))
            continue
        assert stats['nonfinite'] == 0
        assert _one_ulp32(stats['coef'], d['coef']) and abs(stats['norm'] - d['norm']) <= 1e-12 * d['norm']
        assert abs(sum(v * v for v in stats['norms'].values()) - stats['norm'] ** 2) <= 1e-12 * stats['norm'] ** 2
        got, tol = _yardstick(flat.w.cpu().numpy(), w64)
        print('step', k, 'coef', stats['coef'], 'max |w - w64|', got, 'bound', tol)
        assert got <= tol, (k, got, tol)
        assert float(np.abs(opt.m.cpu().numpy() - m64).max()) <= 1e-5 * float(np.abs(m64).max()) + 1e-12
    assert opt.t == 4 and opt.guard_stats()['skipped'] == 1
    opt.t = 9                                      # the setter writes both sides
    assert opt.guard_stats()['applied'] == 9 and opt._t == 9


def test_guarded_adam_is_bit_identical_to_the_plain_step_when_it_only_measures():
    from efgh_amd.train import FusedAdam
    fa, fb = _flat3(), _flat3()
    assert torch.equal(fa.w, fb.w)
    guarded = FusedAdam(fa, lr=1e-3, max_grad_norm=INF, segments=SEG3)
    plain = FusedAdam(fb, lr=1e-3)
    grads = contract.gradients(fa.n, seed=3, scales=(1e-3, 1e2, 1e-1))
    for g in grads:
        fa.g.copy_(torch.from_numpy(g)); fb.g.copy_(torch.from_numpy(g))
        guarded.step(grad_scale=0.5); plain.step(grad_scale=0.5)
        for a, b in ((fa.w, fb.w), (guarded.m, plain.m), (guarded.v, plain.v)):
            assert torch.equal(_bits(a), _bits(b))
    assert guarded.t == 3 and type(guarded.t) is int and plain.t == 3
    stats = guarded.guard_stats()
    assert stats['applied'] == 3 and stats['coef'] == 1.0 and stats['skipped'] == 0
    assert float((fa.w - _flat3().w).abs().max()) > 0


def test_nonfinite_gradient_propagates_as_in_torch_without_skipping():
    from efgh_amd.train import FusedAdam
    flat = _flat3()
    opt = FusedAdam(flat, lr=1e-3, max_grad_norm=1.0, segments=SEG3)
    g = contract.gradients(flat.n, seed=2)[2]
    assert np.isnan(g).sum() == 1
    flat.g.copy_(torch.from_numpy(g))
    opt.step()
    assert bool(torch.isnan(flat.w).all())           # clip_grad_norm_(error_if_nonfinite=False): a NaN coefficient, NaN weights
    stats = opt.guard_stats()
    assert stats['nonfinite'] == 1 and stats['applied'] == 1 and stats['skipped'] == 0 and math.isnan(stats['coef'])


# ---- Trainer, small configuration of tests/test_gpu_train.py (tests/train_harness.py) ----
@pytest.fixture(scope='module')
def default_run(world):
    """a Trainer with defaults after batches 0 and 2"""
    tr = _trainer(world)
    _step(tr, world, 0)
    w1 = tr.flat.w.clone()
    _step(tr, world, 2)
    return {'tr': tr, 'w1': w1, 'w2': tr.flat.w.clone(), 'm2': tr.opt.m.clone(), 'v2': tr.opt.v.clone()}


@pytest.fixture(scope='module')
def measured_run(world):
    """a Trainer that only measures (max_grad_norm = inf) after batch 0"""
    tr = _trainer(world, max_grad_norm=INF)
    _step(tr, world, 0)
    return {'tr': tr, 'stats': tr.guard_stats(), 'w1': tr.flat.w.clone()}


@pytest.fixture(scope='module')
def skip_run(world):
    """skip_nonfinite=True over batches 0, 1, 2 with the loss of the second step multiplied by inf"""
    tr = _trainer(world, bad_calls=(2,), skip_nonfinite=True)
    _step(tr, world, 0)
    before = [_bits(t) for t in (tr.flat.w, tr.opt.m, tr.opt.v)]
    losses, _ = _step(tr, world, 1)
    after = [_bits(t) for t in (tr.flat.w, tr.opt.m, tr.opt.v)]
    stats2 = tr.guard_stats()
    buffers_finite = all(bool(torch.isfinite(b).all()) for b in tr.model.buffers() if b.dtype.is_floating_point)
    _step(tr, world, 2)
    return {'tr': tr, 'before': before, 'after': after, 'stats2': stats2, 'stats3': tr.guard_stats(),
            'bad_total': float(losses['total'].detach()), 'buffers_finite': buffers_finite}


def test_trainer_defaults_change_nothing(world, default_run):
    tr = _trainer(world)
    assert not tr.opt.guarded and tr.opt.state is None and tr.opt.workspace is None      # there is no state block to touch
    _step(tr, world, 0)
    _step(tr, world, 2)
    assert torch.equal(_bits(tr.flat.w), _bits(default_run['w2']))
    assert torch.equal(_bits(tr.opt.m), _bits(default_run['m2'])) and torch.equal(_bits(tr.opt.v), _bits(default_run['v2']))
    assert tr.opt.t == 2 and type(tr.opt.t) is int
    with pytest.raises(_C.EfghError):
        tr.guard_stats()


def test_trainer_measure_only_equals_the_default_step(world, default_run, measured_run):
    """max_grad_norm = inf: the guarded route, coefficient exactly 1 - the first step gives the bits of an unguarded Trainer's"""
    assert torch.equal(_bits(default_run['w1']), _bits(measured_run['w1']))
    s = measured_run['stats']
    assert s['coef'] == 1.0 and s['applied'] == 1 and s['skipped'] == 0 and s['nonfinite'] == 0 and s['norm'] > 0


def test_trainer_clips_like_clip_grad_norm_and_adam(world, measured_run):
    """max_grad_norm = a tenth of the first step's norm: coef ~ 0.1, per-sub-network norms, and two steps that follow
    clip_grad_norm_ + torch.optim.Adam on shadow copies fed the same gradients, within the FusedAdam yardstick"""
    norm0 = measured_run['stats']['norm']
    mx = norm0 / 10
    tr = _trainer(world, max_grad_norm=mx)
    assert [s[0] for s in tr.opt.segments] == ['E', 'H', 'F', 'G']
    shadow = [p.detach().clone().requires_grad_(True) for p in tr.flat.params]
    opt = torch.optim.Adam(shadow, lr=1e-3, weight_decay=0.0)
    for it in range(2):
        _step(tr, world, 0)
        s = tr.guard_stats()
        assert s['nonfinite'] == 0 and s['applied'] == it + 1 and s['skipped'] == 0
        assert _one_ulp32(s['coef'], min(1.0, mx / (s['norm'] + 1e-6)))
        if it == 0:
            assert abs(s['norm'] - norm0) <= 1e-12 * norm0 and abs(s['coef'] - 0.1) < 1e-4
        assert list(s['norms']) == ['E', 'H', 'F', 'G'] and all(v > 0 for v in s['norms'].values())
        assert abs(sum(v * v for v in s['norms'].values()) - s['norm'] ** 2) <= 1e-12 * s['norm'] ** 2
        for q, p in zip(shadow, tr.flat.params):
            q.grad = p.grad.detach().clone()
        torch.nn.utils.clip_grad_norm_(shadow, mx)
        opt.step()
        for q, p in zip(shadow, tr.flat.params):
            d = float((q.detach() - p.detach()).abs().max())
            assert d <= 2e-6 + 1e-5 * float(q.detach().abs().max()), (it, d)


def test_trainer_skips_a_nonfinite_step(world, skip_run):
    r = skip_run
    assert not math.isfinite(r['bad_total']) and r['buffers_finite']          # finite forward and BatchNorm buffers, infinite loss
    for b, a in zip(r['before'], r['after']):                                 # all 353 parameters and both moments: same bits
        assert torch.equal(b, a)
    assert r['stats2']['skipped'] == 1 and r['stats2']['applied'] == 1 and r['stats2']['nonfinite'] > 0
    assert r['stats3']['skipped'] == 1 and r['stats3']['applied'] == 2 and r['stats3']['nonfinite'] == 0
    assert len(r['tr'].flat.params) == 353
    # the third step against a run that never saw the bad batch, only batches 0 and 2 (the same guarded route, so that not even a
    # last-bit difference of a bias correction can flip one of the network's discontinuous heads between the two runs)
    tr = r['tr']
    clean = _trainer(world, skip_nonfinite=True)
    _step(clean, world, 0)
    _step(clean, world, 2)
    assert clean.guard_stats()['applied'] == 2 and clean.guard_stats()['skipped'] == 0
    off_w = clean.flat.w
    for (off, k) in tr.flat.offsets:
        a, b = tr.flat.w[off:off + k], off_w[off:off + k]
        d = float((a - b).abs().max())
        assert d <= 2e-6 + 1e-5 * float(b.abs().max()), (off, d)
    assert bool(torch.isfinite(tr.flat.w).all())


def test_checkpoint_carries_the_applied_step_count(world, skip_run):
    from efgh_amd.io import checkpoint as ck
    from efgh_amd.nets import EFGHBackbone
    from efgh_amd.train import FlatParams, FusedAdam
    tr = skip_run['tr']
    sd = ck.adam_state_dict(tr.opt)
    assert len(sd['state']) == 353 and all(int(st['step']) == 2 for st in sd['state'].values())      # three calls, two applied
    flat = FlatParams(EFGHBackbone(syn.default_args(RAW, 'cuda')).cuda())
    opt = FusedAdam(flat, lr=1e-3, skip_nonfinite=True)
    ck.load_adam_state(opt, sd)
    assert opt.t == 2 and opt.guard_stats()['applied'] == 2
    assert torch.equal(opt.m, tr.opt.m)
    flat.g.copy_(tr.flat.g)                        # (the finite gradient of the third step)
    opt.step()
    s = opt.guard_stats()
    assert opt.t == 3 and s['applied'] == 3 and s['skipped'] == 0
    assert _bias_corrections_ok(_C.GuardState.from_buffer_copy(opt.state.cpu().numpy().tobytes()), 3)


def test_guarded_step_adds_no_aten_ops_and_no_host_sync(world, default_run, measured_run):
    plain, guarded = default_run['tr'], measured_run['tr']
    for tr in (plain, guarded):
        _step(tr, world, 0)
    n_plain = sum(census(lambda: _step(plain, world, 0)).values())
    n_guarded = sum(census(lambda: _step(guarded, world, 0)).values())
    assert n_guarded <= n_plain, (n_guarded, n_plain)
    # the optimizer step alone: no aten op at all, and nothing that waits for the device
    assert sum(census(lambda: guarded.opt.step()).values()) == 0
    waits_for_nothing(guarded.opt.step)
