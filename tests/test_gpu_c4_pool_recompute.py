"""The pooled 4-channel input layers in training without their full-resolution raw map (ops.C4_POOL_RECOMPUTE; csrc/c4conv.hip's
statistics-only, train-mode pooled and recomputing-apply kernels, backward.hip's raw_win reduction) against the stored-raw kernels
they replace, on the same inputs.  Every comparison is torch.equal on the fp32 (and float64) tensors: the path is bit-identical or
it is wrong.

Cases: B = 2 maps of 6x70 (two 32-pixel units and a tail, even), 7x67 (odd last row and column) and 4x4 (one unit) with N = 64, and
7x67 with N = 32 (with ops.C4_POOL_RECOMPUTE_MIN_BYTES at 0: by default only maps beyond the caches take the path).  Channels:
ordinary ones, gamma = 0, gamma < 0, gamma = 1e-6 with beta = 1 and |beta| = 3 |gamma| (the last two and gamma = 0 take xhat from
raw: the raw_win route).  The input holds constant blocks, so that whole windows tie exactly, and the pooled
gradient has both signs."""
import ctypes
import functools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

CASES = [(2, 6, 70, 64), (2, 7, 67, 64), (2, 4, 4, 64), (2, 7, 67, 32)]
SENTINEL = -12345.0


def _input(B, H, W):
    g = torch.Generator().manual_seed(11 * H + W)
    x = torch.randn(B, H, W, 4, generator=g)
    if W > 40:
        x[:, :4, :6] = x[:, :1, :1]                        # constant blocks: the windows inside tie exactly, element for element
        x[:, -5:, 30:40] = x[:, -1:, 30:31]
        x[:, :, -5:] = 0.0                                 # ... and a block of zeros at the right edge (raw = bias there)
    return x.cuda()


def _params(N):
    g = torch.Generator().manual_seed(N)
    gamma = torch.empty(N).uniform_(0.5, 1.5, generator=g)
    beta = torch.randn(N, generator=g) * 0.2
    gamma[1] = 0.0
    gamma[2] = -0.8
    gamma[3], beta[3] = 1e-6, 1.0
    gamma[4], beta[4] = 0.5, 1.5
    gamma[9], beta[9] = -0.25, -0.75
    return gamma.cuda(), beta.cuda()


def _first_max(e):
    """index of the first maximum along dim 0 under a strict `>` (pool_cell_dpre)"""
    best = torch.zeros(e.shape[1:], dtype=torch.long, device=e.device)
    cur = e[0].clone()
    for k in range(1, e.shape[0]):
        m = e[k] > cur
        best[m] = k
        cur = torch.where(m, e[k], cur)
    return best


def _windows(t, Hp, Wp):
    """[B][H][W][N] -> [4][B][Hp][Wp][N]: the elements of every 2x2 window in scan order"""
    return torch.stack([t[:, 0:2 * Hp:2, 0:2 * Wp:2], t[:, 0:2 * Hp:2, 1:2 * Wp:2], t[:, 1:2 * Hp:2, 0:2 * Wp:2], t[:, 1:2 * Hp:2, 1:2 * Wp:2]])


@functools.lru_cache(maxsize=None)
def _case(B, H, W, N):
    """both paths on one case, kernel by kernel: computed once, shared by the checks below (which leave it unchanged)"""
    from efgh_amd import _C, ops
    from efgh_amd.nets import layers as L
    lib, ptr, by = _C.lib(), _C.ptr, ctypes.byref
    st = _C.stream_ptr()
    torch.manual_seed(5)
    dev = 'cuda'
    x = _input(B, H, W)
    Wp = (torch.randn(N, 9, 4) * 0.3).cuda()
    bias = (torch.randn(N) * 0.1).cuda()
    gamma, beta = _params(N)
    geom, M, Hp, Wq = L._same3x3_geom(B, H, W), B * H * W, H // 2, W // 2
    r = {}

    def finalize(stats):
        rm, rv = torch.zeros(N, device=dev), torch.ones(N, device=dev)
        return ops.bn_finalize(stats, stats.shape[0], N, float(M), gamma, beta, rm, rv, 0.1, 1e-5, save=True)
    # ---- the stored-raw path: conv with statistics, pooling pass, pooled reduction and apply from raw
    raw = torch.empty(B, H, W, N, device=dev)
    stats0 = torch.zeros(ops.stats_rows(1, 4, N, geom, M), 2, N, device=dev)
    ops.gather_gemm(x, 4, 4, 9, Wp, N, M, raw, N, mode=1, geom=geom, bias=bias, stats=stats0)
    scale, shift, mean, invstd = finalize(stats0)
    y0 = ops.maxpool2_affine(raw, scale, shift, ops.ACT_RELU)
    dy = torch.randn(B, Hp, Wq, N, device=dev)
    G = lib.efgh_bwd_groups(B * Hp * Wq)

    def sums(entry, third):
        s1, s2 = torch.empty(N, device=dev), torch.empty(N, device=dev)
        m1, m2 = torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.float64, device=dev)
        part = torch.empty(G, 2, N, dtype=torch.float64, device=dev)
        _C.check(entry(ptr(dy), ptr(y0), ptr(third), ptr(mean), ptr(invstd), ptr(scale), ptr(shift), B, H, W, N, ptr(part), ptr(s1),
                       ptr(s2), ptr(m1), ptr(m2), st))
        return s1, s2, m1, m2
    r['sums0'] = sums(lib.efgh_pool_bn_bwd_reduce_pooled, raw)
    m1, m2 = r['sums0'][2:]
    draw0 = torch.full((B, H, W, N), SENTINEL, device=dev)
    _C.check(lib.efgh_pool_bn_bwd_apply(ptr(dy), ptr(raw), ptr(mean), ptr(invstd), ptr(scale), ptr(m1), ptr(m2), ptr(scale), ptr(shift),
                                        B, H, W, N, ops.ACT_RELU, 0.0, ptr(draw0), st))
    # ---- the recompute path
    layer = ops.C4PoolLayer(x, 4, Wp, N, geom, M, bias)
    old, ops.C4_POOL_RECOMPUTE_MIN_BYTES = ops.C4_POOL_RECOMPUTE_MIN_BYTES, 0
    try:
        assert ops.c4_pool_recompute_ok(layer, 1, 4)
    finally:
        ops.C4_POOL_RECOMPUTE_MIN_BYTES = old
    stats1 = ops.c4_pool_stats(layer)
    y1 = torch.full((B, Hp, Wq, N), SENTINEL, device=dev)
    raw_win = torch.full((B, Hp, Wq, N), SENTINEL, device=dev)
    _C.check(lib.efgh_c4_conv3x3_pooled_train(by(layer.desc(out=y1, ldo=N, scale=scale, shift=shift, act=ops.ACT_RELU)), ptr(mean),
                                              ptr(invstd), ptr(raw_win), st))
    r['sums1'] = sums(lib.efgh_pool_bn_bwd_reduce_pooled_win, raw_win)
    draw1 = torch.full((B, H, W, N), SENTINEL, device=dev)
    _C.check(lib.efgh_c4_pool_bwd_draw(by(layer.desc(scale=scale, shift=shift, act=ops.ACT_RELU)), ptr(dy), ptr(mean), ptr(invstd),
                                       ptr(scale), ptr(m1), ptr(m2), ptr(draw1), st))
    torch.cuda.synchronize()
    r.update(raw=raw, stats0=stats0, stats1=stats1, y0=y0, y1=y1, raw_win=raw_win, draw0=draw0, draw1=draw1, scale=scale, shift=shift,
             mean=mean, invstd=invstd, Hp=Hp, Wq=Wq)
    return r


@pytest.mark.parametrize('case', CASES)
def test_statistics_rows_are_those_of_the_storing_launch(case):
    r = _case(*case)
    assert r['stats0'].shape == r['stats1'].shape
    assert torch.equal(r['stats0'], r['stats1'])


@pytest.mark.parametrize('case', CASES)
def test_pooled_output_is_conv_then_maxpool2_affine(case):
    r = _case(*case)
    assert torch.isfinite(r['y0']).all() and float(r['y0'].max()) > 0
    assert torch.equal(r['y0'], r['y1'])


@pytest.mark.parametrize('case', CASES)
def test_raw_win_is_raw_at_the_first_maximum_for_the_qualifying_channels_only(case):
    r = _case(*case)
    scale, shift, mean, invstd = (r[k] for k in ('scale', 'shift', 'mean', 'invstd'))
    beta = torch.addcmul(shift.double(), mean.double(), scale.double()).float()          # fmaf(mean, pscale, pshift)
    q = (scale == 0) | (beta.abs() * invstd.abs() > 2.0 * scale.abs())
    assert q[[1, 3, 4, 9]].all() and not q[[0, 2]].any() and 4 <= int(q.sum()) < q.numel() // 2
    w = _windows(r['raw'], r['Hp'], r['Wq'])
    # the activated value as the kernels form it: ONE rounding of raw*scale + shift (the float64 product is exact)
    e = torch.relu((w.double() * scale.double() + shift.double()).float())
    best = _first_max(e)
    ties = (e == e.max(0).values).sum(0) > 1
    assert ties[..., ~q].any() and (best > 0).any()
    want = torch.gather(w, 0, best[None])[0]
    got = r['raw_win']
    assert torch.equal(got[..., q], want[..., q])
    assert (got[..., ~q] == SENTINEL).all()


@pytest.mark.parametrize('case', CASES)
def test_sums_from_raw_win_equal_the_sums_from_raw(case):
    r = _case(*case)
    for a, b in zip(r['sums0'], r['sums1']):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert float(r['sums0'][0].abs().max()) > 0


@pytest.mark.parametrize('case', CASES)
def test_draw_from_the_recomputed_raw_equals_the_apply_pass(case):
    r = _case(*case)
    assert (r['draw0'] != SENTINEL).all()                  # every element is written, odd last row and column included
    assert torch.equal(r['draw0'], r['draw1'])


def _layer_run(conv, bn, x, gy, on, act=1, slope=0.0, stride=1, min_bytes=0):
    from efgh_amd import ops
    from efgh_amd.nets import layers as L
    old, ops.C4_POOL_RECOMPUTE = ops.C4_POOL_RECOMPUTE, on
    old_min, ops.C4_POOL_RECOMPUTE_MIN_BYTES = ops.C4_POOL_RECOMPUTE_MIN_BYTES, min_bytes      # (0: these small maps qualify)
    try:
        ops.TLS.train_step = True
        bn.running_mean.zero_(); bn.running_var.fill_(1.0)
        xg = x.clone().requires_grad_(True)
        y = L.conv2d(L.Ctx(True), xg, conv, bn, act, slope, pool=True)
        fn = y.grad_fn
        while not hasattr(fn, 'c4'):                       # (a view in front of the layer's own node)
            fn = fn.next_functions[0][0]
        saved = [tuple(t.shape) for t in fn.saved_tensors if t is not None]
        took = bool(fn.c4)
        y.backward(gy)
        torch.cuda.synchronize()
        params = [conv.weight, conv.bias, bn.weight, bn.bias]
        out = [y.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in params] + [bn.running_mean.clone(), bn.running_var.clone()]
        return out, saved, took
    finally:
        ops.TLS.train_step = False
        ops.C4_POOL_RECOMPUTE = old
        ops.C4_POOL_RECOMPUTE_MIN_BYTES = old_min
        for p in (conv.weight, conv.bias, bn.weight, bn.bias):
            p.grad = None


def _layer(N, stride=1):
    torch.manual_seed(N + stride)
    conv = nn.Conv2d(4, N, 3, stride, 1).cuda()
    bn = nn.BatchNorm2d(N).cuda()
    gamma, beta = _params(N)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    return conv, bn


@pytest.mark.parametrize('case', CASES)
def test_layer_is_bit_equal_with_the_switch_on_and_off_and_saves_no_full_resolution_tensor(case):
    B, H, W, N = case
    conv, bn = _layer(N)
    x = _input(B, H, W)
    gy = torch.randn(B, H // 2, W // 2, N, device='cuda')
    on, saved_on, took_on = _layer_run(conv, bn, x, gy, True)
    off, saved_off, took_off = _layer_run(conv, bn, x, gy, False)
    assert took_on and not took_off
    names = ('y', 'dx', 'dweight', 'dbias', 'dgamma', 'dbeta', 'running_mean', 'running_var')
    assert [n for n, a, b in zip(names, on, off) if not torch.equal(a, b)] == []
    assert float(on[2].abs().max()) > 0 and float(on[1].abs().max()) > 0
    full = B * H * W * N

    def numel(s):
        n = 1
        for d in s:
            n *= d
        return n
    assert [s for s in saved_on if numel(s) == full] == []
    assert [s for s in saved_off if numel(s) == full] == [(B, H, W, N)]          # (the stored-raw path does keep it: the check can fail)


def test_stride_2_and_leaky_relu_layers_keep_the_stored_raw_path():
    B, H, W, N = 2, 8, 70, 64
    x = _input(B, H, W)
    conv, bn = _layer(N)
    _, saved, took = _layer_run(conv, bn, x, torch.randn(B, H // 2, W // 2, N, device='cuda'), True, act=2, slope=0.2)
    assert not took and (B, H, W, N) in saved
    conv2, bn2 = _layer(N, stride=2)
    _, saved, took = _layer_run(conv2, bn2, x, torch.randn(B, H // 4, W // 4, N, device='cuda'), True)
    assert not took and (B, H // 2, W // 2, N) in saved


def test_size_bound_keeps_cache_resident_maps_on_the_stored_raw_path_and_takes_the_trunks_first_layers():
    from efgh_amd import ops
    B, H, W, N = 2, 6, 70, 64
    conv, bn = _layer(N)
    gy = torch.randn(B, H // 2, W // 2, N, device='cuda')
    _, saved, took = _layer_run(conv, bn, _input(B, H, W), gy, True, min_bytes=ops.C4_POOL_RECOMPUTE_MIN_BYTES)
    assert not took and (B, H, W, N) in saved
    _, saved, took = _layer_run(conv, bn, _input(B, H, W), gy, True, min_bytes=4 * B * H * W * N)          # exactly at the bound
    assert took and (B, H, W, N) not in saved
    # the layers the path was built for, at the training batch: F's range trunk and the two camera trunks
    assert ops.C4_POOL_RECOMPUTE and 0 < ops.C4_POOL_RECOMPUTE_MIN_BYTES <= 4 * 8 * 384 * 1280 * 64 < 4 * 8 * 384 * 5120 * 64
