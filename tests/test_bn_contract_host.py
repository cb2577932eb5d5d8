"""The float64 reference of tests/bn_contract.py, checked on the CPU before it meets a kernel: (1) the reference functions chained into
conv output -> training BatchNorm -> activation (-> residual) (-> MaxPool2d(2,2)) against torch float64 autograd, forward and every
gradient to 1e-12; (2) the pooled-from-y formulation of the pooled BatchNorm-backward sums against the from-raw one; (3) the input
generator: after its moves no case of the GPU module has an element or a window that fp32 and float64 could decide differently."""
import pytest
import torch
import torch.nn.functional as F

import bn_contract as BC

REL = 1e-12
SHAPES = [(2, 4, 6, 8), (1, 5, 7, 4), (3, 2, 2, 36), (1, 3, 2, 12)]
ACTS3 = [(BC.ACT_NONE, 0.0), (BC.ACT_RELU, 0.0), (BC.ACT_LEAKY, 0.2)]


def _close(got, want, what):
    err = float((got - want).abs().max())
    assert err <= REL * (float(want.abs().max()) + 1e-300), (what, err)


def _torch_act(v, a, slope):
    return v if a == BC.ACT_NONE else (F.relu(v) if a == BC.ACT_RELU else F.leaky_relu(v, BC.f32(slope)))      # (the slope a kernel gets is a float argument)


def _inputs(shape, seed):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * (0.5 + torch.rand(C, generator=g, dtype=torch.float64))
         + torch.randn(C, generator=g, dtype=torch.float64))
    gamma = 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    gamma[C // 2] = -gamma[C // 2]
    beta = 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    return x, gamma, beta, g


def _forward_ref(x2, gamma, beta, res, a, slope):
    M = x2.shape[0]
    st, _ = BC.col_stats(x2)
    assert st.shape[0] == BC.col_stats_groups(M)
    fin = {k: v[0] for k, v in BC.bn_finalize(st, float(M), gamma, beta, None, None, 0.1, BC.EPS).items()}
    y, _, pre = BC.scale_shift_act(x2, fin['scale'], fin['shift'], res, a, slope)
    return fin, y, pre


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('a,slope', ACTS3)
@pytest.mark.parametrize('with_res', [False, True])
def test_reference_chain_equals_float64_autograd(shape, a, slope, with_res):
    B, H, W, C = shape
    M = B * H * W
    x, gamma, beta, g = _inputs(shape, 11 + C + a)
    x2 = x.view(M, C)
    res = torch.randn((M, C), generator=g, dtype=torch.float64) if with_res else None
    wgt = torch.randn((M, C), generator=g, dtype=torch.float64)
    fin, y, pre = _forward_ref(x2, gamma, beta, res, a, slope)
    # the three mask sources agree (the recompute only where there is no residual)
    pos = BC.mask_of(y=y)
    if a != BC.ACT_NONE:
        assert torch.equal(pos, pre > 0)
    if (M * C) % 32 == 0:
        assert torch.equal(BC.unpack_bits(BC.pack_bits(pre > 0), M, C), pre > 0)
    if not with_res:
        assert torch.equal(BC.mask_of(raw=x2, pscale=fin['scale'], pshift=fin['shift']), pre > 0)
    pos = pre > 0
    s, _ = BC.act_bn_bwd_reduce(wgt, pos, x2, fin['mean'], fin['invstd'], a, slope)
    draw, _, dres, _ = BC.act_bn_bwd_apply(wgt, pos, x2, fin['mean'], fin['invstd'], gamma * fin['invstd'], s[0] / M, s[1] / M, a, slope)

    xt, gt, bt = x2.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    rt = res.clone().requires_grad_() if with_res else None
    v = F.batch_norm(xt, None, None, gt, bt, True, 0.1, BC.f32(BC.EPS))
    yt = _torch_act(v + rt if with_res else v, a, slope)
    (yt * wgt).sum().backward()
    _close(y, yt.detach(), 'forward')
    _close(draw, xt.grad, 'draw')
    _close(s[1], gt.grad, 'dgamma')
    _close(s[0], bt.grad, 'dbeta')
    if with_res:
        _close(dres, rt.grad, 'dres')
    # the forms without statistics: the bias gradient and coef * dpre
    s0, _ = BC.act_bn_bwd_reduce(wgt, pos, None, None, None, a, slope)
    _close(s0[0], s[0], 'sum dpre without mean')
    d0 = BC.act_bn_bwd_apply(wgt, pos, None, None, None, gamma, None, None, a, slope)[0]
    _close(d0, gamma * dres, 'coef * dpre')


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('a,slope', ACTS3)
def test_pooled_reference_chain_equals_float64_autograd(shape, a, slope):
    B, H, W, C = shape
    M = B * H * W
    x, gamma, beta, g = _inputs(shape, 23 + C + a)
    x2 = x.view(M, C)
    wp = torch.randn((B, H // 2, W // 2, C), generator=g, dtype=torch.float64)
    fin, y, pre = _forward_ref(x2, gamma, beta, None, a, slope)
    sc, sh, mu, inv = fin['scale'], fin['shift'], fin['mean'], fin['invstd']
    yp, _ = BC.maxpool2_affine(x, sc, sh, a, slope)
    assert torch.equal(yp, BC.maxpool2(y.view(B, H, W, C)))
    v2 = BC.maxpool_v2(y.view(B, H, W, C))
    assert torch.equal(torch.maximum(v2[:, :, 0:2 * (W // 2):2], v2[:, :, 1:2 * (W // 2):2]), yp)
    s, _ = BC.pool_bn_bwd_reduce(wp, x, mu, inv, sc, sh, a, slope)
    draw, _ = BC.pool_bn_bwd_apply(wp, x, mu, inv, gamma * inv, s[0] / M, s[1] / M, sc, sh, a, slope)
    # the unfused route: pool backward, then the BatchNorm backward of the full-resolution gradient
    dyf = torch.zeros((B, H, W, C), dtype=torch.float64)
    dyf[:, :2 * (H // 2), :2 * (W // 2)] = BC.maxpool2_bwd(y.view(B, H, W, C), wp)
    assert torch.equal(dyf[:, :2 * (H // 2), :2 * (W // 2)], BC.maxpool2_bwd_affine(x, sc, sh, a, slope, wp))
    s_u, _ = BC.act_bn_bwd_reduce(dyf.view(M, C), pre > 0, x2, mu, inv, a, slope)
    _close(s_u, s, 'fused against unfused sums')

    xt, gt, bt = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    v = F.batch_norm(xt.view(M, C), None, None, gt, bt, True, 0.1, BC.f32(BC.EPS)).view(B, H, W, C)
    yt = F.max_pool2d(_torch_act(v, a, slope).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    (yt * wp).sum().backward()
    _close(yp, yt.detach(), 'pooled forward')
    _close(draw, xt.grad, 'draw')
    _close(s[1], gt.grad, 'dgamma')
    _close(s[0], bt.grad, 'dbeta')


@pytest.mark.parametrize('shape', SHAPES)
def test_pooled_from_y_equals_from_raw_in_float64(shape):
    B, H, W, C = shape
    M = B * H * W
    x, gamma, beta, g = _inputs(shape, 37 + C)
    gamma[0] = 0.0                                  # (a constant channel: xhat from raw at the window's first element)
    wp = torch.randn((B, H // 2, W // 2, C), generator=g, dtype=torch.float64)
    fin, _, _ = _forward_ref(x.view(M, C), gamma, beta, None, BC.ACT_RELU, 0.0)
    sc, sh, mu, inv = fin['scale'], fin['shift'], fin['mean'], fin['invstd']
    yp, _ = BC.maxpool2_affine(x, sc, sh, BC.ACT_RELU, 0.0)
    s, bnd = BC.pool_bn_bwd_reduce(wp, x, mu, inv, sc, sh, BC.ACT_RELU, 0.0)
    for fr in (None, torch.arange(C) % 2 == 1, torch.ones(C, dtype=torch.bool)):
        sy, _ = BC.pool_bn_bwd_reduce_pooled(wp, yp, x, mu, inv, sc, sh, from_raw=fr)
        assert float(((sy - s).abs() / (bnd + 1e-300)).max()) <= 1e-11


def test_reference_semantics_at_the_edges():
    e = torch.tensor([[1.0, 2.0, 2.0, 0.0], [3.0, 0.0, 1.0, 3.0], [0.0, 0.0, 0.0, 0.0], [-1.0, float('nan'), 5.0, 5.0]]).t().double()
    best, val = BC.first_max(e.contiguous())
    assert best.tolist() == [1, 0, 0, 2] and val.tolist() == [2.0, 3.0, 0.0, 5.0]
    nan = torch.tensor([[float('nan'), -1.0, 2.0, 0.0]])
    for a, s in BC.ACTS:
        y, _, _ = BC.scale_shift_act(nan, None, None, None, a, s)
        assert torch.isnan(y[0, 0]) and not bool((y[0] > 0)[0])
    assert BC.scale_shift_act(nan, None, None, None, BC.ACT_LEAKY, 0.2)[0][0, 1:].tolist() == [-1.0 * BC.f32(0.2), 2.0, 0.0]
    pos = torch.zeros(2, 32, dtype=torch.bool)
    pos[0, 0] = pos[0, 31] = pos[1, 5] = True
    assert BC.pack_bits(pos).tolist() == [1 - 2 ** 31, 32]
    x = torch.arange(513 * 4, dtype=torch.float32).view(513, 4)
    st, mag = BC.col_stats(x)
    assert st.shape == (2, 2, 4) and st[1, 0].tolist() == x[512].tolist() and float(st[0, 0, 0]) == float(x[:512, 0].sum())
    one = BC.bn_finalize(torch.tensor([[[2.0], [5.0]]]), 1.0, torch.ones(1), torch.zeros(1), torch.zeros(1), torch.ones(1), 0.5, 0.0)
    assert float(one['rvar'][0]) == 0.5 + 0.5 * 1.0            # count == 1: the biased variance (5 - 4) goes into the running update
    two = BC.bn_finalize(torch.tensor([[[2.0], [4.0]]]), 2.0, torch.ones(1), torch.zeros(1), torch.zeros(1), torch.ones(1), 0.5, 0.0)
    assert float(two['rvar'][0]) == 0.5 + 0.5 * 2.0            # var 1, unbiased 2


def test_unsettled_inputs_do_have_ambiguous_elements():
    """the generator's check is not vacuous: the same draw without the moves has elements near 0 and near-ties"""
    p = BC.bn_params(64, 5, 'cpu')
    raw = torch.randn(3, 8, 6, 64) * p['std'] + p['mean']
    near0, tie = BC.ambiguous(raw, p['scale'], p['shift'], None, BC.ACT_RELU, 0.0, True)
    assert int(near0.sum()) > 0 and int(tie.sum()) > 0
    assert BC.settle(raw, p['scale'], p['shift'], None, BC.ACT_RELU, 0.0, True) == 0


@pytest.mark.parametrize('kind,shape,a,slope', BC.host_cases(), ids=lambda v: str(v).replace(' ', ''))
def test_generated_case_has_an_empty_ambiguous_set(kind, shape, a, slope):
    c = BC.gen_case(kind, shape, a, slope, 'cpu')
    assert c['ambiguous'] == 0
    assert bool(torch.isfinite(c['raw']).all())
    if tuple(shape) == BC.POOL_TIES and kind == 'pool':
        p = c['p']
        _, _, e, _ = BC._affine_windows(c['raw'][0:1], p['scale'], p['shift'], a, slope)
        e = e[:, 0, 0, :, :][:, :, p['scale'] != 0]                  # [4][window j][channel]
        assert bool((e[:, 0] == e[0:1, 0]).all())                     # four equal values
        assert bool((e[1, 1] == e[2, 1]).all()) and BC.first_max(e)[0][1].unique().tolist() == [1]
        assert bool((e[0, 2] == e[3, 2]).all()) and BC.first_max(e)[0][2].unique().tolist() == [0]
        if a == BC.ACT_RELU:
            assert bool((e[:, 3] == 0).all()) and BC.first_max(e)[0][3].unique().tolist() == [0]
        if a == BC.ACT_LEAKY and slope > 0:
            assert bool((e[1, 3] == e[2, 3]).all()) and bool((e[1, 3] < 0).all()) and BC.first_max(e)[0][3].unique().tolist() == [1]
