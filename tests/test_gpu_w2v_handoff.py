"""The input transform V = B^T x B of a 2-D Winograd layer goes from the layer's forward to its weight gradient on the layer's own
autograd node (GemmLayerFn: ctx.kept_v, ops.gather_gemm keep_v= -> ops.gather_wgrad pre_v=): held to the run that transforms again
(ops.W2V_KEEP off - the same kernels on the same bytes, so every gradient is torch.equal), counted by wrapping ops.wino2d_input.

Shapes: C = N = 128 (the default WINO2D_MIN_C*), B = 2 on a 9 x 13 map - both sides at least 8 and no multiple of 4, so the edge
tiles are there."""
import gc

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C, B, H, W = 128, 2, 9, 13


def _layer(seed):
    torch.manual_seed(seed)
    conv, bn = nn.Conv2d(C, C, 3, 1, 1, bias=False), nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.2)
    return conv.cuda(), bn.cuda()


def _inputs():
    torch.manual_seed(1)
    return torch.randn(B, H, W, C).cuda(), torch.randn(B, H, W, C).cuda()


@pytest.fixture
def counted(monkeypatch):
    """[number of ops.wino2d_input calls], with TLS.train_step on for the test"""
    from efgh_amd import ops
    n, orig = [0], ops.wino2d_input

    def wrapped(*a, **k):
        n[0] += 1
        return orig(*a, **k)
    monkeypatch.setattr(ops, 'wino2d_input', wrapped)
    monkeypatch.setattr(ops.TLS, 'train_step', True)
    return n


def _grads(x, mods):
    torch.cuda.synchronize()
    out = [x.grad.clone()] + [p.grad.clone() for m in mods for p in m.parameters()]
    x.grad = None
    for m in mods:
        for p in m.parameters():
            p.grad = None
    return out


def _run(build, keep, counted, monkeypatch):
    """build(x) -> (outputs, modules) on fresh seeded layers; -> (gradients of x and of every parameter, transforms, LAZY_HITS[0])"""
    from efgh_amd import ops
    monkeypatch.setattr(ops, 'W2V_KEEP', keep)
    x0, gy = _inputs()
    x = x0.requires_grad_(True)
    n0, h0 = counted[0], ops.LAZY_HITS[0]
    ys, mods = build(x)
    torch.autograd.backward(ys, [gy] * len(ys))
    return _grads(x, mods), counted[0] - n0, ops.LAZY_HITS[0] - h0


def _same(a, b):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i


def _one(x):
    from efgh_amd.nets import layers as L
    conv, bn = _layer(2)
    return [L.conv2d(L.Ctx(True), x, conv, bn, L.ACT_RELU)], [conv, bn]


def test_one_layer_transforms_once(counted, monkeypatch):
    on, n_on, _ = _run(_one, True, counted, monkeypatch)
    off, n_off, _ = _run(_one, False, counted, monkeypatch)
    assert (n_on, n_off) == (1, 2)
    assert len(on) == 4                      # dx, dW, dgamma, dbeta
    _same(on, off)


def test_deferred_activation_is_applied_once(counted, monkeypatch):
    from efgh_amd.nets import layers as L

    def build(x):
        (c1, b1), (c2, b2) = _layer(2), _layer(3)
        ctx = L.Ctx(True)
        defer = L.lazy_consumer_ok(ctx, c2, B, H, W)
        assert defer
        y1 = L.conv2d(ctx, x, c1, b1, L.ACT_RELU, defer_act=defer)
        assert getattr(y1, '_efgh_lazy', None) is not None
        return [L.conv2d(ctx, y1, c2, b2, L.ACT_RELU)], [c1, b1, c2, b2]
    on, _, lazy_on = _run(build, True, counted, monkeypatch)
    off, _, lazy_off = _run(build, False, counted, monkeypatch)
    assert (lazy_on, lazy_off) == (1, 2)
    _same(on, off)


def test_two_layers_on_one_input_each_keep_their_own(counted, monkeypatch):
    from efgh_amd.nets import layers as L

    def build(x):
        (c1, b1), (c2, b2) = _layer(2), _layer(3)
        ctx = L.Ctx(True)
        return [L.conv2d(ctx, x, c1, b1, L.ACT_RELU), L.conv2d(ctx, x, c2, b2, L.ACT_RELU)], [c1, b1, c2, b2]
    on, n_on, _ = _run(build, True, counted, monkeypatch)
    off, n_off, _ = _run(build, False, counted, monkeypatch)
    assert (n_on, n_off) == (2, 4)
    _same(on, off)


def test_dropped_forward_frees_its_transform(counted):
    """the node owns V: a train-mode forward whose outputs are dropped without a backward, and without any clear call, leaves nothing"""
    from efgh_amd.nets import layers as L
    conv, bn = _layer(2)
    x0, gy = _inputs()
    x = x0.requires_grad_(True)
    y = L.conv2d(L.Ctx(True), x, conv, bn, L.ACT_RELU)       # warm-up: packed weights, scratch and the .grad tensors exist afterwards
    y.backward(gy)
    del y
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    y = L.conv2d(L.Ctx(True), x, conv, bn, L.ACT_RELU)
    assert y.grad_fn.kept_v[0] is not None and torch.cuda.memory_allocated() > base
    del y
    gc.collect()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base


def test_second_backward_over_a_retained_graph_transforms_again(counted):
    from efgh_amd.nets import layers as L
    conv, bn = _layer(2)
    x0, gy = _inputs()
    x = x0.requires_grad_(True)
    y = L.conv2d(L.Ctx(True), x, conv, bn, L.ACT_RELU)
    assert counted[0] == 1
    y.backward(gy, retain_graph=True)
    assert counted[0] == 1 and y.grad_fn.kept_v is None
    first = _grads(x, [conv, bn])
    y.backward(gy, retain_graph=True)
    assert counted[0] == 2
    _same(_grads(x, [conv, bn]), first)


def test_route_flipped_between_forward_and_backward_drops_the_transform(counted, monkeypatch):
    """ops.WINO2D_MIN_C_WGRAD raised behind the forward: the weight gradient runs on the 1-D Winograd kernel, which has no use for V.
    Against torch in float64, at the bound tests/test_gpu_backward.py::test_conv_bn_act_backward holds its 128-channel 3x3 layers to
    (on maps the 2-D path does not take their weight gradient goes the same way): 2e-4 on the Frobenius norm, 1e-5 on the output,
    no gradient fed within 1e-4 of the activation's kink"""
    from efgh_amd import ops
    from efgh_amd.nets import layers as L
    conv, bn = _layer(2)
    x0, gy = _inputs()
    xr = x0.detach().cpu().double().permute(0, 3, 1, 2).requires_grad_(True)
    cr, br = nn.Conv2d(C, C, 3, 1, 1, bias=False).double(), nn.BatchNorm2d(C).double()
    cr.load_state_dict({k: v.cpu().double() for k, v in conv.state_dict().items()})
    br.load_state_dict({k: v.cpu().double() for k, v in bn.state_dict().items()})
    pre = br(cr(xr))
    yr = F.relu(pre)
    gy = gy * (pre.detach().abs() > 1e-4).permute(0, 2, 3, 1).to(gy.dtype).cuda()
    yr.backward(gy.cpu().double().permute(0, 3, 1, 2))

    x = x0.requires_grad_(True)
    geom = L._same3x3_geom(B, H, W)
    assert ops.wgrad_route(1, C, C, 9, geom) == 'wino2d'
    y = L.conv2d(L.Ctx(True), x, conv, bn, L.ACT_RELU)
    assert y.grad_fn.kept_v[0] is not None
    monkeypatch.setattr(ops, 'WINO2D_MIN_C_WGRAD', 1024)
    assert ops.wgrad_route(1, C, C, 9, geom) == 'wino'
    n0 = counted[0]
    y.backward(gy)
    torch.cuda.synchronize()
    assert y.grad_fn.kept_v is None
    assert counted[0] - n0 <= 1              # (the data gradient's own transform of draw; x is not transformed again)

    def relerr(a, b):
        return float((a.double().cpu() - b).norm() / (b.norm() + 1e-20))
    assert relerr(y.detach().permute(0, 3, 1, 2), yr.detach()) < 1e-5
    assert relerr(x.grad.permute(0, 3, 1, 2), xr.grad) < 2e-4
    assert relerr(conv.weight.grad, cr.weight.grad) < 2e-4
    assert relerr(bn.weight.grad, br.weight.grad) < 2e-4
    assert relerr(bn.bias.grad, br.bias.grad) < 2e-4
