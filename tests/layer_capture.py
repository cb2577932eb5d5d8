"""What the layer executors of efgh_amd/nets/layers.py hand to the library, recorded without a GPU: the public layer functions run on
CPU tensors under route_capture.Capture (every efgh_* launch is recorded and does nothing; the query functions go to the real
libefgh_hip.so) with _C.require_cuda replaced too.  tests/test_layers_host.py compares the table this produces with
tests/golden/layers.json.

Per case and (train, grad) context the table holds: the entry points of the forward and of backward() in order; every argument handed
to the library (route_capture's digests: descriptor fields verbatim, pointers as (named tensor, byte offset) with the layer's input,
parameters, residual, `out` buffer, returned tensors and the gradients fed to backward named, 'tmp' for what the layer allocated
itself); shape, strides and storage relation of what the layer returns and whether it carries _efgh_lazy / _efgh_bnsrc; which
gradients come back as None; the num_batches_tracked counters.  A case that raises is recorded by its exception type alone.

Every tensor torch makes during a case is kept alive until the case has been digested (_Keep), so that no address is used twice and a
pointer names one tensor whatever the allocator does."""
import json
import os
import sys
import types

import torch
import torch.nn as nn
from torch.utils._python_dispatch import TorchDispatchMode

import route_capture as RC

OFF_IN_TURN = ('LAZY_ACT', 'W2_BWD_FUSED', 'W2_BWD_FUSED_POOL', 'BN_MASK_BITS', 'USE_WINO2D', 'USE_THIN')
SETTINGS = [('default', {})] + [(k + ' off', {k: False}) for k in OFF_IN_TURN]
CONTEXTS = ((False, False), (True, False), (False, True), (True, True))          # (train, grad)
RAISES = ('blur r2 weight of radius 1',)          # the deliberate rejections: the only cases that may raise


class _Keep(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.held = []

    def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
        r = func(*args, **(kwargs or {}))
        self.held.append(r)
        return r


class LayerCapture(RC.Capture):
    def _ptr(self, p):                # resolved once the case has returned (the returned tensors are named too)
        return ['@', p] if p else None

    def __enter__(self):
        super().__enter__()
        ops, _C = self.ops, self._C
        self.saved += [(_C, 'require_cuda', _C.require_cuda)] + [(ops, k, getattr(ops, k)) for k in OFF_IN_TURN + ('BLUR_DGRAD_FUSED',)
                                                                    if not any(s[1] == k for s in self.saved)]
        _C.require_cuda = lambda *t: None
        return self

    def _resolve(self, x, named):
        if isinstance(x, dict):
            return {k: self._resolve(v, named) for k, v in x.items()}
        if isinstance(x, list):
            if len(x) == 2 and x[0] == '@':
                for name, t in named:
                    s = t.untyped_storage()
                    if s.data_ptr() <= x[1] < s.data_ptr() + max(s.nbytes(), 1):
                        return [name, x[1] - t.data_ptr()]
                return 'tmp'
            return [self._resolve(v, named) for v in x]
        return x

    def take(self):
        calls, dig = '+'.join(self.calls), list(self.digest)
        del self.calls[:], self.digest[:]
        return calls, dig

    def case(self, build, train, grad):
        """-> [forward entry points | exception type, backward entry points, digest]"""
        from efgh_amd.nets import layers as L
        ops = self.ops
        ops.TLS.train_step, ops.BLUR_DGRAD_FUSED = bool(train and grad), True
        self.take()
        with torch.set_grad_enabled(grad), _Keep() as keep:
            named, bns, run = build(grad)
            named = [(k, v) for k, v in named.items() if torch.is_tensor(v)]
            try:
                ret = run(L.Ctx(train))
            except Exception as e:
                return [type(e).__name__, '', '']
            fcalls, fdig = self.take()
            rets = [r for r in (ret if isinstance(ret, tuple) else (ret,))]
            shapes = []
            for i, r in enumerate(rets):
                rel = 'own'
                for name, t in named:
                    if t.untyped_storage().data_ptr() == r.untyped_storage().data_ptr():
                        rel = [name, r.data_ptr() - t.data_ptr()]
                        break
                shapes.append([list(r.shape), list(r.stride()), rel, hasattr(r, '_efgh_lazy'), hasattr(r, '_efgh_bnsrc'), r.requires_grad])
                named.append(('ret%d' % i, r))
            bcalls, bdig, grads = '', [], []
            back = [r for r in rets if r.requires_grad and r.grad_fn is not None]
            if back:
                dys = [torch.zeros(r.shape) for r in back]
                named += [('dy%d' % i, d) for i, d in enumerate(dys)]
                torch.autograd.backward(back, dys)
                bcalls, bdig = self.take()
                grads = [[name, t.grad is None] for name, t in named if t.is_leaf and t.requires_grad]
            nbt = [int(b.num_batches_tracked) for b in bns]
            digest = RC._h([self._resolve(fdig, named), self._resolve(bdig, named), shapes, grads, nbt])
            del keep.held[:]
        return [fcalls, bcalls, digest]


# ---- the case list ------------------------------------------------------------------------------------------------------------------
def ceil4(n):
    return (n + 3) // 4 * 4


def T(*shape, grad=False):
    t = torch.zeros(shape)
    return t.requires_grad_() if grad else t


def P(named, prefix, *mods):
    """name the parameters and the float buffers of the modules"""
    for i, m in enumerate(mods):
        if m is None:
            continue
        for k, v in list(m.named_parameters()) + [(k, b) for k, b in m.named_buffers() if b.dtype == torch.float32]:
            named['%s%d.%s' % (prefix, i, k)] = v
    return named


def bns_of(*mods):
    return [b for m in mods if m is not None for b in m.modules() if isinstance(b, (nn.BatchNorm1d, nn.BatchNorm2d))]


def conv_case(ci, co, k, s, H, W, B=2, bias=False, bn=True, res=False, act=1, slope=0.0, xgrad=True, out=False, in_ch=False,
              skip_out=False, pool=False, consumer=None):
    def build(grad):
        L = _layers()
        m = nn.Conv2d(ci, co, k, s, k // 2, bias=bias)
        b = nn.BatchNorm2d(co) if bn else None
        Cp = ceil4(ci)
        x = T(B, H, W, 2 * Cp if in_ch else Cp, grad=grad and xgrad)
        Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
        r = T(B, Ho, Wo, ceil4(co), grad=grad) if res else None
        buf = T(B, Ho, Wo, 2 * co) if out else None
        nxt = nn.Conv2d(co, consumer, 3, 1, 1, bias=False) if consumer else None
        nbn = nn.BatchNorm2d(consumer) if consumer else None
        named = P({'x': x, 'res': r, 'out': buf}, 'm', m, b, nxt, nbn)

        def run(ctx):
            kw = {}
            if nxt is not None:           # the producer defers its activation to a consumer that can apply it (as run_vgg does)
                kw['defer_act'] = L.lazy_consumer_ok(ctx, nxt, B, Ho, Wo)
            y = L.conv2d(ctx, x, m, b, act, slope, residual=r, out=(buf, co) if out else None, in_ch=(Cp, Cp) if in_ch else None,
                         skip_out=skip_out, pool=bool(pool and ctx.grad), **kw)
            if nxt is None:
                return y
            return L.conv2d(ctx, y, nxt, nbn, act, slope)
        return named, bns_of(m, b, nbn), run
    return build


def convt_case(ci, co, H, W, op=1, B=2, bias=False, bn=True, skip_out=False, defer=False, out=False):
    def build(grad):
        L = _layers()
        m = nn.ConvTranspose2d(ci, co, 3, 2, 1, output_padding=op, bias=bias)
        b = nn.BatchNorm2d(co) if bn else None
        nxt = nn.Conv2d(co, co, 3, 1, 1, bias=False) if defer else None
        x = T(B, H, W, ci, grad=grad)
        Ho, Wo = (H - 1) * 2 - 2 + 3 + op, (W - 1) * 2 - 2 + 3 + op
        buf = T(B, Ho, Wo, 2 * co) if out else None
        named = P({'x': x, 'out': buf}, 'm', m, b)

        def run(ctx):
            return L.conv_transpose2d(ctx, x, m, b, 2, 0.2, out=(buf, co) if (out and not ctx.grad) else None, skip_out=skip_out,
                                      defer_for=nxt if ctx.grad else None)
        return named, bns_of(b), run
    return build


def linear_case(M, C, O, bias=True, bn=False, count=None, slice_=False, out=False, act=1):
    def build(grad):
        L = _layers()
        m = nn.Linear(C, O, bias=bias)
        b = nn.BatchNorm1d(O) if bn else None
        Cp = ceil4(C)
        x = T(M, 2 * Cp if slice_ else Cp, grad=grad)
        buf = T(M, 2 * ceil4(O)) if out else None
        named = P({'x': x, 'out': buf}, 'm', m, b)

        def run(ctx):
            kw = dict(lda=2 * Cp, a_off=Cp) if slice_ else {}
            return L.linear_rows(ctx, x, M, C, m.weight, m.bias, b, act, 0.0, out=(buf, ceil4(O)) if (out and not ctx.grad) else None,
                                 count=count, **kw)
        return named, bns_of(b), run
    return build


def blur_case(H, C, C0, C1, level=None, F=15, fused=True, out=False):
    """level: None (a bare table), 1 or 2 (a lattice level object of that radius; its weight has F taps)"""
    def build(grad):
        L = _layers()
        ops = sys.modules['efgh_amd.ops']
        c0, c1 = nn.Conv2d(C, C0, (F, 1)), nn.Conv2d(C0, C1, 1)
        splat = T(H, C, grad=grad)
        buf = T(H, 2 * C1) if out else None
        i32 = torch.int32
        if level is None:
            table = torch.zeros(H, 16, dtype=i32)
            named = {'x': splat, 'out': buf, 'table': table}
        else:
            Fl = 15 if level == 1 else 65
            table = types.SimpleNamespace(nbr=torch.zeros(H, Fl + (Fl + 31) // 32 if level != 1 else 16, dtype=i32), radius=level, F=Fl,
                                          H=H, alist=torch.zeros(64, dtype=i32), info=torch.zeros(16, dtype=i32), n_alias=1)
            named = {'x': splat, 'out': buf, 'table': table.nbr, 'alist': table.alist, 'info': table.info}
        P(named, 'm', c0, c1)

        def run(ctx):
            ops.BLUR_DGRAD_FUSED = fused          # (read in backward: LayerCapture.case puts it back before the next case)
            return L.blur_conv(ctx, splat, H, C, table, c0, c1, out=(buf, C1) if (out and not ctx.grad) else None, last_act=1)
        return named, [], run
    return build


def _vgg(cfg, ci=3):
    mods = []
    for v in cfg:
        if v == 'M':
            mods.append(nn.MaxPool2d(2, 2))
        else:
            mods += [nn.Conv2d(ci, v, 3, padding=1), nn.BatchNorm2d(v), nn.ReLU()]
            ci = v
    return nn.Sequential(*mods)


def vgg_case(cfg, H, W, B=1):
    def build(grad):
        L = _layers()
        f = _vgg(cfg)
        x = T(B, H, W, 4)
        return P({'x': x}, 'f', f), bns_of(f), lambda ctx: L.run_vgg(ctx, f, x)
    return build


def _block(ci, co, stride):
    blk = nn.Module()
    blk.conv1, blk.bn1 = nn.Conv2d(ci, co, 3, stride, 1, bias=False), nn.BatchNorm2d(co)
    blk.conv2, blk.bn2 = nn.Conv2d(co, co, 3, 1, 1, bias=False), nn.BatchNorm2d(co)
    blk.downsample = None
    if stride != 1 or ci != co:
        blk.downsample = nn.Sequential(nn.Conv2d(ci, co, 1, stride, bias=False), nn.BatchNorm2d(co))
    return blk


def block_case(ci, co, stride, H, W, B=2, alias_in=False, out=False, layer=False):
    def build(grad):
        L = _layers()
        blk = nn.Sequential(_block(ci, co, stride), _block(co, co, 1)) if layer else _block(ci, co, stride)
        x = T(B, H, W, ci, grad=grad)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        buf = T(B, Ho, Wo, 2 * co) if out else None
        fn = L.run_resnet_layer if layer else L.run_basic_block
        return (P({'x': x, 'out': buf}, 'b', blk), bns_of(blk),
                lambda ctx: fn(ctx, blk, x, out=(buf, co) if out else None, alias_in=alias_in))
    return build


def _convt_seq(ci, co, op=1):
    return nn.Sequential(nn.ConvTranspose2d(ci, co, 3, 2, 1, output_padding=op, bias=False), nn.BatchNorm2d(co), nn.LeakyReLU(0.2),
                         nn.Conv2d(co, co, 3, 1, 1, bias=False), nn.BatchNorm2d(co), nn.LeakyReLU(0.2))


def convt_bn_relu_case(ci, co, H, W, B=2, skip_out=False, out=False):
    def build(grad):
        L = _layers()
        seq = _convt_seq(ci, co)
        x = T(B, H, W, ci, grad=grad)
        buf = T(B, 2 * H, 2 * W, 2 * co) if out else None
        return (P({'x': x, 'out': buf}, 's', seq), bns_of(seq),
                lambda ctx: L.run_convt_bn_relu(ctx, seq, x, out=(buf, co) if out else None, skip_out=skip_out))
    return build


def conv_bn_relu_case(ci, co, H, W, B=2, skip_out=False, out=False, in_ch=False):
    def build(grad):
        L = _layers()
        seq = nn.Sequential(nn.Conv2d(ci, co, 3, 1, 1, bias=False), nn.BatchNorm2d(co), nn.LeakyReLU(0.2))
        x = T(B, H, W, 2 * ci if in_ch else ci, grad=grad)
        buf = T(B, H, W, 2 * co) if out else None
        return (P({'x': x, 'out': buf}, 's', seq), bns_of(seq),
                lambda ctx: L.run_conv_bn_relu(ctx, seq, x, out=(buf, co) if out else None, in_ch=(ci, ci) if in_ch else None,
                                               skip_out=skip_out))
    return build


def heads_case(ci, H, W, B=1):
    def build(grad):
        L = _layers()
        sd, sm = _convt_seq(ci, 1), _convt_seq(ci, 2)
        x = T(B, H, W, ci, grad=grad)

        def run(ctx):
            assert L.convt_heads_fusable(sd, sm)
            return L.run_convt_heads(ctx, sd, sm, x)
        return P({'x': x}, 's', sd, sm), bns_of(sd, sm), run
    return build


def _layers():
    from efgh_amd.nets import layers
    return layers


def cases():
    """[(name, build)]"""
    out = []

    def add(name, b):
        out.append((name, b))
    # the grid: 3x3 / 1x1 at stride 1 / 2 over the channel counts, maps on both sides of the 8 x 8 limit of the 2-D Winograd path
    for k, s in ((3, 1), (3, 2), (1, 1), (1, 2)):
        for c in (3, 16, 32, 64, 128, 256):
            for H, W in ((6, 7), (8, 8), (12, 16)):
                co = 16 if c == 3 else c
                add('conv %dx%d s%d C%d %dx%d bn' % (k, k, s, c, H, W), conv_case(c, co, k, s, H, W, xgrad=c != 3))
    add('conv 3x3 C32 200x320 bn', conv_case(32, 32, 3, 1, 200, 320, B=1))
    add('conv 3x3 C3->64 bn', conv_case(3, 64, 3, 1, 16, 16, xgrad=False))
    add('conv 3x3 s2 C3->64 bn', conv_case(3, 64, 3, 2, 16, 16, xgrad=False))
    add('conv 1x1 C64->32 bn', conv_case(64, 32, 1, 1, 8, 8))
    for c, H in ((16, 8), (64, 8), (128, 8), (128, 6), (256, 12)):
        t = 'conv 3x3 C%d %dx%d ' % (c, H, H)
        add(t + 'plain', conv_case(c, c, 3, 1, H, H, bn=False, act=0))
        add(t + 'bias', conv_case(c, c, 3, 1, H, H, bn=False, bias=True, act=2, slope=0.2))
        add(t + 'bias bn', conv_case(c, c, 3, 1, H, H, bias=True))
        add(t + 'bn res', conv_case(c, c, 3, 1, H, H, res=True))
        add(t + 'res', conv_case(c, c, 3, 1, H, H, bn=False, res=True))
        add(t + 'bn act none', conv_case(c, c, 3, 1, H, H, act=0))
        add(t + 'bn out', conv_case(c, c, 3, 1, H, H, out=True))
        add(t + 'bn res out', conv_case(c, c, 3, 1, H, H, res=True, out=True))
        add(t + 'bn in_ch', conv_case(c, c, 3, 1, H, H, in_ch=True))
        add(t + 'bn skip_out', conv_case(c, c, 3, 1, H, H, skip_out=True))
        add(t + 'bn no x grad', conv_case(c, c, 3, 1, H, H, xgrad=False))
        add(t + 'bn pool', conv_case(c, c, 3, 1, H, H, pool=True))
        add(t + 'bias bn pool leaky', conv_case(c, c, 3, 1, H, H, pool=True, bias=True, act=2, slope=0.2))
        add(t + 'bn defer', conv_case(c, c, 3, 1, H, H, consumer=c))
    add('conv 3x3 s2 C64 bn skip_out', conv_case(64, 128, 3, 2, 9, 9, skip_out=True))
    add('conv 1x1 s2 C64 bn skip_out', conv_case(64, 128, 1, 2, 9, 9, skip_out=True, act=0))
    add('conv 3x3 C64 defer to a 64-channel consumer', conv_case(64, 128, 3, 1, 8, 8, consumer=64))
    for co in (1, 2, 3, 10):
        add('conv 3x3 C16->%d bn' % co, conv_case(16, co, 3, 1, 8, 8))
        add('conv 3x3 C16->%d bias' % co, conv_case(16, co, 3, 1, 8, 8, bn=False, bias=True))
        add('conv 1x1 C64->%d bn' % co, conv_case(64, co, 1, 1, 8, 8))
        add('conv 3x3 C%d->%d bn' % (co, co), conv_case(co, co, 3, 1, 8, 8))
    # transposed convolutions: odd sizes, output padding 1 and 0, the col2im form at <= 3 output channels
    for co in (64, 32, 3, 2, 1):
        for op in (1, 0):
            add('convT C128->%d op%d 5x7' % (co, op), convt_case(128, co, 5, 7, op=op))
        add('convT C128->%d skip_out' % co, convt_case(128, co, 5, 7, skip_out=True))
        add('convT C128->%d defer_for' % co, convt_case(128, co, 4, 4, defer=True))
        if co % 4 == 0:
            add('convT C128->%d out' % co, convt_case(128, co, 5, 7, out=True))
    add('convT C128->128 defer_for 8x8', convt_case(128, 128, 8, 8, defer=True))
    add('convT C128->128 defer_for skip_out', convt_case(128, 128, 8, 8, defer=True, skip_out=True))
    add('convT C64->3 bias', convt_case(64, 3, 5, 7, bias=True))
    add('convT C64->3 no bn', convt_case(64, 3, 5, 7, bn=False))
    add('convT C64->64 no bn bias', convt_case(64, 64, 5, 7, bn=False, bias=True))
    add('convT 1x1 map', convt_case(64, 64, 1, 1, op=0))
    add('heads C128 8x8', heads_case(128, 8, 8))
    add('heads C64 5x7', heads_case(64, 5, 7))
    # linear rows
    for C, O in ((64, 64), (256, 12), (3, 64), (64, 4), (4, 4)):
        t = 'linear C%d O%d ' % (C, O)
        add(t + 'plain', linear_case(100, C, O, act=0))
        add(t + 'no bias', linear_case(100, C, O, bias=False))
        add(t + 'bn', linear_case(100, C, O, bn=True))
        add(t + 'bn count', linear_case(100, C, O, bn=True, count=90))
        add(t + 'bn slice', linear_case(100, C, O, bn=True, slice_=True))
        add(t + 'slice out', linear_case(100, C, O, slice_=True, out=True))
        add(t + 'bn out', linear_case(100, C, O, bn=True, out=True))
    # BCL blur
    for C, C0, C1 in ((128, 64, 32), (32, 64, 64), (6, 32, 30)):
        t = 'blur C%d ' % C
        add(t + 'table', blur_case(1000, C, C0, C1))
        add(t + 'table out', blur_case(1000, C, C0, C1, out=True))
        add(t + 'level', blur_case(1000, C, C0, C1, level=1))
        add(t + 'level unfused dgrad', blur_case(1000, C, C0, C1, level=1, fused=False))
        add(t + 'r2', blur_case(1000, C, C0, C1, level=2, F=65))
        add(t + 'r2 out', blur_case(1000, C, C0, C1, level=2, F=65, out=True))
    add('blur rows above the k-split limit', blur_case(17000, 128, 64, 32, level=1))
    add(RAISES[0], blur_case(1000, 32, 64, 64, level=2, F=15))
    # the runners
    add('vgg 64 64 M 128 128 M 256 256 M', vgg_case((64, 64, 'M', 128, 128, 'M', 256, 256, 'M'), 32, 32))
    add('vgg 64 M 128 256 odd map', vgg_case((64, 'M', 128, 256), 18, 22, B=2))
    add('vgg 16 16 M 32', vgg_case((16, 16, 'M', 32), 16, 16))
    for ci, co, s, H in ((64, 64, 1, 8), (128, 128, 1, 8), (128, 128, 1, 6), (64, 128, 2, 16), (128, 256, 2, 16), (64, 128, 2, 9), (64, 128, 1, 8)):
        for alias in (False, True):
            t = 'block C%d->%d s%d %dx%d%s' % (ci, co, s, H, H, ' alias_in' if alias else '')
            add(t, block_case(ci, co, s, H, H, alias_in=alias))
            add(t + ' out', block_case(ci, co, s, H, H, alias_in=alias, out=True))
            add('layer ' + t, block_case(ci, co, s, H, H, alias_in=alias, layer=True))
    add('layer block C64->128 s2 out', block_case(64, 128, 2, 16, 16, out=True, layer=True))
    for ci, co in ((128, 64), (256, 128), (64, 32), (32, 16)):
        for skip in (False, True):
            t = 'convt_bn_relu C%d->%d%s' % (ci, co, ' skip_out' if skip else '')
            add(t, convt_bn_relu_case(ci, co, 8, 8, skip_out=skip))
            add(t + ' out', convt_bn_relu_case(ci, co, 4, 6, skip_out=skip, out=True))
    for c in (32, 128):
        add('conv_bn_relu C%d' % c, conv_bn_relu_case(c, c, 8, 8))
        add('conv_bn_relu C%d skip_out' % c, conv_bn_relu_case(c, c, 8, 8, skip_out=True))
        add('conv_bn_relu C%d out in_ch' % c, conv_bn_relu_case(c, c, 8, 8, out=True, in_ch=True))
    return out


def table():
    """{'names': [case names], 'settings': {setting: [[forward calls, backward calls, digest] per case and context]}}"""
    cs = cases()
    names = ['%s | train=%d grad=%d' % (n, t, g) for n, _ in cs for t, g in CONTEXTS]
    assert len(set(names)) == len(names)
    settings = {}
    torch.manual_seed(0)
    with LayerCapture() as cap:
        for sname, sw in SETTINGS:
            for k, v in sw.items():
                setattr(cap.ops, k, v)
            settings[sname] = [cap.case(b, t, g) for _, b in cs for t, g in CONTEXTS]
            for k in sw:
                setattr(cap.ops, k, True)
    return {'names': names, 'settings': settings}


def pack(t):
    """-> the compact form kept in tests/golden/layers.json: the case names as one hash, the entry points met, the distinct call
    sequences (one character per entry point), the distinct records 'forward.backward.digest' (indices into the call sequences),
    'default' as one record index per case, every other setting as the [position, record] pairs where it differs from 'default'"""
    eps, seqs, recs = {}, {}, {}

    def seq(c):
        return seqs.setdefault(''.join(chr(35 + eps.setdefault(e, len(eps))) for e in c.split('+')), len(seqs))

    def rec(r):
        return recs.setdefault('%d.%d.%s' % (seq(r[0]), seq(r[1]), r[2]), len(recs))
    ids = {s: [rec(r) for r in rows] for s, rows in t['settings'].items()}
    assert len(eps) <= 90
    settings = {'default': ids['default']}
    for s, _ in SETTINGS[1:]:
        settings[s] = [x for i, (a, b) in enumerate(zip(ids['default'], ids[s])) if a != b for x in (i, b)]
    return {'names': [len(t['names']), RC._h(t['names'])], 'entries': sorted(eps, key=eps.get), 'calls': sorted(seqs, key=seqs.get),
            'records': sorted(recs, key=recs.get), 'settings': settings}


def unpack(f):
    """the compact form -> {setting: [[forward calls, backward calls, digest] per case and context]}"""
    calls = ['+'.join(f['entries'][ord(ch) - 35] for ch in c) for c in f['calls']]

    def row(i):
        a, b, h = f['records'][i].split('.', 2)
        return [calls[int(a)], calls[int(b)], h]
    out = {'default': [row(i) for i in f['settings']['default']]}
    for s, _ in SETTINGS[1:]:
        ids, d = list(f['settings']['default']), f['settings'][s]
        for pos, r in zip(d[::2], d[1::2]):
            ids[pos] = r
        out[s] = [row(i) for i in ids]
    return out


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    t = table()
    packed = pack(t)
    assert unpack(json.loads(RC.dumps(packed))) == t['settings'], 'pack / unpack do not round-trip'
    open(sys.argv[1], 'w').write(RC.dumps(packed))
