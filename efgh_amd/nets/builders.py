"""Parameter containers with the reference's module names / shapes / init.
Only construction lives here; execution is in layers.py (HIP)."""
import numbers

import torch.nn as nn


def init_small(m):
    """N(0,1e-3) weights, zero bias; BN2d to (1,0)   (nets/net_utils.py:22-33)"""
    if isinstance(m, (nn.Conv2d, nn.Linear, nn.ConvTranspose2d)):
        m.weight.data.normal_(0, 1e-3)
        if m.bias is not None:
            m.bias.data.zero_()
    elif isinstance(m, nn.BatchNorm2d):
        m.weight.data.fill_(1)
        m.bias.data.zero_()


def conv_1x1(cin, cout, leaky):
    """Conv1d(k=1)+ReLU/LeakyReLU(0.1)  (net_utils.py:35-43; Conv1d keeps torch's default init)"""
    act = nn.LeakyReLU(0.1, inplace=True) if leaky else nn.ReLU(inplace=True)
    return nn.Sequential(nn.Conv1d(cin, cout, 1, 1, 0, bias=True), act)


def conv_bn_relu(cin, cout, k, stride=1, padding=0):
    seq = nn.Sequential(nn.Conv2d(cin, cout, k, stride, padding, bias=False), nn.BatchNorm2d(cout),
                        nn.LeakyReLU(0.2, inplace=True))
    seq.apply(init_small)
    return seq


def convt_bn_relu(cin, cout, k, stride=1, padding=0, output_padding=0):
    seq = nn.Sequential(nn.ConvTranspose2d(cin, cout, k, stride, padding, output_padding, bias=False),
                        nn.BatchNorm2d(cout), nn.LeakyReLU(0.2, inplace=True),
                        nn.Conv2d(cout, cout, 3, 1, 1, bias=False), nn.BatchNorm2d(cout),
                        nn.LeakyReLU(0.2, inplace=True))
    seq.apply(init_small)
    return seq


class VGGFeatures(nn.Module):
    """`features` of nets/vgg.py:69-83 with kaiming-normal(fan_out) conv init (:55-66)."""
    CFG = {'A': [64, 'M', 128, 'M', 256, 256, 'M', 512, 512, 'M', 512, 512, 'M'],
           'C': [64, 'M', 128, 'M', 256, 256, 'M', 512, 512, 'M']}

    def __init__(self, cfg):
        super().__init__()
        layers, cin = [], 3
        for v in self.CFG[cfg]:
            if v == 'M':
                layers.append(nn.MaxPool2d(2, 2))
            else:
                layers += [nn.Conv2d(cin, v, 3, padding=1), nn.BatchNorm2d(v), nn.ReLU(inplace=True)]
                cin = v
        self.features = nn.Sequential(*layers)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)


class BasicBlock(nn.Module):
    """parameter layout of nets/resnet.py:33-53"""

    def __init__(self, inplanes, planes, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        if stride != 1 or inplanes != planes:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False),
                                            nn.BatchNorm2d(planes))


def resnet18_layers():
    """layer1..4 of resnet18 (resnet.py:171-193, 226-234), re-initialised N(0,1e-3) (gnet.py:32,83)"""
    out, inpl = [], 64
    for planes, stride in ((64, 1), (128, 2), (256, 2), (512, 2)):
        layer = nn.Sequential(BasicBlock(inpl, planes, stride), BasicBlock(planes, planes, 1))
        layer.apply(init_small)
        out.append(layer)
        inpl = planes
    return out


class BilateralConvFlex(nn.Module):
    """nets/bilateralNN.py:55-263: splat -> blur / convolution stack -> slice on one permutohedral lattice level, with the
    reference's constructor values, buffers, parameters (names, shapes, order, init) and results.

    BilateralConvFlex(num_input, num_output, neighborhood_size=1, *, d=3, use_bias=True, use_leaky=True, use_norm=True,
    do_splat=True, do_slice=False, last_relu=False) - or the reference's own positional order (d, neighborhood_size, num_input,
    num_output, DEVICE, use_bias, use_leaky, use_norm, do_splat, do_slice, last_relu[, chunk_size]).  neighborhood_size = the
    radius r of the blur, (r+1)^4 - r^4 taps (get_filter_size); num_output: one channel count per convolution, any length >= 1
    (the first is the (F,1) blur, the others (1,1)); DEVICE and chunk_size are accepted and ignored (the kernels run where the
    tensors live; chunking does not change a value).  d = 3, radius 1 / 2 / 3 and channel counts that are multiples of 4 are
    served; anything else raises EfghError.

    LAYOUT: forward(features, level, out_points=None) takes ROWS, channels last - features [n_in][num_input] (do_splat: one row
    per point of `level`, an efgh_amd.lattice.LatticeLevel covering all samples of the batch, sample-major) or [H][num_input]
    (do_splat=False: one row per lattice vertex) - and returns [n_out][num_output[-1]] (do_slice: one row per point of
    `out_points`, an efgh_amd.lattice.OutPoints; None = the level's own points) or [H][num_output[-1]].  The reference's
    (B, C, N) tensors, its barycentric / offset / neighbour arguments and its zero row live in the level."""

    def __init__(self, *args, **kw):
        super().__init__()
        import torch
        from .._C import EfghError
        from ..lattice import check_radii, filter_size
        if len(args) >= 2 and not isinstance(args[1], (list, tuple)):       # the reference's positional order
            names = ('d', 'neighborhood_size', 'num_input', 'num_output', 'DEVICE', 'use_bias', 'use_leaky', 'use_norm', 'do_splat',
                     'do_slice', 'last_relu', 'chunk_size')
        else:
            names = ('num_input', 'num_output', 'neighborhood_size')
        if len(args) > len(names) or any(n in kw for n in names[:len(args)]):
            raise TypeError('BilateralConvFlex: too many or repeated arguments')
        kw.update(zip(names, args))
        known = dict(d=3, neighborhood_size=1, DEVICE=None, use_bias=True, use_leaky=True, use_norm=True, do_splat=True, do_slice=False,
                     last_relu=False, chunk_size=None)
        extra = set(kw) - set(known) - {'num_input', 'num_output'}
        if extra or 'num_input' not in kw or 'num_output' not in kw:
            raise TypeError('BilateralConvFlex: num_input and num_output are required; unknown arguments %s' % sorted(extra))
        known.update(kw)
        num_input, num_output = known['num_input'], list(known['num_output'])
        if known['d'] != 3:
            raise EfghError('BilateralConvFlex: d = %r; the permutohedral lattice is built for d = 3 only' % (known['d'],))
        self.d, self.d1 = 3, 4
        self.neighborhood_size = check_radii([known['neighborhood_size']], 1)[0]
        chans = [num_input] + num_output
        if len(num_output) < 1 or any(isinstance(c, bool) or not isinstance(c, numbers.Integral) or c < 4 or c % 4 for c in chans):
            raise EfghError('BilateralConvFlex: num_input %r / num_output %r - channel counts that are multiples of 4 are served (float4 rows)'
                            % (num_input, num_output))
        F = self.filter_size = filter_size(self.neighborhood_size)
        self.num_input, self.num_output = int(num_input), [int(c) for c in num_output]
        num_input, num_output = self.num_input, self.num_output
        self.use_bias, self.use_leaky, self.use_norm = bool(known['use_bias']), bool(known['use_leaky']), bool(known['use_norm'])
        self.do_splat, self.do_slice, self.last_relu = bool(known['do_splat']), bool(known['do_slice']), bool(known['last_relu'])
        # registration order = the reference's (bilateralNN.py:99-143): the state_dict lists its keys in the same order
        self.register_buffer('feat_indices', torch.arange(num_input, dtype=torch.long))
        if self.do_slice:
            self.register_buffer('out_indices', torch.arange(num_output[-1], dtype=torch.long))
        seq, cin = [], num_input
        for i, cout in enumerate(num_output):
            seq.append(nn.Conv2d(cin, cout, (F, 1) if i == 0 else (1, 1), 1, 0, bias=True))
            if i < len(num_output) - 1:
                seq.append(nn.ReLU(inplace=False))
            elif self.last_relu:
                seq.append(nn.LeakyReLU(0.1, inplace=False) if self.use_leaky else nn.ReLU(inplace=False))
            cin = cout
        self.blur_conv = nn.Sequential(*seq)
        self.blur_conv.apply(init_small)
        if self.do_slice and self.use_bias:
            self.register_parameter('bias', nn.Parameter(torch.zeros((num_output[-1],), dtype=torch.float32), requires_grad=True))

    def forward(self, features, level, out_points=None):
        """rows in, rows out (see the class docstring); runs layers.bilateral_conv on the HIP path, with autograd when it is on"""
        from . import layers as L
        return L.bilateral_conv(L.Ctx(self.training), self, features, level, out_points)
