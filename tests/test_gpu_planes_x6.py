"""The split-bf16 plane GEMMs (efgh_plane_gemm_x6 / efgh_plane_wgrad_x6_batched, fp32 'high' matmul precision) on the GPU:
kernel accuracy against float64 next to the exact kernels on the same inputs, guard rows, run-to-run bit identity, refusals and
NaN propagation; a 2-D Winograd layer's y / dx / dW under the mode; the mode a forward resolved carried into its backward; and
the config-S model (eval forward against the oracle, batch-2 training step against the batched oracle, bit-reproducible
gradients) with the mode on."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (T2, C, N): the sets of tests/test_gpu_ops.py's plane tests, then the config-S shapes at batch 2 (2*H*W/16 tiles) and ragged counts
GEMM_SHAPES = [(128, 128, 128), (1000, 256, 128), (777, 128, 384), (4099, 512, 256), (37, 64, 128),
               (3840, 256, 256), (960, 512, 512), (3847, 256, 256), (963, 512, 512)]
WGRAD_SHAPES = [(256, 128, 128), (5000, 256, 128), (3333, 128, 256), (20011, 256, 256), (3840, 512, 512),
                (15360, 128, 128), (3840, 256, 256), (960, 512, 512), (15365, 128, 128)]


def _lib():
    from efgh_amd import _C
    return _C, _C.lib()


def _gemm_desc(_C, V, U, o, T2, C, N):
    g = _C.GemmDesc()
    g.A, g.lda, g.C, g.T, g.mode = V.data_ptr(), 36 * C, C, 1, 0
    g.W, g.N, g.M = U.data_ptr(), N, T2
    g.out, g.ldo = o.data_ptr(), 36 * N
    g.nbatch, g.batch_stride_a, g.batch_stride_w, g.batch_stride_out = 36, C, N * C, N
    return g


def _run_gemm(x6, V, U, T2, C, N, nbuf=0):
    _C, lib = _lib()
    o = torch.full((T2 + 1, 36, N), 7.0, device='cuda')          # (one guard row behind the last tile)
    g = _gemm_desc(_C, V, U, o, T2, C, N)
    fn = lib.efgh_plane_gemm_x6 if x6 else lib.efgh_plane_gemm
    _C.check(fn(ctypes.byref(g), _C.c_int32(nbuf), _C.stream_ptr()))
    torch.cuda.synchronize()
    return o


def _run_wgrad(x6, V, Gy, T2, C, N, nbuf=0):
    _C, lib = _lib()
    g = _C.GemmDesc()
    g.A, g.lda, g.C, g.T, g.mode, g.N, g.M = V.data_ptr(), 36 * C, C, 1, 0, N, T2
    g.nbatch, g.batch_stride_a = 36, C
    assert lib.efgh_plane_wgrad_supported(ctypes.byref(g), _C.c_int64(36 * N)) == 1
    S = torch.full((36, N, C), 3.0, device='cuda')
    ws = torch.empty(max(1, lib.efgh_plane_wgrad_workspace(ctypes.byref(g))), device='cuda')
    fn = lib.efgh_plane_wgrad_x6_batched if x6 else lib.efgh_plane_wgrad_batched
    _C.check(fn(ctypes.byref(g), _C.ptr(Gy), _C.c_int64(36 * N), _C.c_int64(N), _C.ptr(S), _C.c_int64(N * C), _C.ptr(ws),
                _C.c_int32(nbuf), _C.stream_ptr()))
    torch.cuda.synchronize()
    return S


def _errs(got, ref):
    d = got.double() - ref
    return float(d.abs().max()), float(d.norm() / ref.norm())


@pytest.mark.parametrize('T2,C,N', GEMM_SHAPES)
def test_plane_gemm_x6_accuracy_vs_float64(T2, C, N):
    torch.manual_seed(T2 + C + N)
    V = torch.randn(T2, 36, C, device='cuda')
    U = torch.randn(36, N, C, device='cuda')
    ref = torch.einsum('tac,anc->tan', V.double(), U.double())
    ex = _run_gemm(False, V, U, T2, C, N)
    x6 = _run_gemm(True, V, U, T2, C, N)
    assert bool((x6[T2] == 7.0).all())                                  # nothing written past the last row
    assert torch.equal(x6, _run_gemm(True, V, U, T2, C, N))             # bit-reproducible run to run
    assert torch.equal(x6, _run_gemm(True, V, U, T2, C, N, nbuf=3))     # (the ring depth changes nothing but the schedule)
    (mx_e, l2_e), (mx_s, l2_s) = _errs(ex[:T2], ref), _errs(x6[:T2], ref)
    print('gemm %s: exact max %.2e rel-L2 %.2e | x6 max %.2e rel-L2 %.2e' % ((T2, C, N), mx_e, l2_e, mx_s, l2_s))
    assert mx_s <= 1.25 * mx_e and l2_s <= 1.25 * l2_e
    assert l2_s < 2e-6
    assert not torch.equal(ex, x6)                                      # (a different arithmetic really ran)


@pytest.mark.parametrize('T2,C,N', WGRAD_SHAPES)
def test_plane_wgrad_x6_accuracy_vs_float64(T2, C, N):
    torch.manual_seed(T2 + 3 * C + N)
    V = torch.randn(T2, 36, C, device='cuda')
    Gy = torch.randn(T2, 36, N, device='cuda')
    ref = torch.einsum('tan,tac->anc', Gy.double(), V.double())
    ex = _run_wgrad(False, V, Gy, T2, C, N)
    x6 = _run_wgrad(True, V, Gy, T2, C, N)
    assert torch.equal(x6, _run_wgrad(True, V, Gy, T2, C, N))           # fixed chunks, fixed fold order
    (mx_e, l2_e), (mx_s, l2_s) = _errs(ex, ref), _errs(x6, ref)
    print('wgrad %s: exact max %.2e rel-L2 %.2e | x6 max %.2e rel-L2 %.2e' % ((T2, C, N), mx_e, l2_e, mx_s, l2_s))
    assert mx_s <= 1.25 * mx_e and l2_s <= 1.25 * l2_e
    assert l2_s < 5e-6


def test_plane_x6_refuses_what_the_exact_forms_refuse():
    _C, lib = _lib()
    V, U, o = torch.randn(64, 96, device='cuda'), torch.randn(64, 96, device='cuda'), torch.empty(64, 64, device='cuda')
    g = _C.GemmDesc()
    g.A, g.lda, g.C, g.T, g.mode, g.W, g.N, g.M, g.out, g.ldo = V.data_ptr(), 96, 96, 1, 0, U.data_ptr(), 64, 64, o.data_ptr(), 64
    assert lib.efgh_plane_gemm_supported(ctypes.byref(g)) == 0           # N % 128 != 0
    assert lib.efgh_plane_gemm_x6(ctypes.byref(g), _C.c_int32(0), _C.stream_ptr()) != 0
    assert lib.efgh_plane_wgrad_x6_batched(ctypes.byref(g), _C.ptr(U), _C.c_int64(64), _C.c_int64(0), _C.ptr(o), _C.c_int64(0),
                                           None, _C.c_int32(0), _C.stream_ptr()) != 0
    V2, U2 = torch.randn(40, 36, 128, device='cuda'), torch.randn(36, 128, 128, device='cuda')
    o2 = torch.empty(40, 36, 128, device='cuda')
    g2 = _gemm_desc(_C, V2, U2, o2, 40, 128, 128)
    assert lib.efgh_plane_gemm_x6(ctypes.byref(g2), _C.c_int32(4), _C.stream_ptr()) != 0        # nbuf 2 or 3 only
    g2.act = 1                                                                                     # no epilogue
    assert lib.efgh_plane_gemm_supported(ctypes.byref(g2)) == 0
    assert lib.efgh_plane_gemm_x6(ctypes.byref(g2), _C.c_int32(0), _C.stream_ptr()) != 0
    torch.cuda.synchronize()


def test_plane_x6_nan_propagates():
    """a NaN operand gives NaN outputs in its row / column (an Inf may give NaN as well: its residual is Inf - Inf); the other
    outputs stay finite"""
    T2, C, N = 300, 128, 128
    torch.manual_seed(5)
    V = torch.randn(T2, 36, C, device='cuda')
    U = torch.randn(36, N, C, device='cuda')
    V[17, 3, 40] = float('nan')
    U[9, 100, 5] = float('nan')
    o = _run_gemm(True, V, U, T2, C, N)[:T2]
    assert bool(o[17, 3].isnan().all()) and bool(o[:, 9, 100].isnan().all())
    keep = torch.ones_like(o, dtype=torch.bool)
    keep[17, 3] = False
    keep[:, 9, 100] = False
    assert bool(torch.isfinite(o[keep]).all())
    Gy = torch.randn(T2, 36, N, device='cuda')
    V2 = torch.randn(T2, 36, C, device='cuda')
    V2[33, 7, 64] = float('nan')
    S = _run_wgrad(True, V2, Gy, T2, C, N)
    assert bool(S[7, :, 64].isnan().all())
    S[7, :, 64] = 0
    assert bool(torch.isfinite(S).all())


# ---------------------------------------------------------------------------------------------------------------------------------
def _layer(split, x, conv, bn, gy):
    """one 256 -> 256 3x3 convolution + train-mode BatchNorm + LeakyReLU on the HIP path with ops.PLANES_SPLIT = split:
    (y, dx, dW) and the split-hit counts it added (forward, backward)"""
    import copy
    from efgh_amd import ops
    from efgh_amd.nets import layers as L
    conv_g, bn_g = copy.deepcopy(conv).cuda(), copy.deepcopy(bn).cuda()
    bn_g.train(True)
    cin, cout = conv.in_channels, conv.out_channels
    old = ops.PLANES_SPLIT
    ops.PLANES_SPLIT = split
    try:
        xg = ops.nchw_to_nhwc(x.cuda(), cin).requires_grad_(True)
        h0 = list(ops.PLANE_SPLIT_HITS)
        yg = L.conv2d(L.Ctx(True), xg, conv_g, bn_g, L.ACT_LEAKY, 0.2)
        torch.cuda.synchronize()
        h1 = list(ops.PLANE_SPLIT_HITS)
        gyg = torch.zeros_like(yg)
        gyg[..., :cout] = gy.permute(0, 2, 3, 1).cuda()
        yg.backward(gyg)
        torch.cuda.synchronize()
        h2 = list(ops.PLANE_SPLIT_HITS)
    finally:
        ops.PLANES_SPLIT = old
    outs = (yg[..., :cout].permute(0, 3, 1, 2).detach(), xg.grad[..., :cin].permute(0, 3, 1, 2), conv_g.weight.grad.clone())
    return outs, (h1[0] - h0[0], h1[1] - h0[1]), (h2[0] - h1[0], h2[1] - h1[1])


def _layer_case(seed=0, hw=(24, 40)):
    torch.manual_seed(seed)
    conv = nn.Conv2d(256, 256, 3, 1, 1, bias=True)
    bn = nn.BatchNorm2d(256)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.2)
    x = torch.randn(2, 256, *hw)
    # float64 reference: conv2d, train-mode BatchNorm, LeakyReLU
    x64 = x.double().requires_grad_(True)
    w64 = conv.weight.detach().double().requires_grad_(True)
    y0 = F.conv2d(x64, w64, conv.bias.detach().double(), padding=1)
    yb = F.batch_norm(y0, None, None, bn.weight.detach().double(), bn.bias.detach().double(), training=True, eps=bn.eps)
    y = F.leaky_relu(yb, 0.2)
    gy = torch.randn(y.shape, dtype=torch.float64)
    gy = gy * (yb.detach().abs() > 1e-3)                     # (no gradient at the activation's kink: an fp32 flip there is not an error)
    y.backward(gy)
    return x, conv, bn, gy.float(), (y.detach(), x64.grad, w64.grad)


def _rel_l2(a, ref):
    return float((a.double().cpu() - ref).norm() / ref.norm())


def test_wino2d_layer_under_split_vs_float64():
    x, conv, bn, gy, ref = _layer_case()
    exact, hf_e, hb_e = _layer(False, x, conv, bn, gy)
    split, hf_s, hb_s = _layer(True, x, conv, bn, gy)
    assert hf_e == (0, 0) and hb_e == (0, 0)
    assert hf_s[0] > 0 and hf_s[1] == 0                     # forward planes
    assert hb_s[0] > 0 and hb_s[1] > 0                      # data-gradient planes and weight-gradient planes
    for what, e, s, r in zip(('y', 'dx', 'dW'), exact, split, ref):
        ee, es = _rel_l2(e, r), _rel_l2(s, r)
        print('%s: exact %.2e split %.2e' % (what, ee, es))
        assert es <= 1.25 * ee + 1e-7, (what, ee, es)


def test_wino2d_layer_default_switch_is_exact(monkeypatch):
    """torch at its default: no split launch, outputs bit-identical to PLANES_SPLIT = False"""
    x, conv, bn, gy, _ = _layer_case(1, (16, 28))
    torch.backends.cuda.matmul.fp32_precision = 'ieee'
    try:
        dflt, hf, hb = _layer(None, x, conv, bn, gy)
    finally:
        torch.backends.cuda.matmul.fp32_precision = 'none'
    exact, _, _ = _layer(False, x, conv, bn, gy)
    assert hf == (0, 0) and hb == (0, 0)
    for a, b in zip(dflt, exact):
        assert torch.equal(a, b)


@pytest.mark.parametrize('fwd,bwd', [('tf32', 'ieee'), ('ieee', 'tf32')])
def test_split_mode_is_carried_into_backward(fwd, bwd):
    """the mode a layer's forward resolved holds for its backward (run on autograd's device thread) even if torch's switch
    changes in between: the gradients are bit-identical to a step run entirely in the forward's mode"""
    import copy
    from efgh_amd import ops
    from efgh_amd.nets import layers as L
    x, conv, bn, gy, _ = _layer_case(2, (16, 28))
    m = torch.backends.cuda.matmul
    ref, _, _ = _layer(fwd == 'tf32', x, conv, bn, gy)
    conv_g, bn_g = copy.deepcopy(conv).cuda(), copy.deepcopy(bn).cuda()
    bn_g.train(True)
    assert ops.PLANES_SPLIT is None
    try:
        m.fp32_precision = fwd
        xg = ops.nchw_to_nhwc(x.cuda(), 256).requires_grad_(True)
        yg = L.conv2d(L.Ctx(True), xg, conv_g, bn_g, L.ACT_LEAKY, 0.2)
        m.fp32_precision = bwd
        gyg = torch.zeros_like(yg)
        gyg[..., :256] = gy.permute(0, 2, 3, 1).cuda()
        h0 = list(ops.PLANE_SPLIT_HITS)
        yg.backward(gyg)
        torch.cuda.synchronize()
        h1 = list(ops.PLANE_SPLIT_HITS)
    finally:
        m.fp32_precision = 'none'
    if fwd == 'tf32':
        assert h1[0] > h0[0] and h1[1] > h0[1]
    else:
        assert h1 == h0
    assert torch.equal(xg.grad[..., :256].permute(0, 3, 1, 2), ref[1])
    assert torch.equal(conv_g.weight.grad, ref[2])


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def split_on():
    from efgh_amd import ops
    old = ops.PLANES_SPLIT
    ops.PLANES_SPLIT = True
    yield ops
    ops.PLANES_SPLIT = old


def test_fullsize_eval_forward_under_split_vs_oracle(manifest, split_on):
    """config S, eval forward with the split planes against the oracle: the pose-logit bar of tests/test_gpu_fullsize.py"""
    from test_gpu_fullsize import NPTS, RAW, _eval_forward, _stagewise          # (tests/ is on sys.path under pytest)
    h0 = split_on.PLANE_SPLIT_HITS[0]
    st = _eval_forward(manifest, RAW, NPTS)
    assert split_on.PLANE_SPLIT_HITS[0] > h0
    _stagewise(st, manifest, RAW)


def test_fullsize_training_step_batch2_under_split_vs_batched_oracle(manifest, monkeypatch, split_on):
    from efgh_amd import synthetic as syn
    from test_gpu_fullsize import NPTS, RAW, _training_step
    h0 = list(split_on.PLANE_SPLIT_HITS)
    rel, relg = _training_step(manifest, monkeypatch, RAW, NPTS, batch=syn.make_batch(RAW, NPTS, 2))
    assert rel['E'] < 2e-3 and rel['H'] < 1e-2 and (rel['F'] == 0.0 or rel['F'] < 2e-2), rel
    assert relg < 2e-2
    assert split_on.PLANE_SPLIT_HITS[0] > h0[0] and split_on.PLANE_SPLIT_HITS[1] > h0[1]


def test_training_step_under_split_is_bit_reproducible(manifest, split_on):
    """two identical batch-2 training steps with the split planes give bit-identical gradients"""
    from efgh_amd import synthetic as syn
    from efgh_amd.losses import EFGHCriterion
    from efgh_amd.nets import EFGHBackbone
    raw, npts = (384, 1280), 65536
    args = syn.default_args(raw, 'cuda')
    b = syn.make_batch(raw, npts, 2)
    inp = [torch.from_numpy(b[k]).cuda() for k in ('pc', 'img', 'calib', 'A')]
    grads = []
    for _ in range(2):
        m = EFGHBackbone(args)
        m.load_state_dict(syn.synthetic_state_dict(manifest['state_dict'], 1), strict=True)
        m = m.cuda().train()
        crit = EFGHCriterion(args)
        h0 = list(split_on.PLANE_SPLIT_HITS)
        pred = m(*inp)
        L, _ = crit.compute_loss(inp[0], inp[1], inp[2], inp[3], {k: torch.from_numpy(v) for k, v in b['gt'].items()}, pred)
        L['total'].backward()
        torch.cuda.synchronize()
        assert split_on.PLANE_SPLIT_HITS[0] > h0[0] and split_on.PLANE_SPLIT_HITS[1] > h0[1]
        grads.append({k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 0
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
