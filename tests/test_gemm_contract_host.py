"""The float64 reference of the gather-GEMM contract (tests/gemm_contract.py) on the CPU: against torch's own float64 convolutions
on descriptors built the way nets/layers.py builds them, its error bound against injected faults at the largest reduction each
kernel family meets in the model, and the Python dispatch predicates of ops.py against the C predicates of the library."""
import ctypes
import itertools
import os

import pytest
import torch
import torch.nn.functional as F

import gemm_contract as GC

torch.manual_seed(0)
DT = torch.float32


def _lay(x):
    """(B, C, H, W) -> [B][H][W][C] float32, contiguous"""
    return x.permute(0, 2, 3, 1).contiguous().to(DT)


def _pack_conv(w, Cp=None):
    """Conv2d weight (O, C, kh, kw) -> packed [O][T][Cp] (layers.conv2d: ops.pack_weight(w, O, T, Cw, Cw*T, T, 1, range(T)))"""
    O, C, kh, kw = w.shape
    Cp = Cp or C
    p = torch.zeros((O, kh * kw, Cp), dtype=DT)
    p[:, :, :C] = w.reshape(O, C, kh * kw).permute(0, 2, 1)
    return p


def _launch(**kw):
    L = dict(A=None, lda=0, C=0, T=1, Wp=None, N=0, M=0, out=None, ldo=0, mode=0, geom=None, table=None, bias=None, scale=None,
             shift=None, residual=None, ldr=0, act=0, slope=0.0, stats=None, a_off=0, out_off=0, res_off=0, M_dev=None, batch=None,
             alias_mask=False, bn_bwd=None, pool=False, lazy=None, pre_v=None)
    L.update(kw)
    return L


def emulate(L):
    """what an exact kernel leaves in flat(out) (float64, everything outside the write set as it was) and its [1][2][N] statistics"""
    out = GC.flat(L['out']).double().clone()
    M, N = GC.m_launch(L), L['N']
    s = torch.zeros((1, 2, N), dtype=torch.float64)
    for z in range(GC.nbatch(L)):
        ms = torch.arange(M, dtype=torch.int64)
        f = GC.forward_rows(L, ms, z)
        out[GC.out_index(L, f['orow'], z)] = f['v']
        s[0, 0] += f['pre'].sum(0)
        s[0, 1] += (f['pre'] ** 2).sum(0)
    return out, s


def _run(L):
    """emulate L into its out buffer (rounded to float32) -> the reference's own check of that result"""
    ref, s = emulate(L)
    before = GC.flat(L['out']).clone()
    GC.flat(L['out']).copy_(ref.to(DT))
    if L['stats'] is not None:
        L['stats'].copy_(s.to(DT))
    return before, ref


# --------------------------------------------------------------------------------------------------- reference vs torch
CONV_CASES = {      # (kh, kw, stride, pad)
    'same3x3': (3, 3, 1, 1),
    '3x3s2': (3, 3, 2, 1),
    '1x1s2': (1, 1, 2, 0),
    'range1x2': (1, 2, 1, 0),
}


@pytest.mark.parametrize('case', sorted(CONV_CASES))
def test_forward_conv_vs_torch(case):
    """mode 1 with a channel slice of the input (a_off, lda > C), the output into channels [out_off, out_off + N) of a wider buffer
    (ldo > N), bias / scale / shift / residual / leaky ReLU and the statistics epilogue"""
    kh, kw, s, p = CONV_CASES[case]
    B, H, W, C, N, ldx, cx, ldo, co = 2, 9, 11, 8, 12, 20, 4, 24, 8
    x = torch.randn(B, ldx, H, W, dtype=torch.float64)
    w = torch.randn(N, C, kh, kw, dtype=torch.float64)
    b, sc, sh = torch.randn(N, dtype=torch.float64), torch.randn(N, dtype=torch.float64), torch.randn(N, dtype=torch.float64)
    Ho, Wo = (H + 2 * p - kh) // s + 1, (W + 2 * p - kw) // s + 1
    res = torch.randn(B, N, Ho, Wo, dtype=torch.float64)
    out = torch.full((B, Ho, Wo, ldo), 7.0, dtype=DT)
    T = kh * kw
    geom = (B, H, W, Ho, Wo, s, s, [i // kw - p for i in range(T)], [i % kw - p for i in range(T)], Ho, Wo, 1, 1, 0, 0)
    stats = torch.empty((1, 2, N), dtype=DT)
    L = _launch(A=_lay(x), lda=ldx, C=C, T=T, Wp=_pack_conv(w.to(DT)), N=N, M=B * Ho * Wo, out=out, ldo=ldo, mode=1, geom=geom,
                bias=b.to(DT), scale=sc.to(DT), shift=sh.to(DT), residual=_lay(res), ldr=N, act=2, slope=0.1, a_off=cx, out_off=co,
                stats=stats)
    before, _ = _run(L)
    xs = x[:, cx:cx + C].to(DT).double()
    pre = F.conv2d(xs, w.to(DT).double(), b.to(DT).double(), stride=s, padding=p)
    y = F.leaky_relu(pre * sc.to(DT).double()[:, None, None] + sh.to(DT).double()[:, None, None] + _lay(res).double().permute(0, 3, 1, 2), 0.1)
    got = out[..., co:co + N].permute(0, 3, 1, 2).double()
    assert float((got - y).abs().max()) <= 1e-6 * float(y.abs().max())
    assert torch.equal(out[..., :co], torch.full_like(out[..., :co], 7.0)) and torch.equal(out[..., co + N:], torch.full_like(out[..., co + N:], 7.0))
    assert torch.allclose(stats[0, 0].double(), pre.sum((0, 2, 3)), rtol=1e-6, atol=1e-6)
    assert torch.allclose(stats[0, 1].double(), (pre ** 2).sum((0, 2, 3)), rtol=1e-6, atol=1e-6)
    r = GC.check_forward(L, GC.flat(out), before, GC.TAU['fp32'])
    assert r['bad'] == 0 and r['wild'] == 0 and r['stats'][1] == 0, r


def _convt_launches(x, w, ph, oph, out, ldo):
    """nn.ConvTranspose2d(k=3, s=2) as the four output-parity classes of layers.conv_transpose2d"""
    B, H, W, Cw = x.shape
    O = w.shape[1]
    Ho, Wo = (H - 1) * 2 - 2 * ph + 3 + oph, (W - 1) * 2 - 2 * ph + 3 + oph
    Ls = []
    for cy in range(2):
        for cx in range(2):
            taps = [(a, b_) for a in range(3) if (cy + ph - a) % 2 == 0 for b_ in range(3) if (cx + ph - b_) % 2 == 0]
            Hv, Wv = (Ho - cy + 1) // 2, (Wo - cx + 1) // 2
            if Hv <= 0 or Wv <= 0:
                continue
            dh = [(cy + ph - a) // 2 for a, _ in taps]
            dw = [(cx + ph - b_) // 2 for _, b_ in taps]
            tapidx = [a * 3 + b_ for a, b_ in taps]
            Wp = w.reshape(Cw, O, 9)[:, :, tapidx].permute(1, 2, 0).contiguous().to(DT)          # [O][T][Cw]
            geom = (B, H, W, Hv, Wv, 1, 1, dh, dw, Ho, Wo, 2, 2, cy, cx)
            Ls.append(_launch(A=x, lda=Cw, C=Cw, T=len(taps), Wp=Wp, N=O, M=B * Hv * Wv, out=out, ldo=ldo, mode=1, geom=geom))
    return Ls, Ho, Wo


@pytest.mark.parametrize('ph,oph', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_forward_conv_transpose_classes_vs_torch(ph, oph):
    """the four output classes (osh = 2, oh0 / ow0 = parity) of a stride-2 ConvTranspose2d tile the output exactly: every
    class writes only its own pixels"""
    B, H, W, Cw, O = 2, 5, 7, 8, 12
    x = torch.randn(B, Cw, H, W, dtype=torch.float64)
    w = torch.randn(Cw, O, 3, 3, dtype=torch.float64)
    Ho, Wo = (H - 1) * 2 - 2 * ph + 3 + oph, (W - 1) * 2 - 2 * ph + 3 + oph
    out = torch.full((B, Ho, Wo, O), float('nan'), dtype=DT)
    Ls, _, _ = _convt_launches(_lay(x), w, ph, oph, out, O)
    for L in Ls:
        before, _ = _run(L)
        r = GC.check_forward(L, GC.flat(out), before, GC.TAU['fp32'])
        assert r['bad'] == 0 and r['wild'] == 0, r
    ref = F.conv_transpose2d(x.to(DT).double(), w.to(DT).double(), stride=2, padding=ph, output_padding=oph)
    assert float((out.permute(0, 3, 1, 2).double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())


@pytest.mark.parametrize('k', [1, 3])
def test_data_gradient_geometry_vs_autograd(k):
    """the stride-2 data gradient of layers._conv2d_dgrad: one launch per input-parity class on the gradient (Ho x Wo) with the placement
    (2i + cy, 2j + cx) in the input image; for the 1x1 downsample only one class exists and it accumulates into the other branch's
    gradient in place (residual = out)"""
    B, H, W, C, O = 2, 9, 10, 8, 12
    p = k // 2
    x = torch.randn(B, C, H, W, dtype=torch.float64, requires_grad=True)
    w = torch.randn(O, C, k, k, dtype=torch.float64)
    y = F.conv2d(x, w.to(DT).double(), stride=2, padding=p)
    gy = torch.randn_like(y).to(DT).double()
    add = torch.randn(B, C, H, W, dtype=torch.float64).to(DT).double()
    (dx,) = torch.autograd.grad(y, x, gy)
    Ho, Wo = y.shape[2], y.shape[3]
    T = k * k
    dxo = _lay(add) if k == 1 else torch.full((B, H, W, C), float('nan'), dtype=DT)
    for cy in range(2):
        for cx in range(2):
            taps = [(a, b_) for a in range(k) if (cy + p - a) % 2 == 0 for b_ in range(k) if (cx + p - b_) % 2 == 0]
            Hv, Wv = (H - cy + 1) // 2, (W - cx + 1) // 2
            if not taps:
                continue
            tapidx = [a * k + b_ for a, b_ in taps]
            Wd = w.to(DT).reshape(O, C, T)[:, :, tapidx].permute(1, 2, 0).contiguous()          # [C][T][O]
            g = (B, Ho, Wo, Hv, Wv, 1, 1, [(cy + p - a) // 2 for a, _ in taps], [(cx + p - b_) // 2 for _, b_ in taps], H, W, 2, 2, cy, cx)
            L = _launch(A=_lay(gy), lda=O, C=O, T=len(taps), Wp=Wd, N=C, M=B * Hv * Wv, out=dxo, ldo=C, mode=1, geom=g,
                        residual=dxo if k == 1 else None, ldr=C if k == 1 else 0)
            res0 = dxo.clone() if k == 1 else None
            ref, _ = emulate(dict(L, residual=res0))
            before = GC.flat(dxo).clone()
            GC.flat(dxo).copy_(ref.to(DT))
            r = GC.check_forward(L, GC.flat(dxo), before, GC.TAU['fp32'], residual=res0)
            assert r['bad'] == 0 and r['wild'] == 0, r
    want = dx + (add if k == 1 else 0)
    assert float((dxo.permute(0, 3, 1, 2).double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


def _table(M, H, T, alias_frac=0.2, seed=1):
    g = torch.Generator().manual_seed(seed)
    tab = torch.randint(-1, H, (M, 16), generator=g, dtype=torch.int32)
    bits = (torch.rand((M, T), generator=g) < alias_frac).to(torch.int64)
    tab[:, 15] = (bits << torch.arange(T)).sum(1).to(torch.int32)
    return tab, bits.bool()


def test_table_mode_vs_index_select():
    """mode 2: row = table[m*16 + t], -1 reads zeros, with table_alias_mask the taps marked in column 15 read zeros; the split-K form
    of ops._blur_gemm_ksplit (nbatch problems over batch_stride_table columns) adds up to the same product"""
    H, M, T, C, N = 50, 37, 15, 8, 12
    A = torch.randn(H, C, dtype=DT)
    tab, alias = _table(M, H, T)
    Wp = torch.randn(N, T * C, dtype=DT)
    idx = tab[:, :T].long()
    X = torch.where((idx >= 0)[..., None], A.double().index_select(0, idx.clamp_min(0).reshape(-1)).view(M, T, C), torch.zeros(()))
    for masked in (False, True):
        Xm = torch.where((masked & alias)[..., None], torch.zeros(()), X)
        want = Xm.reshape(M, -1) @ Wp.double().t()
        out = torch.zeros((M, N), dtype=DT)
        L = _launch(A=A, lda=C, C=C, T=T, Wp=Wp, N=N, M=M, out=out, ldo=N, mode=2, table=tab, alias_mask=masked)
        got, _ = emulate(L)
        assert torch.allclose(got.view(M, N), want, rtol=1e-12, atol=1e-12)
        S, Ts = 5, 3
        Wg = Wp.view(N, S, Ts * C).permute(1, 0, 2).contiguous()
        part = torch.zeros((S, M, N), dtype=DT)
        Lk = _launch(A=A, lda=C, C=C, T=Ts, Wp=Wg, N=N, M=M, out=part, ldo=N, mode=2, table=tab, alias_mask=masked,
                     batch=(S, 0, N * Ts * C, M * N, Ts))
        got, _ = emulate(Lk)
        assert torch.allclose(got.view(S, M, N).sum(0), want, rtol=1e-12, atol=1e-12)


def test_batched_planes_and_row_stack():
    """nbatch > 1 in mode 0 (the 36 planes of a 2-D Winograd layer: tile-major rows, batch strides C / N*C / N), and mode 3 (row
    stack of the correlation head: tap t = image row t, C floats from pixel j)"""
    R, C, N, P = 10, 8, 12, 6
    A3 = torch.randn(R, P, C, dtype=DT)
    W3 = torch.randn(P, N, C, dtype=DT)
    out = torch.zeros((R, P, N), dtype=DT)
    L = _launch(A=A3, lda=P * C, C=C, T=1, Wp=W3, N=N, M=R, out=out, ldo=P * N, mode=0, batch=(P, C, N * C, N))
    got, _ = emulate(L)
    want = torch.einsum('rpc,pnc->rpn', A3.double(), W3.double())
    assert torch.allclose(got.view(R, P, N), want, rtol=1e-12, atol=1e-12)
    B, Hin, Win, Wv, ld, Cs = 2, 3, 9, 5, 4, 12           # window of Cs = 3 pixels x 4 channels
    img = torch.randn(B, Hin, Win, ld, dtype=DT)
    Wc = torch.randn(N, Hin * Cs, dtype=DT)
    out = torch.zeros((B * Wv, N), dtype=DT)
    L = _launch(A=img, lda=ld, C=Cs, T=Hin, Wp=Wc, N=N, M=B * Wv, out=out, ldo=N, mode=3, geom=(B, Hin, Win, 1, Wv) + (0,) * 10)
    got, _ = emulate(L)
    win = torch.stack([img[:, :, j:j + 3, :].reshape(B, -1) for j in range(Wv)], 1).double()      # [B][Wv][Hin*Cs]
    assert torch.allclose(got.view(B, Wv, N), win @ Wc.double().t(), rtol=1e-12, atol=1e-12)


def test_lazy_operand_and_pooled_epilogues():
    """lazy: A is raw and the launch reads act(A*scale + shift) (padding stays zero); pool=True the 2x2 max, pool='h' the
    horizontal half [B][Ho][Wo/2][ldo] of the epilogue result"""
    B, H, W, C, N = 1, 6, 7, 8, 8
    x = torch.randn(B, C, H, W, dtype=torch.float64)
    w = torch.randn(N, C, 3, 3, dtype=torch.float64)
    sc, sh = torch.rand(C, dtype=DT) + 0.5, torch.randn(C, dtype=DT)

    class Lazy:
        scale, shift, act, slope = sc, sh, 1, 0.0
    geom = (B, H, W, H, W, 1, 1, [t // 3 - 1 for t in range(9)], [t % 3 - 1 for t in range(9)], H, W, 1, 1, 0, 0)
    xa = F.relu(x.to(DT).double() * sc.double()[:, None, None] + sh.double()[:, None, None])
    full = F.conv2d(xa, w.to(DT).double(), padding=1)
    for pool, want in ((False, full), (True, F.max_pool2d(full, 2)), ('h', F.max_pool2d(full, (1, 2)))):
        Ho, Wo = want.shape[2], want.shape[3]
        out = torch.zeros((B, Ho, Wo, N), dtype=DT)
        L = _launch(A=_lay(x), lda=C, C=C, T=9, Wp=_pack_conv(w.to(DT)), N=N, M=B * H * W, out=out, ldo=N, mode=1, geom=geom,
                    lazy=Lazy, pool=pool)
        before = GC.flat(out).clone()
        GC.flat(out).copy_(_lay(want).reshape(-1))
        r = GC.check_forward(L, GC.flat(out), before, GC.TAU['fp32'])
        assert r['bad'] == 0 and r['wild'] == 0, (pool, r)
        GC.flat(out)[N + 1] += 1e-3 * float(want.abs().max())
        assert GC.check_forward(L, GC.flat(out), before, GC.TAU['fp32'])['bad'] == 1, pool


@pytest.mark.parametrize('case', sorted(CONV_CASES) + ['convT', 'table'])
def test_weight_gradient_vs_autograd(case):
    """dW[n][t*C + c] = sum_m G[orow(m)][n] * A[row(m,t)][c] against torch.autograd.grad in float64, both through the packed dWp and
    through the caller's layout of the out descriptor (+= when it accumulates)"""
    B, H, W, C, N = 2, 9, 11, 8, 12
    if case == 'table':
        Hn, M, T = 40, 33, 15
        A = torch.randn(Hn, C, dtype=DT)
        tab, _ = _table(M, Hn, T)
        Wp = torch.randn(N, T * C, dtype=torch.float64, requires_grad=True)
        idx = tab[:, :T].long()
        X = torch.where((idx >= 0)[..., None], A.double().index_select(0, idx.clamp_min(0).reshape(-1)).view(M, T, C), torch.zeros(()))
        y = X.reshape(M, -1) @ Wp.t()
        G = torch.randn(M, N, dtype=DT)
        (want,) = torch.autograd.grad(y, Wp, G.double())
        Ls = [(dict(A=A, lda=C, C=C, T=T, N=N, M=M, G=G, ldg=N, mode=2, table=tab, geom=None), want.view(N, T, C))]
    elif case == 'convT':
        x = torch.randn(B, C, 4, 5, dtype=torch.float64)
        w = torch.randn(C, N, 3, 3, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose2d(x.to(DT).double(), w, stride=2, padding=1, output_padding=1)
        G = torch.randn_like(y).to(DT)
        (want,) = torch.autograd.grad(y, w, G.double())                         # (C, N, 3, 3)
        Ls = []
        outs, _, _ = _convt_launches(_lay(x), w.detach(), 1, 1, torch.zeros(1), N)
        for L in outs:
            cy, cx = L['geom'][13], L['geom'][14]
            tapidx = [a * 3 + b_ for a in range(3) if (cy + 1 - a) % 2 == 0 for b_ in range(3) if (cx + 1 - b_) % 2 == 0]
            Ls.append((dict(A=L['A'], lda=C, C=C, T=L['T'], N=N, M=L['M'], G=_lay(G), ldg=N, mode=1, table=None, geom=L['geom']),
                       want.reshape(C, N, 9)[:, :, tapidx].permute(1, 2, 0)))
    else:
        kh, kw, s, p = CONV_CASES[case]
        x = torch.randn(B, C, H, W, dtype=torch.float64)
        w = torch.randn(N, C, kh, kw, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x.to(DT).double(), w, stride=s, padding=p)
        G = torch.randn_like(y).to(DT)
        (want,) = torch.autograd.grad(y, w, G.double())
        Ho, Wo = y.shape[2], y.shape[3]
        T = kh * kw
        geom = (B, H, W, Ho, Wo, s, s, [i // kw - p for i in range(T)], [i % kw - p for i in range(T)], Ho, Wo, 1, 1, 0, 0)
        Ls = [(dict(A=_lay(x), lda=C, C=C, T=T, N=N, M=B * Ho * Wo, G=_lay(G), ldg=N, mode=1, table=None, geom=geom),
               want.reshape(N, C, T).permute(0, 2, 1))]
    for L, want in Ls:
        ref, S = GC.wgrad_ref(dict(L, lazy=None))
        assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max() + 1)
        dWp = ref.to(DT).contiguous()
        r = GC.check_wgrad(dict(L, dWp=dWp, lazy=None), False, GC.TAU['fp32'])
        assert r['bad'] == 0, r
        # the caller's layout: W[n*sn + c*sc + taps[t]*st], accumulating into a buffer with one spare element at each end
        Nn, T, Cc = want.shape
        buf = torch.randn(Nn * Cc * T + 2, dtype=DT)
        dW = buf[1:-1]
        before = buf.clone()[1:-1]
        up = (dW, Nn, T, Cc, Cc, Cc * T, T, 1, list(range(T)), True)
        dW.view(Nn, Cc, T).add_(ref.permute(0, 2, 1).to(DT))
        r = GC.check_wgrad(dict(L, dWp=None, unpack=up, lazy=None), True, GC.TAU['fp32'], dW_before=before)
        assert r['bad'] == 0 and r['wild'] == 0, r


# --------------------------------------------------------------------------------------------------- sensitivity
# the largest K = T*C each family meets in the model (tests/test_gpu_launch_contract.py prints them with its summary)
FAMILY_K = {
    'fp32': (15, 448),           # K = 6720
    'wino1d': (9, 512),          # K = 4608
    'wino2d': (9, 512),
    'wino2d_split': (9, 512),
}


def _fault_case(T, C, N=72, H=7, W=9, B=1, seed=0):
    """a same-size 3x3 launch (T = 9) or a 15-tap table launch, ReLU-like non-negative inputs as the model's, signed weights"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, H, W, C), generator=g, dtype=DT)
    Wp = (torch.randn((N, T * C), generator=g) / (T * C) ** 0.5).to(DT)
    ldo, co = N + 8, 4
    out = torch.zeros((B, H, W, ldo), dtype=DT)
    if T == 9:
        geom = (B, H, W, H, W, 1, 1, [t // 3 - 1 for t in range(9)], [t % 3 - 1 for t in range(9)], H, W, 1, 1, 0, 0)
        L = _launch(A=x, lda=C, C=C, T=9, Wp=Wp, N=N, M=B * H * W, out=out, ldo=ldo, mode=1, geom=geom, out_off=co)
    else:
        tab, _ = _table(B * H * W, B * H * W, T, alias_frac=0.0, seed=seed)
        tab[:, :T] = tab[:, :T].abs()
        L = _launch(A=x.view(-1, C), lda=C, C=C, T=T, Wp=Wp, N=N, M=B * H * W, out=out, ldo=ldo, mode=2, table=tab, out_off=co)
    return L


def _rejects(L, got, before, tau):
    r = GC.check_forward(L, got, before, tau)
    return r['bad'] > 0 or r['wild'] > 0


@pytest.mark.parametrize('family', sorted(FAMILY_K))
def test_checker_rejects_forward_faults(family):
    """each fault applied to the float64 result of a correct launch, at the family's largest K and tau: the checker rejects it"""
    T, C = FAMILY_K[family]
    tau = GC.TAU[family]
    L = _fault_case(T, C)
    before = GC.flat(L['out']).clone()
    ref, _ = emulate(L)
    good = ref.to(DT)
    assert not _rejects(L, good, before, tau)                           # the honest result passes
    M, N = L['M'], L['N']
    rows = GC.out_index(L, GC.out_rows(L, torch.arange(M)))             # [M][N] offsets
    faults = {}
    # a tap dropped from one output row
    m = M // 2
    X, _ = GC.gather_a(L, torch.tensor([m]))
    X.view(T, C)[4] = 0
    g = good.clone()
    g[rows[m]] = (X @ GC.weight_rows(L).t()).view(-1).to(DT)
    faults['tap dropped'] = g
    # the last output row, and the last partial column block (N = 72: columns 64..71), left unwritten
    g = good.clone()
    g[rows[-1]] = before[rows[-1]]
    faults['last row unwritten'] = g
    g = good.clone()
    g[rows[:, 64:]] = before[rows[:, 64:]]
    faults['last column block unwritten'] = g
    # the whole output placed one pixel further on
    g = before.clone()
    g[rows[1:]] = good[rows[:-1]]
    faults['placement shifted'] = g
    # two input channels swapped
    A2 = L['A'].clone()
    A2[..., [1, C - 2]] = A2[..., [C - 2, 1]]
    g, _ = emulate(dict(L, A=A2))
    faults['channels swapped'] = g.to(DT)
    # one element written into a column of the destination outside [out_off, out_off + N)
    g = good.clone()
    g[rows[M // 3, 0] - 1] = 1.0
    faults['write outside the columns'] = g
    missed = [k for k, g in faults.items() if not _rejects(L, g, before, tau)]
    assert not missed, (family, missed)


@pytest.mark.parametrize('family', sorted(FAMILY_K))
def test_checker_rejects_wgrad_missing_rows(family):
    """weight gradient at M ~ 5000 with the last 32 rows of M missing from the sum: rejected at the family's largest K and tau"""
    T, C = FAMILY_K[family]
    L = _fault_case(T, C, N=64, H=50, W=100)
    M = L['M']
    assert 4900 <= M <= 5100
    g = torch.Generator().manual_seed(3)
    G = torch.randn((M, 64), generator=g, dtype=DT)
    W = dict(A=L['A'], lda=C, C=C, T=T, N=64, M=M, G=G, ldg=64, mode=L['mode'], geom=L['geom'], table=L['table'], lazy=None)
    rows = family == 'wino1d'                  # (the scale the GPU test gives that family's weight gradients)
    ref, _ = GC.wgrad_ref(W)
    assert GC.check_wgrad(dict(W, dWp=ref.to(DT).contiguous()), False, GC.TAU[family], rows=rows)['bad'] == 0
    short, _ = GC.wgrad_ref(dict(W, M=M - 32))
    assert GC.check_wgrad(dict(W, dWp=short.to(DT).contiguous()), False, GC.TAU[family], rows=rows)['bad'] > 0


# --------------------------------------------------------------------------------------------------- dispatch predicates
def _lib():
    from efgh_amd import _C
    if not os.path.exists(_C.SO_PATH):
        pytest.fail('libefgh_hip.so is not built: run __graft_entry__.build() first')
    return _C


def _geoms():
    """3x3 / pad 1 at stride 1 and 2, 1x1 at stride 1, sizes below 8, odd and even"""
    for H, W in ((1, 1), (3, 5), (4, 4), (7, 9), (8, 8), (13, 16), (16, 11)):
        for s in (1, 2):
            Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
            yield (1, H, W, Ho, Wo, s, s, [t // 3 - 1 for t in range(9)], [t % 3 - 1 for t in range(9)], Ho, Wo, 1, 1, 0, 0)
        yield (2, H, W, H, W, 1, 1, [0], [0], H, W, 1, 1, 0, 0)


def _desc(_C, C, N, geom):
    d = _C.GemmDesc()
    d.A, d.W, d.out = 256, 512, 1024                 # 16-byte aligned dummies: nothing is launched
    d.lda, d.C, d.T, d.mode, d.N, d.ldo = ((C + 3) // 4) * 4, C, len(geom[7]), 1, N, ((N + 3) // 4) * 4
    (d.B, d.Hin, d.Win, d.Hv, d.Wv, d.sh, d.sw, dh, dw, d.Ho, d.Wo, d.osh, d.osw, d.oh0, d.ow0) = geom
    for i, (a, b) in enumerate(zip(dh, dw)):
        d.dh[i], d.dw[i] = a, b
    d.M = geom[0] * geom[3] * geom[4]
    return d


def test_dispatch_predicates_mirror_the_library(monkeypatch):
    """over a grid of descriptors every Python *_eligible that ops.gemm_route / wgrad_route decide on, and the family they name,
    implies the C predicate of the kernel it routes to (Python never routes a launch the kernel refuses); those whose docstring claims a mirror are equal
    to it once the Python-only thresholds are 0 (WINO2D_MIN_C*, SC_MIN_PIXELS_32).  The 2-D Winograd form is a mirror only where
    the model can use it: maps of at least 8 x 8 and >= 64 channels on both sides (below, wino2d_eligible inherits the 1-D form's
    C % 16 / N % 64 and the map-size floor, which efgh_wino2d_supported does not ask for - stricter, never looser)"""
    from efgh_amd import ops
    _C = _lib()
    lib = _C.lib()
    by = ctypes.byref
    chans = (1, 2, 3, 4, 16, 32, 64, 128, 256, 512)
    FWD = {'thin': 'efgh_thin_supported', 'c4': 'efgh_c4_supported', 'sc': 'efgh_sc_supported', 'wino2d': 'efgh_wino2d_supported',
           'wino': 'efgh_wino_supported'}
    WGRAD = {'sc_c4': 'efgh_sc_wgrad_supported', 'sc': 'efgh_sc_wgrad_supported', 'c4': 'efgh_c4_wgrad_supported',
             'wino2d': 'efgh_wino2d_supported', 'wino': 'efgh_wino_supported'}
    for thr in (False, True):
        if thr:
            for k in ('WINO2D_MIN_C', 'WINO2D_MIN_C_WGRAD', 'WINO2D_MIN_C_TRAIN', 'SC_MIN_PIXELS_32'):
                monkeypatch.setattr(ops, k, 0)
        bad = []
        for C, N, geom in itertools.product(chans, chans, list(_geoms())):
            d = _desc(_C, C, N, geom)
            T = len(geom[7])
            w2d_exact = geom[1] >= 8 and geom[2] >= 8 and min(C, N) >= 64
            fwd, wg = ops.gemm_route(1, C, N, T, geom, d.M), ops.wgrad_route(1, C, N, T, geom)
            pairs = [
                ('wino', ops.wino_eligible(1, C, N, geom), lib.efgh_wino_supported(by(d)), True),
                ('wino2d', ops.wino2d_eligible(1, C, N, geom), lib.efgh_wino2d_supported(by(d)), w2d_exact),
                ('wino2d wgrad', ops.wino2d_eligible(1, C, N, geom, wgrad=True), lib.efgh_wino2d_supported(by(d)), w2d_exact),
                ('c4', ops.c4_eligible(1, C, N, geom), lib.efgh_c4_supported(by(d)), True),
                ('c4 wgrad', ops.c4_eligible(1, C, N, geom, wgrad=True), lib.efgh_c4_wgrad_supported(by(d)), True),
                ('sc', ops.sc_eligible(1, C, N, geom), lib.efgh_sc_supported(by(d)), True),
                # (the weight-gradient route also sends the 4-channel input layers at stride 1 to efgh_sc_wgrad: 'sc_c4')
                ('sc wgrad', wg in ('sc', 'sc_c4'), lib.efgh_sc_wgrad_supported(by(d)), True),
                ('thin', ops.thin_eligible(1, C, N, T), lib.efgh_thin_supported(by(d)), False),
            ]
            # the family each route names implies the C predicate of the kernel that serves it
            if fwd in FWD:
                pairs.append(('route ' + fwd, True, getattr(lib, FWD[fwd])(by(d)), False))
            if wg in WGRAD:
                pairs.append(('wgrad route ' + wg, True, getattr(lib, WGRAD[wg])(by(d)), False))
            pf = ops.pool_fusable(1, C, N, geom)
            if pf is True and fwd == 'c4':
                pairs.append(('c4 pooled', True, lib.efgh_c4_pooled_supported(by(d)), False))
            elif pf is True:
                pairs.append(('wino2d pooled', fwd == 'wino2d', lib.efgh_wino2d_supported(by(d)), False))
            elif pf == 'h':
                pairs.append(('wino hpool', True, lib.efgh_wino_supported(by(d)), False))
            for name, py, c, exact in pairs:
                if (py and not c) or (thr and exact and bool(py) != bool(c)):
                    bad.append((name, C, N, geom[1:7], T, bool(py), int(c)))
        assert not bad, (sorted({b[0] for b in bad}), bad[:20])
