"""The float64 contract of tests/w2_contract.py, checked on the CPU before it meets a kernel:
(1) its matrices are right by mathematics: in float64 the transforms chained into A^T [U .* V] A equal a direct 3x3 / pad-1 correlation
    and A3^T [sum_t Gy .* V] A3 equals torch.nn.grad.conv2d_weight, to 1e-12, at H, W in {1, 4, 5, 9};
(2) an fp32 emulation of each of the five kernels (the same order of operations, no contraction, fp32 where the kernel computes in
    fp32 and float64 where it computes in float64) passes the contract on the cases of the GPU module - the ceilings are reachable by
    a correct implementation; its worst |got - ref| / S per class is printed by the last test;
(3) each of nine faults planted into the emulation is caught by the same comparison at a shape of the GPU module's case list.

Worst ratio of the emulation (x 2^-24): V 3.43 of a ceiling of 8, V of input_act 2.84 / 10, Gy of efgh_wino2d_dy 3.98 / 10,
Vd 5.23 / 9, Gy of the fused forms 5.12 / 11."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_contract as BC
import w2_contract as W2
from bn_contract import ACT_LEAKY, ACT_NONE, ACT_RELU, outside_unchanged, view2

REL = 1e-12
HW = [1, 4, 5, 9]
EMU = {}                 # class -> (largest |got - ref| / S of the emulation, its case)
SENT = -7777.0


# ------------------------------------------------------------------------------------------------ (1) the mathematics
def _close(got, want, what):
    err = float((got - want).abs().max())
    assert err <= REL * (float(want.abs().max()) + 1e-300), (what, err)


@pytest.mark.parametrize('H', HW)
@pytest.mark.parametrize('W', HW)
def test_transforms_chain_into_the_convolution_and_its_weight_gradient(H, W):
    B, C, N = 2, 3, 5
    g = torch.Generator().manual_seed(100 * H + W)
    x = torch.randn((B, H, W, C), generator=g, dtype=torch.float64)
    w = torch.randn((N, C, 3, 3), generator=g, dtype=torch.float64)
    gy = torch.randn((B, H, W, N), generator=g, dtype=torch.float64)
    TH, TW, T = W2.geo(B, H, W)
    V, _ = W2.input_ref(x)                                                   # [T][36][C]
    Uw = torch.einsum('ik,nckl,jl->ijnc', W2.G3, w, W2.G3).reshape(36, N, C)
    M = torch.einsum('tac,anc->tan', V, Uw).view(B, TH, TW, 6, 6, N)
    y = torch.einsum('ik,bytkln,jl->byitjn', W2.AT4, M, W2.AT4).reshape(B, 4 * TH, 4 * TW, N)[:, :H, :W]
    _close(y, F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1), 'forward')
    Gy, _ = W2.dy_ref(gy)                                                    # [T][36][N]
    S = torch.einsum('tan,tac->anc', Gy, V).view(6, 6, N, C)
    dW = torch.einsum('ik,klnc,jl->ncij', W2.AT3, S, W2.AT3)
    want = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), w.shape, gy.permute(0, 3, 1, 2), padding=1)
    _close(dW, want, 'weight gradient')


def test_geometry_of_the_non_temporal_cases():
    assert W2.geo(2, 5, 9) == (2, 3, 12) and W2.tiles_of((1, 1, 2), 5, 9) == (9, 12) and W2.rows_of((1, 1, 2), 5) == (4, 5)
    assert W2.nt_bytes(*W2.NT_BELOW, W2.NT_N) < BC.NT_BYTES <= W2.nt_bytes(*W2.NT_ABOVE, W2.NT_N)
    chunks = W2.tile_row_chunks(*W2.NT_BELOW, W2.NT_N)
    assert len(chunks) > 1 and chunks[0][1] == 0 and chunks[-1][2] == 170
    assert all(c[2] == d[1] for c, d in zip(chunks, chunks[1:]))


# ------------------------------------------------------------------------------------------------ (2) the fp32 emulation
A_, B_, A2, B2, A2B2, SUM, A3, B3 = 0.75, 1.5, 0.5625, 2.25, 1.265625, 2.8125, 0.421875, 3.375       # (all fp32 numbers)
F0 = float(np.float32(1.0) / np.float32(1.265625))
FA = float(np.float32(-128.0) / np.float32(243.0))
FB = float(np.float32(32.0) / np.float32(243.0))


def bt6(d):
    t1, s1 = d[4] - B2 * d[2], A_ * (d[3] - B2 * d[1])
    t3, s3 = d[4] - A2 * d[2], B_ * (d[3] - A2 * d[1])
    return [A2B2 * d[0] - SUM * d[2] + d[4], t1 + s1, t1 - s1, t3 + s3, t3 - s3, A2B2 * d[1] - SUM * d[3] + d[5]]


def g46(g):
    pa, qa = g[0] + A2 * g[2], A_ * g[1] + A3 * g[3]
    pb, qb = g[0] + B2 * g[2], B_ * g[1] + B3 * g[3]
    return [F0 * g[0], (pa + qa) * FA, (pa - qa) * FA, (pb + qb) * FB, (pb - qb) * FB, g[3]]


def windows32(x):
    """x [B][H][W][C] fp32 -> (the 6x6 windows [B][TH][TW][6][6][C] read at clamped coordinates, ok [TH][TW][6][6][1]: in the image)"""
    B, H, W, C = x.shape
    TH, TW, _ = W2.geo(B, H, W)
    ys = 4 * torch.arange(TH)[:, None] - 1 + torch.arange(6)[None, :]
    xs = 4 * torch.arange(TW)[:, None] - 1 + torch.arange(6)[None, :]
    yc, xc = ys.clamp(0, H - 1), xs.clamp(0, W - 1)
    win = x[:, yc[:, None, :, None], xc[None, :, None, :]]
    ok = ((ys >= 0) & (ys < H))[:, None, :, None] & ((xs >= 0) & (xs < W))[None, :, None, :]
    return win, ok.unsqueeze(-1)


def scatter_tiles(planes, B, H, W, fault):
    """planes [B][TH][TW][6][6][C] -> [T][36][C] at t = (b*TH + ty)*TW + tx (fault tile_stride: ... *(W/4) + tx, into a sentinel-filled T)"""
    TH, TW, T = W2.geo(B, H, W)
    C = planes.shape[-1]
    flat = planes.reshape(T, 36, C)
    if fault != 'tile_stride':
        return flat
    out = torch.full((T, 36, C), SENT)
    for b in range(B):
        for ty in range(TH):
            for tx in range(TW):
                out[(b * TH + ty) * (W // 4) + tx] = planes[b, ty, tx].reshape(36, C)
    return out


def two_pass_bt(win):
    w = torch.stack(bt6([win[..., :, k, :] for k in range(6)]), dim=-2)              # along x
    return torch.stack(bt6([w[..., r, :, :] for r in range(6)]), dim=-3)             # along y


def two_pass_g4(win, fault=None):
    r0 = 0 if fault == 'gy_rows' else 1
    w = torch.stack(g46([win[..., r0:r0 + 4, 1 + k, :] for k in range(4)]), dim=-2)  # [..][4][6][C]
    return torch.stack(g46([w[..., r, :, :] for r in range(4)]), dim=-3)


def fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()        # (the product of two fp32 numbers is exact in float64)


def emu_input(A, fault=None, affine=None):
    """k_w2_input: affine = (scale, shift, act, slope) for the _act form"""
    B, H, W, C = A.shape
    win, ok = windows32(A)
    zero = torch.zeros((), dtype=torch.float32)
    if affine is None:
        win = win if fault == 'clamped' else torch.where(ok, win, zero)
    else:
        sc, sf, a, slope = affine
        neg = 0.0 if a == ACT_RELU else (BC.f32(slope) if a == ACT_LEAKY else 1.0)
        if fault == 'act_shift':
            win = torch.where(ok, win, zero)                     # a zero tap that then goes through the activation: act(shift)
        v = fma32(win, sc, sf)
        v = v.clamp_min(0) + neg * v.clamp_max(0)
        win = v if fault in ('act_shift', 'clamped') else torch.where(ok, v, zero)
    return scatter_tiles(two_pass_bt(win), B, H, W, fault)


def emu_dy(G, fault=None):
    B, H, W, N = G.shape
    win, ok = windows32(G)
    win = win if fault == 'clamped' else torch.where(ok, win, torch.zeros((), dtype=torch.float32))
    return scatter_tiles(two_pass_g4(win, fault), B, H, W, fault)


def _draw32(raw, gv, p, m1, m2):
    cf, inv, mu = p['scale'].double(), p['invstd'].double(), p['mean'].double()
    Ad = cf * inv * m2
    Bd = cf * m1 - Ad * mu
    return (-raw.double() * Ad + (cf * gv.double() - Bd)).float()


def _fused_store(draw, B, H, W, fault):
    win, ok = windows32(draw)
    win = win if fault == 'clamped' else torch.where(ok, win, torch.zeros((), dtype=torch.float32))
    return scatter_tiles(two_pass_bt(win), B, H, W, fault), scatter_tiles(two_pass_g4(win, fault), B, H, W, fault)


def emu_bwd(c, geom, a, slope, src, fault=None, lddres=None, off=8):
    """k_w2_bwd -> (Vd, Gy, the dres buffer: rows of pitch lddres from element `off`, two guard rows behind)"""
    B, H, W = geom
    p = c['p']
    N = c['raw'].shape[-1]
    raw, dy = c['raw'].view(B, H, W, N), c['dy'].view(B, H, W, N)
    pos = c['pos'].view(B, H, W, N) if src == 'bits' else fma32(raw, p['scale'], p['shift']) > 0
    if fault == 'mask_x1':
        pos = pos[:, :, (torch.arange(W) + 1).clamp(max=W - 1)]
    if fault == 'mask_c32':
        pos = pos[..., torch.arange(N) ^ 32]
    negd = 0.0 if a == ACT_RELU else (BC.f32(slope) if a == ACT_LEAKY else 1.0)
    gv = dy * torch.where(pos, torch.ones(()), torch.full((), negd))
    Vd, Gy = _fused_store(_draw32(raw, gv, p, c['m1'], c['m2']), B, H, W, fault)
    lddres = lddres or N + 8
    M = B * H * W
    buf = torch.full((off + (M + 2) * lddres,), SENT)
    view2(buf, off, lddres, M, N).copy_(gv.view(M, N))
    if fault == 'dres_oob' and W % 4:
        # the last tile of the last row writes its out-of-image column x = W: pixel index (b*H + y)*W + W, one past the last pixel
        view2(buf, off, lddres, M + 1, N)[M] = gv[B - 1, H - 1, W - 1]
    return Vd, Gy, buf


def emu_bwd_pool(c, geom, a, slope, fault=None):
    B, H, W = geom
    p = c['p']
    raw, dyp = c['raw'], c['dy_pool']
    Ho, Wo = H // 2, W // 2
    nega = 0.0 if a == ACT_RELU else (BC.f32(slope) if a == ACT_LEAKY else 1.0)
    tt = fma32(raw, p['scale'], p['shift'])
    e = tt.clamp_min(0) + nega * tt.clamp_max(0)
    e4, t4 = BC.windows(e), BC.windows(tt)
    if fault == 'last_max':
        best, cur = torch.zeros(e4.shape[1:], dtype=torch.int64), e4[0]
        for q in (1, 2, 3):
            ge = e4[q] >= cur
            best, cur = torch.where(ge, torch.full_like(best, q), best), torch.where(ge, e4[q], cur)
    else:
        best, _ = BC.first_max(e4)
    d4 = torch.where(t4 > 0, torch.ones(()), torch.full((), nega))
    gv = BC.unwindows(torch.where(BC.one_hot_window(best), dyp.unsqueeze(0) * d4, torch.zeros(())), H, W)
    if fault == 'rim_pooled':
        yy, xx = (torch.arange(H) // 2).clamp(max=Ho - 1), (torch.arange(W) // 2).clamp(max=Wo - 1)
        rim = ((torch.arange(H) >= 2 * Ho)[:, None] | (torch.arange(W) >= 2 * Wo)[None, :])[None, :, :, None]
        gv = torch.where(rim, dyp[:, yy[:, None], xx[None, :]], gv)
    return _fused_store(_draw32(raw, gv, p, c['m1'], c['m2']), B, H, W, fault)


# ------------------------------------------------------------------------------------------------ the comparison
def bad_plain(c, geom, a, slope, src, want_dres, fault=None, table=None):
    """elements of the emulated efgh_wino2d_bwd_transforms outside the contract (Vd, Gy, dres, the write set of dres)"""
    table = {} if table is None else table
    B, H, W = geom
    p = c['p']
    N = c['raw'].shape[-1]
    raw, dy = c['raw'].view(B, H, W, N), c['dy'].view(B, H, W, N)
    lab = 'emulation %s N %d act %d slope %g %s' % ('x'.join(map(str, geom)), N, a, slope, src)
    Vd, Gy, buf = emu_bwd(c, geom, a, slope, src, fault)
    before = torch.full_like(buf, SENT)
    dres4 = view2(buf, 8, N + 8, B * H * W, N).view(B, H, W, N)
    pos = c['pos'].view(B, H, W, N) if src == 'bits' else None
    n = 0
    for ch in W2.tile_row_chunks(B, H, W, N):
        ref = W2.bwd_transforms_ref(dy, raw, pos, p['scale'], p['shift'], p['mean'], p['invstd'], p['scale'], c['m1'], c['m2'], a, slope, ch)
        n += W2.check_tiles('vd', lab, Vd, ref['Vd'], ref['S_Vd'], ch, H, W, table=table)
        n += W2.check_tiles('gyd', lab, Gy, ref['Gy'], ref['S_Gy'], ch, H, W, table=table)
        if want_dres:
            n += W2.check_dres(lab, dres4, ref, ch, H)
    if want_dres:
        n += outside_unchanged(buf, before, 8, N + 8, B * H * W, N)
    return n


def bad_pooled(c, geom, a, slope, fault=None, table=None):
    table = {} if table is None else table
    B, H, W = geom
    p = c['p']
    N = c['raw'].shape[-1]
    lab = 'emulation pooled %s N %d act %d slope %g' % ('x'.join(map(str, geom)), N, a, slope)
    Vd, Gy = emu_bwd_pool(c, geom, a, slope, fault)
    n = 0
    for ch in W2.tile_row_chunks(B, H, W, N):
        ref = W2.bwd_transforms_pooled_ref(c['dy_pool'], c['raw'], p['scale'], p['shift'], p['mean'], p['invstd'], p['scale'], c['m1'],
                                           c['m2'], a, slope, ch)
        n += W2.check_tiles('vd', lab, Vd, ref['Vd'], ref['S_Vd'], ch, H, W, table=table)
        n += W2.check_tiles('gyd', lab, Gy, ref['Gy'], ref['S_Gy'], ch, H, W, table=table)
    return n


def bad_input(geom, C, a, slope, fault=None, table=None, which=('v', 'v_act', 'gy')):
    table = {} if table is None else table
    B, H, W = geom
    c = BC.gen_rows(B * H * W, C, W2.case_seed(geom, C, a, slope), 'cpu', a, slope)
    p = c['p']
    A, G = c['raw'].view(B, H, W, C), c['dy'].view(B, H, W, C)
    lab = 'emulation %s C %d act %d slope %g' % ('x'.join(map(str, geom)), C, a, slope)
    n = 0
    if 'v' in which:
        n += W2.cmp('v', lab, emu_input(A, fault), *W2.input_ref(A), table=table)
    if 'v_act' in which:
        n += W2.cmp('v_act', lab, emu_input(A, fault, (p['scale'], p['shift'], a, slope)),
                    *W2.input_act_ref(A, p['scale'], p['shift'], a, slope), table=table)
    if 'gy' in which:
        n += W2.cmp('gy', lab, emu_dy(G, fault), *W2.dy_ref(G), table=table)
    return n


@pytest.mark.parametrize('geom', W2.GEOMS, ids=lambda g: 'x'.join(map(str, g)))
def test_emulation_of_the_fused_kernels_passes(geom):
    for a, slope in W2.ACTS:
        c = W2.gen_plain(geom, 64, a, slope, 'cpu')
        assert c['ambiguous'] == 0
        for src in ('bits', 'affine'):
            assert bad_plain(c, geom, a, slope, src, True, table=EMU) == 0, (geom, a, slope, src)
        if geom in W2.POOL_GEOMS:
            c = W2.gen_pooled(geom, 64, a, slope, 'cpu', ties=geom == W2.POOL_TIES)
            assert c['ambiguous'] == 0
            assert bad_pooled(c, geom, a, slope, table=EMU) == 0, (geom, a, slope)


@pytest.mark.parametrize('geom', W2.GEOMS, ids=lambda g: 'x'.join(map(str, g)))
def test_emulation_of_the_plain_transforms_passes(geom):
    for C in (4, 64):
        for a, slope in W2.ACTS:
            assert bad_input(geom, C, a, slope, table=EMU) == 0, (geom, C, a, slope)


def test_emulation_at_the_other_channel_counts():
    geom = (2, 5, 9)
    a, slope = ACT_LEAKY, 0.2
    for N in (128, 512):
        c = W2.gen_plain(geom, N, a, slope, 'cpu')
        assert bad_plain(c, geom, a, slope, 'bits', True, table=EMU) == 0
        assert bad_pooled(W2.gen_pooled(geom, N, a, slope, 'cpu'), geom, a, slope, table=EMU) == 0
    assert bad_input(geom, 512, a, slope, table=EMU) == 0


# ------------------------------------------------------------------------------------------------ (3) planted faults
# fault -> (the kernel it is planted into, the shape of the GPU module's list that exposes it, activation)
FAULTS = {
    'clamped': ('plain', (2, 5, 9), (ACT_NONE, 0.0)),           # out-of-image taps left at their clamped value
    'act_shift': ('input_act', (1, 1, 1), (ACT_RELU, 0.0)),     # out-of-image taps of input_act given act(shift)
    'mask_x1': ('plain', (2, 5, 9), (ACT_RELU, 0.0)),           # the mask bit read from column x + 1
    'mask_c32': ('plain', (1, 1, 1), (ACT_RELU, 0.0)),          # the mask bit read from channel c xor 32
    'last_max': ('pooled', W2.POOL_TIES, (ACT_RELU, 0.0)),      # the last maximum on a planted tie
    'rim_pooled': ('pooled', (2, 5, 9), (ACT_NONE, 0.0)),       # the floor-pool rim given a pooled gradient
    'gy_rows': ('plain', (1, 2, 2), (ACT_NONE, 0.0)),           # Gy over window rows 0..3 instead of 1..4
    'tile_stride': ('plain', (2, 5, 9), (ACT_NONE, 0.0)),       # tile row stride W/4 (floor) instead of TW
    'dres_oob': ('plain', (2, 5, 9), (ACT_LEAKY, 0.2)),         # dres written for an out-of-image position of a partial tile
}


@pytest.mark.parametrize('fault', sorted(FAULTS))
def test_planted_fault_is_caught(fault):
    kind, geom, (a, slope) = FAULTS[fault]
    assert geom in W2.GEOMS and (kind != 'pooled' or geom in W2.POOL_GEOMS)
    if kind == 'plain':
        c = W2.gen_plain(geom, 64, a, slope, 'cpu')
        assert bad_plain(c, geom, a, slope, 'bits', True) == 0
        assert bad_plain(c, geom, a, slope, 'bits', True, fault=fault, table={}) > 0
    elif kind == 'pooled':
        c = W2.gen_pooled(geom, 64, a, slope, 'cpu', ties=geom == W2.POOL_TIES)
        assert bad_pooled(c, geom, a, slope) == 0
        assert bad_pooled(c, geom, a, slope, fault=fault, table={}) > 0
    else:
        assert bad_input(geom, 64, a, slope, which=('v_act',)) == 0
        assert bad_input(geom, 64, a, slope, fault=fault, table={}, which=('v_act',)) > 0


@pytest.mark.parametrize('fault', ['clamped', 'tile_stride'])
def test_planted_fault_is_caught_in_the_plain_transforms_too(fault):
    geom = (2, 5, 9)
    for which in ('v', 'v_act', 'gy'):
        assert bad_input(geom, 64, ACT_LEAKY, 0.2, fault=fault, table={}, which=(which,)) > 0, which
    c = W2.gen_pooled(geom, 64, ACT_LEAKY, 0.2, 'cpu')
    assert bad_pooled(c, geom, ACT_LEAKY, 0.2, fault=fault, table={}) > 0


def test_worst_ratio_of_the_emulation_is_below_every_ceiling():
    print('\nclass   emulation max |got - ref| / S      ceiling      case')
    for cls in ('v', 'v_act', 'gy', 'vd', 'gyd'):
        assert cls in EMU, 'this test sums up the module: run the module, not the test'
        v, lab = EMU[cls]
        print('%-7s %.3e (%5.2f x 2^-24)       %5.2f x 2^-24  %s' % (cls, v, v / BC.U, W2.CEIL[cls] / BC.U, lab))
        assert 0 < v <= W2.CEIL[cls] and W2.TAU_W2[cls] <= W2.CEIL[cls]
