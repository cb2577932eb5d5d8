"""The transforms of the 2-D Winograd layers against the float64 contract of tests/w2_contract.py, element by element: direct calls of
efgh_wino2d_input, efgh_wino2d_input_act, efgh_wino2d_dy, efgh_wino2d_bwd_transforms and efgh_wino2d_bwd_transforms_pooled through
the C ABI at the smallest shapes that reach each path (single partial tiles, exact multiples of 4, a last tile one pixel wide, several
images, four tiles per workgroup / two workgroups per tile), every activation, BatchNorm parameter sets that differ per channel within
one launch, both mask sources with the bits drawn independently of raw, dres absent and present, three different pitches and
non-zero offsets into sentinel-filled buffers whose other elements must stay bit-unchanged.  The fused forms are also tied to the
materialised two-pass form (efgh_act_bn_bwd_apply / efgh_pool_bn_bwd_apply -> efgh_wino2d_input + efgh_wino2d_dy), non-finite
gradients must stay inside the tiles that contain them, every entry point runs on both sides of its non-temporal switch, and the
calls the header forbids return an error and write nothing.  The last test prints the table the taus of w2_contract.TAU_W2 come from.

These are the operands of the launches tests/test_gpu_launch_contract.py records as `unchecked (pre_v / pre_gy)`."""
import ctypes

import pytest
import torch

import bn_contract as BC
import w2_contract as W2
from bn_contract import ACT_RELU, outside_unchanged, view2
from w2_contract import cmp

pytestmark = pytest.mark.gpu

SENT = -7777.0
DEV = 'cuda'
CALLS = {}               # entry point -> the byte counts its non-temporal switch saw, one per call
_NT = {}                 # generated inputs of the non-temporal cases, shared by the tests of one shape
_ids = lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731


@pytest.fixture(scope='module', autouse=True)
def release_large_inputs():
    yield
    _NT.clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ buffers and raw calls
def P(buf, off=0):
    """device pointer to element `off` of a tensor (None -> NULL)"""
    return ctypes.c_void_p(0 if buf is None else buf.data_ptr() + buf.element_size() * off)


def i32(v):
    return ctypes.c_int32(int(v))


def i64(v):
    return ctypes.c_int64(int(v))


def f32(v):
    return ctypes.c_float(float(v))


def sentinel(n, dtype=torch.float32):
    return torch.full((int(n),), SENT, dtype=dtype, device=DEV)


def place(t, ld, off, tail=2):
    """t [M][C] inside a sentinel-filled 1-D buffer: pitch ld, first element at `off`, `tail` rows behind -> (buffer, view)"""
    M, C = t.shape
    buf = sentinel(off + (M + tail) * ld)
    v = view2(buf, off, ld, M, C)
    v.copy_(t)
    return buf, v


def out_rows(M, C, ld, off, tail=2):
    buf = sentinel(off + (M + tail) * ld)
    return buf, view2(buf, off, ld, M, C)


def out_tiles(T, N, off=8):
    """a Winograd-domain output [T][36][N] at element `off` of a sentinel-filled buffer, guard zones before and after"""
    buf = sentinel(off + T * 36 * N + 64)
    return buf, buf[off:off + T * 36 * N].view(T, 36, N), off


def tiles_outside_unchanged(buf, T, N, off=8):
    a = buf.view(torch.int32)
    s = torch.tensor(SENT, dtype=torch.float32).view(torch.int32).item()
    return int((a[:off] != s).sum()) + int((a[off + T * 36 * N:] != s).sum())


def call(name, geom, N, *args):
    """one entry point through the C ABI -> its return code; the bytes the non-temporal switch of an accepted call saw are recorded"""
    from efgh_amd import ops
    rc = getattr(ops._L(), name)(*args, ops._st())
    if rc == 0:
        CALLS.setdefault(name, []).append(W2.nt_bytes(*geom, N))
    return rc


def k_input(A, aoff, lda, C, geom, V, voff):
    assert call('efgh_wino2d_input', geom, C, P(A, aoff), i64(lda), i32(C), *map(i32, geom), P(V, voff)) == 0


def k_input_act(A, aoff, lda, C, geom, scale, shift, a, slope, V, voff):
    assert call('efgh_wino2d_input_act', geom, C, P(A, aoff), i64(lda), i32(C), *map(i32, geom), P(scale), P(shift), i32(a), f32(slope),
                P(V, voff)) == 0


def k_dy(G, goff, ldg, N, geom, Gy, gyoff):
    assert call('efgh_wino2d_dy', geom, N, P(G, goff), i64(ldg), i32(N), *map(i32, geom), P(Gy, gyoff)) == 0


def rc_bwd(dy, dyoff, lddy, raw, rawoff, ldraw, bits, bitsoff, psc, psh, p, m1, m2, N, geom, a, slope, Vd, vdoff, Gy, gyoff, dres, dresoff,
           lddres):
    return call('efgh_wino2d_bwd_transforms', geom, N, P(dy, dyoff), i64(lddy), P(raw, rawoff), i64(ldraw), P(bits, bitsoff), P(psc),
                P(psh), P(p['mean']), P(p['invstd']), P(p['scale']), P(m1), P(m2), i32(N), *map(i32, geom), i32(a), f32(slope),
                P(Vd, vdoff), P(Gy, gyoff), P(dres, dresoff), i64(lddres))


def rc_bwd_pooled(dyp, dyoff, lddy, raw, rawoff, ldraw, p, m1, m2, N, geom, a, slope, Vd, vdoff, Gy, gyoff):
    return call('efgh_wino2d_bwd_transforms_pooled', geom, N, P(dyp, dyoff), i64(lddy), P(raw, rawoff), i64(ldraw), P(p['scale']),
                P(p['shift']), P(p['mean']), P(p['invstd']), P(p['scale']), P(m1), P(m2), i32(N), *map(i32, geom), i32(a), f32(slope),
                P(Vd, vdoff), P(Gy, gyoff))


def label_of(what, geom, N, a, slope, extra=''):
    return '%s %s N %d act %d slope %g%s' % (what, 'x'.join(map(str, geom)), N, a, slope, extra)


def placed_bits(pos):
    """the packed mask at a non-zero 8-byte-aligned offset of a larger int32 buffer -> (buffer, offset in words)"""
    w = BC.pack_bits(pos)
    buf = torch.full((w.numel() + 2 + 8,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    buf[2:2 + w.numel()] = w
    return buf, 2


# ------------------------------------------------------------------------------------------------ the fused forms
def check_plain(c, geom, N, a, slope, src, want_dres, unfused=False):
    B, H, W = geom
    M, T = B * H * W, W2.geo(*geom)[2]
    p = c['p']
    assert c['ambiguous'] == 0
    lddy, ldraw, lddres = N + 4, N + 8, N + 12
    dybuf, dy2 = place(c['dy'], lddy, 4)
    rawbuf, raw2 = place(c['raw'], ldraw, 8)
    drbuf, dr2 = out_rows(M, N, lddres, 12)
    b_dr = drbuf.clone()
    vdbuf, Vd, voff = out_tiles(T, N)
    gybuf, Gy, goff = out_tiles(T, N, 4)
    bits, boff = placed_bits(c['pos']) if src == 'bits' else (None, 0)
    psc, psh = (None, None) if src == 'bits' else (p['scale'], p['shift'])
    assert rc_bwd(dybuf, 4, lddy, rawbuf, 8, ldraw, bits, boff, psc, psh, p, c['m1'], c['m2'], N, geom, a, slope, vdbuf, voff, gybuf, goff,
                  drbuf if want_dres else None, 12, lddres) == 0
    torch.cuda.synchronize()
    lab = label_of('bwd_transforms', geom, N, a, slope, ' %s%s' % (src, ' dres' if want_dres else ''))
    dy4, raw4, dr4 = dy2.view(B, H, W, N), raw2.view(B, H, W, N), dr2.view(B, H, W, N)
    pos4 = c['pos'].view(B, H, W, N) if src == 'bits' else None
    if unfused:
        # the materialised form: the two-pass draw, then the stand-alone transforms of it
        from efgh_amd import ops
        draw = sentinel(M * N)
        ops.act_bn_bwd_apply(dybuf[4:], lddy, None if bits is None else bits[boff:], 0, rawbuf[8:], ldraw, p['mean'], p['invstd'], p['scale'],
                             c['m1'], c['m2'], M, N, a, slope, draw, N, None, 0, pscale=psc, pshift=psh)
        _, V2, _ = out_tiles(T, N)
        _, G2, _ = out_tiles(T, N)
        k_input(draw, 0, N, N, geom, V2, 0)
        k_dy(draw, 0, N, N, geom, G2, 0)
        torch.cuda.synchronize()
    for ch in W2.tile_row_chunks(B, H, W, N):
        ref = W2.bwd_transforms_ref(dy4, raw4, pos4, psc, psh, p['mean'], p['invstd'], p['scale'], c['m1'], c['m2'], a, slope, ch)
        assert W2.check_tiles('vd', lab, Vd, ref['Vd'], ref['S_Vd'], ch, H, W) == 0, (lab, 'Vd')
        assert W2.check_tiles('gyd', lab, Gy, ref['Gy'], ref['S_Gy'], ch, H, W) == 0, (lab, 'Gy')
        if want_dres:
            assert W2.check_dres(lab, dr4, ref, ch, H) == 0, (lab, 'dres')
        if unfused:
            t0, t1 = W2.tiles_of(ch, H, W)
            assert cmp('vd', lab, Vd[t0:t1], V2[t0:t1].double(), ref['S_Vd'], factor=2.0) == 0, (lab, 'Vd against efgh_wino2d_input(draw)')
            assert cmp('gyd', lab, Gy[t0:t1], G2[t0:t1].double(), ref['S_Gy'], factor=2.0) == 0, (lab, 'Gy against efgh_wino2d_dy(draw)')
    assert tiles_outside_unchanged(vdbuf, T, N, voff) == 0 and tiles_outside_unchanged(gybuf, T, N, goff) == 0, (lab, 'guard zones')
    if want_dres:
        assert outside_unchanged(drbuf, b_dr, 12, lddres, M, N) == 0, (lab, 'outside dres')
    else:
        assert torch.equal(drbuf, b_dr), (lab, 'dres absent')


@pytest.mark.parametrize('N', W2.FUSED_N)
@pytest.mark.parametrize('geom', W2.GEOMS, ids=_ids)
def test_bwd_transforms(geom, N):
    TH, TW, T = W2.geo(*geom)
    if N == 64:
        assert (TW * N) % 256 != 0 or geom == (1, 4, 13)              # tx >= TW cuts inside a workgroup (TW = 4: a whole one)
    for a, slope in W2.ACTS:
        c = W2.gen_plain(geom, N, a, slope, DEV)
        for src in ('bits', 'affine'):
            for want_dres in (True, False):
                check_plain(c, geom, N, a, slope, src, want_dres, unfused=want_dres)


def check_pooled(c, geom, N, a, slope, unfused=True):
    B, H, W = geom
    Ho, Wo = H // 2, W // 2
    M, T = B * H * W, W2.geo(*geom)[2]
    p = c['p']
    assert c['ambiguous'] == 0
    lddy, ldraw = N + 4, N + 8
    dybuf, dy2 = place(c['dy_pool'].view(-1, N), lddy, 4)
    rawbuf, raw2 = place(c['raw'].view(-1, N), ldraw, 8)
    vdbuf, Vd, voff = out_tiles(T, N)
    gybuf, Gy, goff = out_tiles(T, N, 4)
    assert rc_bwd_pooled(dybuf, 4, lddy, rawbuf, 8, ldraw, p, c['m1'], c['m2'], N, geom, a, slope, vdbuf, voff, gybuf, goff) == 0
    torch.cuda.synchronize()
    lab = label_of('bwd_transforms_pooled', geom, N, a, slope)
    dy4, raw4 = dy2.view(B, Ho, Wo, N), raw2.view(B, H, W, N)
    if unfused:
        from efgh_amd import ops
        draw = sentinel(M * N)
        assert ops._L().efgh_pool_bn_bwd_apply(P(c['dy_pool']), P(c['raw']), P(p['mean']), P(p['invstd']), P(p['scale']), P(c['m1']),
                                               P(c['m2']), P(p['scale']), P(p['shift']), i32(B), i32(H), i32(W), i32(N), i32(a), f32(slope),
                                               P(draw), ops._st()) == 0
        _, V2, _ = out_tiles(T, N)
        _, G2, _ = out_tiles(T, N)
        k_input(draw, 0, N, N, geom, V2, 0)
        k_dy(draw, 0, N, N, geom, G2, 0)
        torch.cuda.synchronize()
    for ch in W2.tile_row_chunks(B, H, W, N):
        ref = W2.bwd_transforms_pooled_ref(dy4, raw4, p['scale'], p['shift'], p['mean'], p['invstd'], p['scale'], c['m1'], c['m2'], a, slope,
                                           ch)
        assert W2.check_tiles('vd', lab, Vd, ref['Vd'], ref['S_Vd'], ch, H, W) == 0, (lab, 'Vd')
        assert W2.check_tiles('gyd', lab, Gy, ref['Gy'], ref['S_Gy'], ch, H, W) == 0, (lab, 'Gy')
        if unfused:
            t0, t1 = W2.tiles_of(ch, H, W)
            assert cmp('vd', lab, Vd[t0:t1], V2[t0:t1].double(), ref['S_Vd'], factor=2.0) == 0, (lab, 'Vd against efgh_wino2d_input(draw)')
            assert cmp('gyd', lab, Gy[t0:t1], G2[t0:t1].double(), ref['S_Gy'], factor=2.0) == 0, (lab, 'Gy against efgh_wino2d_dy(draw)')
    assert tiles_outside_unchanged(vdbuf, T, N, voff) == 0 and tiles_outside_unchanged(gybuf, T, N, goff) == 0, (lab, 'guard zones')


@pytest.mark.parametrize('N', W2.FUSED_N)
@pytest.mark.parametrize('geom', W2.POOL_GEOMS, ids=_ids)
def test_bwd_transforms_pooled(geom, N):
    for a, slope in W2.ACTS:
        check_pooled(W2.gen_pooled(geom, N, a, slope, DEV, ties=geom == W2.POOL_TIES), geom, N, a, slope)


# ------------------------------------------------------------------------------------------------ the stand-alone transforms
def check_standalone(c, geom, C, a, slope, which=('input', 'input_act', 'dy')):
    B, H, W = geom
    M, T = B * H * W, W2.geo(*geom)[2]
    p = c['p']
    lda, ldg = C + 4, C + 8
    abuf, A2 = place(c['raw'], lda, 4)
    gbuf, G2 = place(c['dy'], ldg, 8)
    A4, G4 = A2.view(B, H, W, C), G2.view(B, H, W, C)
    outs = {}
    if 'input' in which:
        outs['input'] = out_tiles(T, C)
        k_input(abuf, 4, lda, C, geom, outs['input'][0], 8)
    if 'input_act' in which:
        outs['input_act'] = out_tiles(T, C, 4)
        k_input_act(abuf, 4, lda, C, geom, p['scale'], p['shift'], a, slope, outs['input_act'][0], 4)
    if 'dy' in which:
        outs['dy'] = out_tiles(T, C, 12)
        k_dy(gbuf, 8, ldg, C, geom, outs['dy'][0], 12)
    torch.cuda.synchronize()
    for ch in W2.tile_row_chunks(B, H, W, C):
        for name, (buf, got, off) in outs.items():
            lab = label_of(name, geom, C, a, slope)
            if name == 'input':
                assert W2.check_tiles('v', lab, got, *W2.input_ref(A4, ch), ch, H, W) == 0, lab
            elif name == 'input_act':
                assert W2.check_tiles('v_act', lab, got, *W2.input_act_ref(A4, p['scale'], p['shift'], a, slope, ch), ch, H, W) == 0, lab
            else:
                assert W2.check_tiles('gy', lab, got, *W2.dy_ref(G4, ch), ch, H, W) == 0, lab
    for name, (buf, got, off) in outs.items():
        assert tiles_outside_unchanged(buf, T, C, off) == 0, (name, geom, C, 'guard zones')


@pytest.mark.parametrize('C', W2.PLAIN_C)
@pytest.mark.parametrize('geom', W2.GEOMS, ids=_ids)
def test_standalone_transforms(geom, C):
    B, H, W = geom
    for i, (a, slope) in enumerate(W2.ACTS):
        c = BC.gen_rows(B * H * W, C, W2.case_seed(geom, C, a, slope), DEV, a, slope)
        assert c['ambiguous'] == 0
        check_standalone(c, geom, C, a, slope, which=('input', 'input_act', 'dy') if i == 0 else ('input_act',))


# ------------------------------------------------------------------------------------------------ non-finite containment
@pytest.mark.parametrize('a,slope', [(BC.ACT_NONE, 0.0), (ACT_RELU, 0.0)])
def test_non_finite_gradient_stays_in_the_tiles_that_contain_it(a, slope):
    """one inf at pixel (0,0) of the first image and one NaN at pixel (H-1,W-1) of the last, every channel: a clamped read of an edge
    pixel must not leak into a tap that is zeroed afterwards"""
    geom, N = W2.NONFINITE_GEOM, 64
    B, H, W = geom
    TH, TW, T = W2.geo(*geom)
    M = B * H * W
    c = W2.gen_plain(geom, N, a, slope, DEV)
    p = c['p']
    dy = c['dy'].clone().view(B, H, W, N)
    planted = [(0, 0, 0), (B - 1, H - 1, W - 1)]
    dy[0, 0, 0] = float('inf')
    dy[B - 1, H - 1, W - 1] = float('nan')
    in_window = torch.zeros(T, dtype=torch.bool, device=DEV)
    in_tile = torch.zeros(T, dtype=torch.bool, device=DEV)
    for b, y, x in planted:
        for ty in range(TH):
            for tx in range(TW):
                t = (b * TH + ty) * TW + tx
                in_window[t] |= 4 * ty - 1 <= y <= 4 * ty + 4 and 4 * tx - 1 <= x <= 4 * tx + 4
                in_tile[t] |= 4 * ty <= y <= 4 * ty + 3 and 4 * tx <= x <= 4 * tx + 3
    assert int(in_window.sum()) == 5 and int(in_tile.sum()) == 2      # (0,0): one tile; (4,8) of 5x9: four windows, one tile
    for src in ('bits', 'affine'):
        lddy, ldraw, lddres = N + 4, N + 8, N + 12
        dybuf, dy2 = place(dy.view(M, N), lddy, 4)
        rawbuf, raw2 = place(c['raw'], ldraw, 8)
        drbuf, dr2 = out_rows(M, N, lddres, 12)
        vdbuf, Vd, voff = out_tiles(T, N)
        gybuf, Gy, goff = out_tiles(T, N, 4)
        bits, boff = placed_bits(c['pos']) if src == 'bits' else (None, 0)
        psc, psh = (None, None) if src == 'bits' else (p['scale'], p['shift'])
        assert rc_bwd(dybuf, 4, lddy, rawbuf, 8, ldraw, bits, boff, psc, psh, p, c['m1'], c['m2'], N, geom, a, slope, vdbuf, voff, gybuf,
                      goff, drbuf, 12, lddres) == 0
        torch.cuda.synchronize()
        lab = label_of('bwd_transforms non-finite', geom, N, a, slope, ' ' + src)
        pos4 = c['pos'].view(B, H, W, N) if src == 'bits' else None
        clean = torch.ones((B, H, W), dtype=torch.bool, device=DEV)
        for b, y, x in planted:
            clean[b, y, x] = False
        for ch in W2.tile_row_chunks(B, H, W, N):
            ref = W2.bwd_transforms_ref(dy2.view(B, H, W, N), raw2.view(B, H, W, N), pos4, psc, psh, p['mean'], p['invstd'], p['scale'],
                                        c['m1'], c['m2'], a, slope, ch)
            t0, t1 = W2.tiles_of(ch, H, W)
            kv, kg = ~in_window[t0:t1], ~in_tile[t0:t1]
            assert bool(torch.isfinite(ref['Vd'][kv]).all()) and bool(torch.isfinite(ref['Gy'][kg]).all())
            assert cmp('vd', lab, Vd[t0:t1][kv], ref['Vd'][kv], ref['S_Vd'][kv]) == 0, (lab, 'Vd')
            assert cmp('gyd', lab, Gy[t0:t1][kg], ref['Gy'][kg], ref['S_Gy'][kg]) == 0, (lab, 'Gy')
            y0, y1 = W2.rows_of(ch, H)
            k = clean[ch[0], y0:y1]
            got = dr2.view(B, H, W, N)[ch[0], y0:y1][k]
            assert BC.cmp('elem', lab + ' dres', got, ref['dres'][k], ref['S_dres'][k]) == 0, (lab, 'dres')
            # the tiles that do contain a planted pixel show it (the case is not vacuous)
            assert not bool(torch.isfinite(Vd[t0:t1][~kv]).all(-1).all(-1).any())


# ------------------------------------------------------------------------------------------------ the non-temporal switch
def nt_inputs(geom):
    if geom not in _NT:
        _NT.clear()
        torch.cuda.empty_cache()
        a, slope = W2.NT_ACT
        _NT[geom] = dict(plain=W2.gen_plain(geom, W2.NT_N, a, slope, DEV), pooled=W2.gen_pooled(geom, W2.NT_N, a, slope, DEV))
    return _NT[geom]


@pytest.mark.parametrize('entry', ['plain_bits', 'plain_affine', 'pooled', 'input', 'input_act', 'dy'])
@pytest.mark.parametrize('geom', [W2.NT_BELOW, W2.NT_ABOVE], ids=_ids)
def test_both_sides_of_the_non_temporal_switch(geom, entry):
    N = W2.NT_N
    nbytes = W2.nt_bytes(*geom, N)
    assert (nbytes < BC.NT_BYTES) == (geom == W2.NT_BELOW) and (nbytes >= BC.NT_BYTES) == (geom == W2.NT_ABOVE)
    assert len(W2.tile_row_chunks(*geom, N)) > 1                       # (the reference runs in tile-row chunks)
    a, slope = W2.NT_ACT
    c = nt_inputs(geom)
    if entry == 'plain_bits':
        check_plain(c['plain'], geom, N, a, slope, 'bits', True)
    elif entry == 'plain_affine':
        check_plain(c['plain'], geom, N, a, slope, 'affine', False)
    elif entry == 'pooled':
        check_pooled(c['pooled'], geom, N, a, slope, unfused=False)
    else:
        check_standalone(c['plain'], geom, N, a, slope, which=(entry,))


# ------------------------------------------------------------------------------------------------ refusals
def test_forbidden_calls_return_an_error_and_write_nothing():
    """every buffer would be valid for the call (sized for N = 128 and H = 4), so a wrongly accepted call cannot go out of bounds"""
    geom, a, slope = (1, 4, 5), ACT_RELU, 0.0
    B, H, W = geom
    M, T, NB = B * H * W, W2.geo(*geom)[2], 128
    c = W2.gen_plain(geom, NB, a, slope, DEV)
    cp = W2.gen_pooled(geom, NB, a, slope, DEV)
    p = c['p']
    ld = NB + 8
    dybuf, _ = place(c['dy'], ld, 8)
    rawbuf, _ = place(c['raw'], ld, 8)
    dypbuf, _ = place(cp['dy_pool'].view(-1, NB), ld, 8)
    bits, boff = placed_bits(c['pos'])
    outs = [out_tiles(T, NB)[0], out_tiles(T, NB)[0], sentinel(8 + (M + 2) * ld)]
    before = [o.clone() for o in outs]
    vd, gy, dr = outs
    sc, sh = p['scale'], p['shift']

    def plain(N=64, dyoff=8, lddy=ld, bits_=None, boff_=0, psc=sc, psh=sh, act=a, geom_=geom, vdoff=8):
        return rc_bwd(dybuf, dyoff, lddy, rawbuf, 8, ld, bits_, boff_, psc, psh, p, c['m1'], c['m2'], N, geom_, act, slope, vd, vdoff, gy, 8,
                      dr, 8, ld)

    def pooled(N=64, dyoff=8, lddy=ld, act=a, geom_=geom):
        return rc_bwd_pooled(dypbuf, dyoff, lddy, rawbuf, 8, ld, cp['p'], cp['m1'], cp['m2'], N, geom_, act, slope, vd, 8, gy, 8)

    refused = {
        'N = 32': plain(N=32), 'N = 96': plain(N=96), 'pooled N = 32': pooled(N=32), 'pooled N = 96': pooled(N=96),
        'both mask sources': plain(bits_=bits, boff_=boff), 'neither mask source': plain(psc=None, psh=None),
        'one half of the affine source': plain(psh=None),
        'ybits at an odd 4-byte offset': plain(bits_=bits, boff_=boff + 1, psc=None, psh=None),
        'lddy % 4 != 0': plain(lddy=ld - 2), 'pooled lddy % 4 != 0': pooled(lddy=ld - 2),
        'dy off by one float': plain(dyoff=9), 'Vd off by one float': plain(vdoff=9), 'pooled dy off by one float': pooled(dyoff=9),
        'act = 3': plain(act=3), 'pooled act = 3': pooled(act=3),
        'pooled at H = 1': pooled(geom_=(1, 1, 5)), 'pooled at W = 1': pooled(geom_=(1, 4, 1)),
    }
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused.values()), {k: rc for k, rc in refused.items() if rc == 0}
    for o, b in zip(outs, before):
        assert torch.equal(o, b), 'a refused call wrote'
    # the same builders with nothing wrong are accepted (the refusals above are not an artefact of the set-up)
    assert plain() == 0 and plain(bits_=bits, boff_=boff, psc=None, psh=None) == 0 and pooled() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ coverage and the tau table
def test_every_entry_point_ran_both_instances_and_the_tau_table():
    _NT.clear()
    torch.cuda.empty_cache()
    missing = [e for e in W2.ENTRY_POINTS if e not in CALLS]
    assert not missing, 'entry points never called (this test sums up the whole module: run the module, not the test): %s' % missing
    print('\nentry point                          calls  below 384 MiB  at or above')
    for e in W2.ENTRY_POINTS:
        lo, hi = sum(s < BC.NT_BYTES for s in CALLS[e]), sum(s >= BC.NT_BYTES for s in CALLS[e])
        print('%-36s %5d  %13d  %11d' % (e, len(CALLS[e]), lo, hi))
        assert lo and hi, '%s was not called on both sides of the non-temporal threshold' % e
    print('class   observed max |got - ref| / S   ceiling     tau        case')
    for cls in ('v', 'v_act', 'gy', 'vd', 'gyd'):
        v, lab = W2.OBSERVED[cls]
        print('%-7s %.3e (%6.2f x 2^-24)      %.3e   %.3e  %s' % (cls, v, v / BC.U, W2.CEIL[cls], W2.TAU_W2[cls], lab))
        assert W2.TAU_W2[cls] <= W2.CEIL[cls]
