"""G's head chain and the layout converters against the float64 contract of tests/heads_contract.py: direct calls of the eight C entry
points through ops._L() - the fold of the one-GEMM transposed convolution and its adjoint unfold on both of their routes (the route
asserted from the predicate of the entry point, restated here), the two 2-way softmax kernels and their backward passes on saturated,
infinite and NaN logit pairs, the planar <-> channels-last converters on NaN payloads, -0.0 and denormals - at the smallest shapes at
which each can go wrong: one pixel, one row, one column, Wo = 255 .. 259 around one 256-thread block, B = 65535 / 65536 at the limit of
gridDim.z, every legal pitch of Y and of the column rows, and pixel counts past the 16384-block grid cap.  Every output lies inside a
larger sentinel-filled buffer at a non-zero offset whose other elements must stay bit-unchanged; input padding is 1e30.  Then the chain
once, end to end, against the float64 CPU run of the same nn modules.  The last test asserts that all eight entry points and both
routes of each fold ran and prints the largest observed figure per class.

On the MI355X (97 tests, 6 s), largest (|got - ref| - floor) / (S x 2^-24) per class against its ceiling:  col2im 2.36 of 6 (vector route,
2x2x129, O 3, pad 1, opad 1, ldy 28, affine, no activation), softmax 2.01 of 5.6 (efgh_heads_to_nchw at 2 x 2097281 pixels; the fp32 CPU
yardstick is 1.86), softmax backward 3.70 of 4 (efgh_heads_bwd at 2 x 2097281 pixels, gradients of 1e-20 .. 1e20); im2col on both routes,
the depth copy, every +0.0 and the layout converters are bit-exact.  The chain, pose_contract.rel_err against the float64 modules: value
1.11e-06 of 2.87e-06 (fused heads 1x1 in train mode, depth), input gradient 3.11e-07 of 7.5e-07 (O 3, 3x129, on the tape), parameter
gradient 3.80e-06 of 1.5e-05 (fused heads 1x1 in train mode, the second BatchNorm weight of the depth stack).  Calls: col2im 235 vector /
1 scalar, im2col 289 vector / 343 scalar."""
import copy

import pytest
import torch

import heads_contract as HC
from heads_contract import bits, cmp, out_size, outside_unchanged, view2
from pose_contract import rel_err

pytestmark = pytest.mark.gpu

SENT = -7777.0
POISON = HC.POISON
DEV = 'cuda'
CALLS = {}
CHAIN_OBSERVED = {}
_QUERIES = ('_workspace', 'efgh_last_error', 'efgh_version')


class _Proxy:
    """ops._L() stand-in: forwards every attribute of the library and counts the calls of the efgh_* entry points"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith('efgh_') or any(q in name for q in _QUERIES):
            return f

        def call(*args):
            CALLS[name] = CALLS.get(name, 0) + 1
            return f(*args)
        return call


@pytest.fixture(scope='module', autouse=True)
def recorded_library():
    from efgh_amd import ops
    mp = pytest.MonkeyPatch()
    proxy = _Proxy(ops._L())
    mp.setattr(ops, '_L', lambda: proxy)
    yield
    mp.undo()


def L():
    from efgh_amd import ops
    return ops._L()


def st():
    from efgh_amd import _C
    return _C.stream_ptr()


def P(buf, off=0):
    return None if buf is None else buf.data_ptr() + buf.element_size() * off


def sentinel(n, value=SENT):
    return torch.full((int(n),), value, dtype=torch.float32, device=DEV)


def ok(rc):
    assert rc == 0, (rc, L().efgh_last_error())
    torch.cuda.synchronize()


def untouched(buf, off, ld, M, C):
    return outside_unchanged(buf, sentinel(buf.numel()), off, ld, M, C) == 0


def route(name, vec):
    k = '%s:%s' % (name, 'vector' if vec else 'scalar')
    CALLS[k] = CALLS.get(k, 0) + 1


# ------------------------------------------------------------------------------------------------ efgh_convt_col2im
OUT_OFF = 8              # 16-byte aligned, as the entry point demands


def run_col2im(case, Yd, y_off, scale, shift):
    """-> (output buffer, its [M][4] view); the route from the predicate of efgh_convt_col2im: the vector kernel iff B and Ho fit a grid"""
    B, Hin, Win, O, pad, opad, ldy, ldo, affine, act = case
    Ho, Wo = out_size(Hin, pad, opad), out_size(Win, pad, opad)
    M = B * Ho * Wo
    ob = sentinel(OUT_OFF + (M + 2) * ldo)
    assert P(ob, OUT_OFF) % 16 == 0
    route('efgh_convt_col2im', B <= 65535 and Ho <= 65535)
    ok(L().efgh_convt_col2im(P(Yd, y_off), ldy, B, Hin, Win, Ho, Wo, O, pad, P(scale), P(shift), act, HC.SLOPE, P(ob, OUT_OFF), ldo, st()))
    return ob, view2(ob, OUT_OFF, ldo, M, 4)


@pytest.mark.parametrize('O', [1, 2, 3, 4])
@pytest.mark.parametrize('geom', HC.GEOMS, ids=lambda g: '%dx%dx%d' % g)
def test_col2im_every_pitch_padding_and_epilogue(geom, O):
    cases = [c for c in HC.col2im_cases() if c[:3] == geom and c[3] == O]
    assert len(cases) >= 6 and {c[7] for c in cases} == {4, 8} and {c[9] for c in cases} == {0, 1, 2} and {c[8] for c in cases} == {0, 1}
    nan_seen = False
    for case in cases:
        B, Hin, Win, _, pad, opad, ldy, ldo, affine, act = case
        buf, scale, shift = HC.gen_col2im(case)
        ref, S = HC.ref_col2im(case)
        nan_seen |= bool(torch.isnan(ref).any())
        sc, sh = (scale.to(DEV), shift.to(DEV)) if affine else (None, None)
        ob, got = run_col2im(case, buf.to(DEV), HC.COL2IM_OFF, sc, sh)
        M = got.shape[0]
        assert cmp('col2im', 'col2im %s' % (case,), got.cpu(), ref.reshape(M, 4), S.reshape(M, 4)) == 0, case
        assert O == 4 or int((bits(got[:, O:]) != 0).sum()) == 0, case                 # channels >= O are +0.0
        assert untouched(ob, OUT_OFF, ldo, M, 4), case                                 # at ldo 8, columns 4..7 keep the sentinel
    assert nan_seen == (geom == HC.NAN_GEOM)


def test_col2im_route_limit_of_the_batch_size():
    """B = 65535: the vector kernel at the largest legal gridDim.z; B = 65536: the scalar kernel.  Both against the reference, and
    bit-equal to each other on the 65535 samples they share"""
    O, ldy = 2, 20
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    Y = torch.full((65536 + 1, ldy), POISON, device=DEV)
    Y[:65536, :9 * O] = torch.randn((65536, 9 * O), generator=g, device=DEV)
    scale, shift = torch.tensor([1.25, -0.5, POISON, POISON], device=DEV), torch.tensor([0.1, 0.3, POISON, POISON], device=DEV)
    outs = []
    for B in (65535, 65536):
        case = (B, 1, 1, O, 1, 1, ldy, 4, 1, 2)
        ob, got = run_col2im(case, Y.reshape(-1), 0, scale, shift)
        ref, S = HC.col2im(Y.reshape(-1).cpu(), ldy, B, 1, 1, 2, 2, O, 1, scale.cpu(), shift.cpu(), 2, HC.SLOPE)
        assert cmp('col2im', 'col2im B %d' % B, got.cpu(), ref.reshape(-1, 4), S.reshape(-1, 4)) == 0
        assert untouched(ob, OUT_OFF, 4, B * 4, 4)
        outs.append(got)
    assert torch.equal(bits(outs[0]), bits(outs[1][:65535 * 4]))
    assert CALLS.get('efgh_convt_col2im:scalar', 0) >= 1


# ------------------------------------------------------------------------------------------------ efgh_convt_im2col
Y_OFF = 8


def im2col_vec(B, Hin, Win, ldy, ldg, Gp, Yp):
    """the predicate `vec` of efgh_convt_im2col, restated"""
    return (B <= 65535 and Hin <= 65535 and ldy % 4 == 0 and ldy <= 40 and ldg % 4 == 0 and Gp % 16 == 0 and Yp % 16 == 0
            and (2 * Win + 8) * ldg * 4 < 2 ** 31)


def run_im2col(case, ldy, want_vec, ldg=None, g_shift=0, y_off=Y_OFF, src=None):
    """-> the [M][ldy] column rows, after holding them to the reference and the buffer around them to the sentinel
    (src: the case whose G buffer is read, when it is a larger one than `case` needs)"""
    B, Hin, Win, O, pad, opad, ldg0 = case
    ldg = ldg or ldg0
    Ho, Wo = out_size(Hin, pad, opad), out_size(Win, pad, opad)
    buf, off = HC.gen_im2col(src or case, ldg)
    gd = sentinel(buf.numel() + g_shift, POISON)
    gd[g_shift:] = buf.to(DEV)
    M = B * Hin * Win
    yb = sentinel(y_off + (M + 2) * ldy)
    Gp, Yp = P(gd, off + g_shift), P(yb, y_off)
    vec = im2col_vec(B, Hin, Win, ldy, ldg, Gp, Yp)
    assert vec == want_vec, (case, ldy, ldg, g_shift, y_off)
    route('efgh_convt_im2col', vec)
    ok(L().efgh_convt_im2col(Gp, ldg, B, Hin, Win, Ho, Wo, O, pad, Yp, ldy, st()))
    got = view2(yb, y_off, ldy, M, ldy)
    label = 'im2col %s ldy %d ldg %d %s' % (case, ldy, ldg, 'vector' if vec else 'scalar')
    assert cmp('copy', label, got.cpu(), HC.im2col(buf, ldg, B, Hin, Win, Ho, Wo, O, pad, ldy, off)) == 0, label     # pad columns +0.0 too
    assert untouched(yb, y_off, ldy, M, ldy), label
    return got


@pytest.mark.parametrize('geom', HC.GEOMS, ids=lambda g: '%dx%dx%d' % g)
def test_im2col_both_routes_every_pitch_and_every_trigger_of_the_scalar_route(geom):
    cases = [c for c in HC.im2col_cases() if c[:3] == geom]
    assert len(cases) == 12 and {c[6] for c in cases} == {4, 8}
    for case in cases:
        O = case[3]
        vec = {ldy: run_im2col(case, ldy, True) for ldy in HC.vec_ldys(O)}
        base = vec[min(vec)][:, :9 * O]
        for ldy in vec:
            assert torch.equal(bits(vec[ldy][:, :9 * O]), bits(base))
        scalar = [run_im2col(case, 44, False), run_im2col(case, min(vec), False, ldg=6), run_im2col(case, min(vec), False, g_shift=1),
                  run_im2col(case, min(vec), False, y_off=Y_OFF + 1)]
        if 9 * O % 4:
            scalar.append(run_im2col(case, 9 * O, False))
        # the two routes are bit-equal wherever both are legal: same G values, same real columns (ldg 6 draws the same numbers)
        for got in scalar:
            assert torch.equal(bits(got[:, :9 * O]), bits(base)), case


def test_im2col_route_limit_of_the_batch_size():
    """B = 65535: the vector kernel at the largest legal gridDim.z; B = 65536: the scalar kernel, on the same G: bit-equal on the
    65535 samples they share"""
    big = (65536, 1, 1, 2, 1, 1, 4)
    outs = [run_im2col((B, 1, 1, 2, 1, 1, 4), 20, want_vec, src=big) for B, want_vec in ((65535, True), (65536, False))]
    assert outs[0].shape == (65535, 20) and torch.equal(bits(outs[0]), bits(outs[1][:65535]))


@pytest.mark.parametrize('O', [1, 2, 3, 4])
def test_fold_and_unfold_are_adjoint_on_the_device(O):
    """<col2im(Y), G> == <Y, im2col(G)> from the device outputs (scale / shift null, act 0): the unfold is exact, so the two sides differ
    by the fold's error alone, sum CEIL S |G|"""
    for B, Hin, Win in [(3, 3, 4), (2, 2, 129), (1, 1, 1)]:
        for pad, opad in HC.PAD_OPAD:
            ldy = HC.ceil4(9 * O)
            ccase = (B, Hin, Win, O, pad, opad, ldy, 4, 0, 0)
            ybuf, _, _ = HC.gen_col2im(ccase)
            if bool(torch.isnan(ybuf).any()):
                ybuf = torch.nan_to_num(ybuf, nan=0.5)
            _, out = run_col2im(ccase, ybuf.to(DEV), HC.COL2IM_OFF, None, None)
            icase = (B, Hin, Win, O, pad, opad, 4)
            cols = run_im2col(icase, ldy, True)
            gbuf, goff = HC.gen_im2col(icase)
            Ho, Wo = out_size(Hin, pad, opad), out_size(Win, pad, opad)
            G = view2(gbuf, goff, 4, B * Ho * Wo, O).double()
            Y = view2(ybuf, HC.COL2IM_OFF, ldy, B * Hin * Win, 9 * O).double()
            lhs = float((out.cpu().double()[:, :O] * G).sum())
            rhs = float((Y * cols.cpu().double()[:, :9 * O]).sum())
            _, S = HC.col2im(ybuf, ldy, B, Hin, Win, Ho, Wo, O, pad, None, None, 0, 0.0, HC.COL2IM_OFF)
            bound = HC.CEIL['col2im'] * float((S.reshape(-1, 4)[:, :O] * G.abs()).sum()) + 1e-12 * abs(rhs) + 1e-30
            assert abs(lhs - rhs) <= bound, (ccase, lhs, rhs, bound)


# ------------------------------------------------------------------------------------------------ the softmax pair and the heads
def place_rows(t, ld, off, value=POISON, tail=1):
    M, C = t.shape
    buf = sentinel(off + (M + tail) * ld, value)
    view2(buf, off, ld, M, C).copy_(t)
    return buf


def planar_in(t, off=3):
    """a contiguous planar input at element `off` of a poisoned buffer"""
    buf = sentinel(off + t.numel() + 5, POISON)
    buf[off:off + t.numel()] = t.reshape(-1).to(DEV)
    return buf


def run_softmax2(lg, ld, B, HW, x_off=3):
    xb = place_rows(lg, ld, x_off)
    ob = sentinel(5 + 2 * B * HW + 3)
    ok(L().efgh_softmax2_to_nchw(P(xb, x_off), ld, P(ob, 5), B, HW, st()))
    assert untouched(ob, 5, 2 * B * HW, 1, 2 * B * HW)
    return ob[5:5 + 2 * B * HW].view(B, 2, HW)


@pytest.mark.parametrize('ld', [2, 4, 7])
def test_softmax2_to_nchw_saturated_infinite_and_nan_pairs(ld):
    nan = 0
    for case in HC.softmax_cases():
        B, HW, rot = case
        lg = HC.gen_logits(case)
        ref, S = HC.softmax2_to_nchw(lg.reshape(-1), 2, B, HW)
        got = run_softmax2(lg, ld, B, HW)
        nan += int(torch.isnan(ref).sum())
        assert cmp('softmax', 'softmax2 ld %d %s' % (ld, case), got.cpu(), ref, S) == 0, case
    assert nan >= 20


def run_heads(x4, B, HW):
    """x4 [B*HW][4] -> (depth [B*HW], mask [B][2][HW]) out of sentinel buffers"""
    xb = place_rows(x4, 4, 8)
    db, mb = sentinel(3 + B * HW + 4), sentinel(5 + 2 * B * HW + 3)
    ok(L().efgh_heads_to_nchw(P(xb, 8), P(db, 3), P(mb, 5), B, HW, st()))
    assert untouched(db, 3, B * HW, 1, B * HW) and untouched(mb, 5, 2 * B * HW, 1, 2 * B * HW)
    return db[3:3 + B * HW], mb[5:5 + 2 * B * HW].view(B, 2, HW)


def test_heads_to_nchw_depth_is_a_copy_and_the_mask_the_softmax():
    for case in HC.softmax_cases():
        B, HW, rot = case
        lg = HC.gen_logits(case)
        x4 = torch.cat([HC.special_floats(B * HW, rot)[:, None], lg, torch.full((B * HW, 1), POISON)], 1)
        depth, mask = run_heads(x4, B, HW)
        d, m, S = HC.heads_fwd(x4.reshape(-1), B, HW)
        assert cmp('copy', 'heads depth %s' % (case,), depth.cpu(), d) == 0, case
        assert cmp('softmax', 'heads %s' % (case,), mask.cpu(), m, S) == 0, case


def run_softmax2_bwd(y, dy, B, HW, ld):
    yb, gb = planar_in(y), planar_in(dy, 7)
    M = B * HW
    dxb = sentinel(5 + (M + 2) * ld)
    ok(L().efgh_softmax2_bwd(P(yb, 3), P(gb, 7), B, HW, P(dxb, 5), ld, st()))
    assert untouched(dxb, 5, ld, M, ld)                                               # rows behind the last keep the sentinel
    return view2(dxb, 5, ld, M, ld)


@pytest.mark.parametrize('ld', [2, 4, 7])
def test_softmax2_bwd_into_a_pitch(ld):
    for case in HC.bwd_cases():
        B, HW, kind = case
        y, dm, _ = HC.gen_bwd(case)
        for tag, g in (('mixed', dm), ('randn', torch.randn(dm.shape, generator=torch.Generator().manual_seed(B + HW)))):
            got = run_softmax2_bwd(y, g, B, HW, ld)
            ref, S = HC.softmax2_to_nchw_bwd(y, g, B, HW, ld)
            assert cmp('softmax_bwd', 'softmax2_bwd ld %d %s %s' % (ld, case, tag), got.cpu(), ref, S) == 0, case
            assert ld == 2 or int((bits(got[:, 2:]) != 0).sum()) == 0, case            # channels >= 2 of every row +0.0


def run_heads_bwd(y, dm, dd, B, HW):
    yb = planar_in(y)
    gb = None if dm is None else planar_in(dm, 7)
    db = None if dd is None else planar_in(dd, 2)
    M = B * HW
    dxb = sentinel(8 + (M + 2) * 4)
    ok(L().efgh_heads_bwd(P(yb, 3), P(gb, 7), P(db, 2), B, HW, P(dxb, 8), st()))
    assert untouched(dxb, 8, 4, M, 4)
    return view2(dxb, 8, 4, M, 4)


def check_heads_bwd(label, got, y, dm, dd, B, HW):
    """got on its device; the reference on the same device"""
    ref, S = HC.heads_bwd(y, dm, dd, B, HW)
    assert cmp('softmax_bwd', label, got[:, 1:3].contiguous(), ref[:, 1:3].contiguous(), S[:, 1:3].contiguous()) == 0, label
    want0 = torch.zeros(B * HW, device=got.device) if dd is None else dd.reshape(-1)
    assert cmp('copy', label, got[:, 0].contiguous(), want0) == 0, label                # a copy, or +0.0 for an absent gradient
    assert int((bits(got[:, 3]) != 0).sum()) == 0, label                               # channel 3 +0.0
    if dm is None:
        assert int((bits(got[:, 1:3]) != 0).sum()) == 0, label


@pytest.mark.parametrize('which', ['dmask', 'ddepth', 'both', 'neither'])
def test_heads_bwd_with_either_gradient_absent(which):
    for case in HC.bwd_cases():
        B, HW, kind = case
        y, dm, dd = HC.gen_bwd(case)
        dm = dm if which in ('dmask', 'both') else None
        dd = dd if which in ('ddepth', 'both') else None
        got = run_heads_bwd(y, dm, dd, B, HW)
        check_heads_bwd('heads_bwd %s %s' % (which, case), got.cpu(), y, dm, dd, B, HW)


def test_softmax_pair_and_heads_past_the_grid_cap():
    """2 x (2097152 + 129) pixels: the grid-stride loop of the four kernels does its second trip.  Compared on the device in float64,
    in chunks"""
    B, HW = HC.SOFTMAX_BIG
    M = B * HW
    assert M > 16384 * 256
    lg = HC.logits(M, 0, DEV)
    x4 = torch.cat([HC.special_floats(M, 9, DEV)[:, None], lg, torch.full((M, 1), POISON, device=DEV)], 1)
    xb = place_rows(x4, 4, 8, tail=2)
    depth, mask = run_heads(x4, B, HW)
    ob = sentinel(5 + 2 * M + 3)
    ok(L().efgh_softmax2_to_nchw(P(xb, 9), 4, P(ob, 5), B, HW, st()))                   # channels 1, 2 of the same rows
    assert untouched(ob, 5, 2 * M, 1, 2 * M)
    soft = ob[5:5 + 2 * M].view(B, 2, HW)
    assert cmp('copy', 'heads depth big', depth, x4[:, 0].contiguous()) == 0
    dm, dd = HC.mixed_grads((B, 2, HW), 3, DEV), HC.mixed_grads((M,), 4, DEV)
    y = torch.nan_to_num(mask, nan=0.5)
    gh = run_heads_bwd(y, dm, dd, B, HW)
    gs = run_softmax2_bwd(y, dm, B, HW, 4)
    step = 1 << 20
    for b in range(B):
        for p0 in range(0, HW, step):
            p1 = min(HW, p0 + step)
            rows = slice(b * HW + p0, b * HW + p1)
            y0, y1, S0, S1 = HC.softmax2(lg[rows, 0], lg[rows, 1])
            ref, S = torch.stack([y0, y1]), torch.stack([S0, S1])
            for name, got in (('heads', mask), ('softmax2', soft)):
                assert cmp('softmax', '%s big' % name, got[b, :, p0:p1].contiguous(), ref, S) == 0, (name, b, p0)
            yc, gc = y[b:b + 1, :, p0:p1].contiguous(), dm[b:b + 1, :, p0:p1].contiguous()
            check_heads_bwd('heads_bwd big', gh[rows], yc, gc, dd[rows], 1, p1 - p0)
            ref, S = HC.softmax2_to_nchw_bwd(yc, gc, 1, p1 - p0, 4)
            assert cmp('softmax_bwd', 'softmax2_bwd big', gs[rows].contiguous(), ref, S) == 0, (b, p0)
            assert int((bits(gs[rows][:, 2:]) != 0).sum()) == 0


# ------------------------------------------------------------------------------------------------ layout
def run_nchw_to_nhwc(pb, B, Cs, HW, Cd):
    ob = sentinel(7 + B * HW * Cd + 9)
    ok(L().efgh_nchw_to_nhwc(P(pb, HC.LAYOUT_OFF), P(ob, 7), B, Cs, HW, Cd, st()))
    assert untouched(ob, 7, B * HW * Cd, 1, B * HW * Cd)
    return ob[7:7 + B * HW * Cd].view(B * HW, Cd)


def run_nhwc_to_nchw(rb, ld, B, Cs, HW, off=HC.LAYOUT_OFF):
    ob = sentinel(3 + B * Cs * HW + 6)
    ok(L().efgh_nhwc_to_nchw(P(rb, off), ld, P(ob, 3), B, Cs, HW, st()))
    assert untouched(ob, 3, B * Cs * HW, 1, B * Cs * HW)
    return ob[3:3 + B * Cs * HW].view(B, Cs, HW)


@pytest.mark.parametrize('case', HC.LAYOUT_CASES, ids=lambda c: '%dx%dx%d_to_%d' % c)
def test_layout_converters_are_bit_exact_and_pad_with_zero(case):
    B, Cs, HW, Cd = case
    pbuf = HC.gen_planar(case)
    got = run_nchw_to_nhwc(pbuf.to(DEV), B, Cs, HW, Cd)
    assert cmp('copy', 'nchw_to_nhwc %s' % (case,), got.cpu(), HC.nchw_to_nhwc(pbuf, B, Cs, HW, Cd, HC.LAYOUT_OFF)) == 0
    back = run_nhwc_to_nchw(got, Cd, B, Cs, HW, 0)                                      # the round trip, bit-identical
    assert torch.equal(bits(back.reshape(-1).cpu()), bits(pbuf[HC.LAYOUT_OFF:HC.LAYOUT_OFF + B * Cs * HW]))
    for ld in HC.nhwc_lds(Cs):
        rbuf = HC.gen_rows(B, Cs, HW, ld)
        got = run_nhwc_to_nchw(rbuf.to(DEV), ld, B, Cs, HW)
        assert cmp('copy', 'nhwc_to_nchw %s ld %d' % (case, ld), got.cpu(), HC.nhwc_to_nchw(rbuf, ld, B, Cs, HW, HC.LAYOUT_OFF)) == 0


@pytest.mark.parametrize('B,Cs,HW,ld', HC.NHWC_EXTRA)
def test_nhwc_to_nchw_one_and_two_channels_of_a_four_channel_map(B, Cs, HW, ld):
    rbuf = HC.gen_rows(B, Cs, HW, ld)
    got = run_nhwc_to_nchw(rbuf.to(DEV), ld, B, Cs, HW)
    assert cmp('copy', 'nhwc_to_nchw Cs %d ld %d' % (Cs, ld), got.cpu(), HC.nhwc_to_nchw(rbuf, ld, B, Cs, HW, HC.LAYOUT_OFF)) == 0


def test_layout_converters_past_the_grid_cap():
    B, Cs, HW, Cd = HC.LAYOUT_BIG
    assert B * HW > 16384 * 256
    x = HC.special_floats(B * Cs * HW, 21, DEV)
    pb = sentinel(HC.LAYOUT_OFF + x.numel() + 7, POISON)
    pb[HC.LAYOUT_OFF:HC.LAYOUT_OFF + x.numel()] = x
    got = run_nchw_to_nhwc(pb, B, Cs, HW, Cd)
    assert cmp('copy', 'nchw_to_nhwc big', got, x.view(B, Cs, HW).permute(0, 2, 1).reshape(B * HW, Cs).contiguous()) == 0
    back = run_nhwc_to_nchw(got, Cd, B, Cs, HW, 0)
    assert torch.equal(bits(back.reshape(-1)), bits(x))
    two = run_nhwc_to_nchw(got, Cd, B, 2, HW, 0)                                        # two of four channels, past the cap as well
    assert torch.equal(bits(two), bits(x.view(B, Cs, HW)[:, :2].contiguous()))


# ------------------------------------------------------------------------------------------------ the chain once, end to end
def chain_check(label, got, ref):
    """got / ref: dict family -> {name: tensor}; every tensor of the float64 run within its family's ceiling"""
    bad = []
    for fam in ref:
        for n in ref[fam]:
            e = rel_err(got[fam][n], ref[fam][n])
            if e > CHAIN_OBSERVED.get(fam, (-1.0, ''))[0]:
                CHAIN_OBSERVED[fam] = (e, '%s %s' % (label, n))
            print('%-40s %-12s %-24s %.3e' % (label, fam, n, e))
            if not e <= HC.CHAIN_CEIL[fam]:
                bad.append((fam, n, e))
    assert not bad, (label, bad)


def _nhwc(x):
    """(B,C,H,W) -> [B][H][W][C] with the strides of a fresh allocation (at W == 1 `permute().contiguous()` keeps stride(-2) == 1,
    and the layers read the pitch of a map from stride(-2))"""
    B, C, H, W = x.shape
    return torch.empty((B, H, W, C), dtype=x.dtype).copy_(x.permute(0, 2, 3, 1))


@pytest.mark.parametrize('mode', HC.CHAIN_MODES)
@pytest.mark.parametrize('O', [1, 2, 3])
@pytest.mark.parametrize('H,W', HC.CHAIN_SHAPES)
def test_chain_transposed_head_layer_against_float64_modules(H, W, O, mode):
    from efgh_amd.nets import layers as LY
    ct, bn, x, gy = HC.chain_layer_case(O, H, W)
    ref = HC.chain_layer_run(O, H, W, mode, torch.float64)
    ct_g, bn_g = copy.deepcopy(ct).to(DEV), copy.deepcopy(bn).to(DEV)
    bn_g.train(mode != 'eval')
    xg = _nhwc(x).to(DEV).requires_grad_(mode == 'tape')
    before = (CALLS.get('efgh_convt_col2im', 0), CALLS.get('efgh_convt_im2col', 0))
    with torch.set_grad_enabled(mode == 'tape'):
        y = LY.conv_transpose2d(LY.Ctx(mode != 'eval'), xg, ct_g, bn_g, LY.ACT_LEAKY, 0.2)
    got = {'value': {'y': y.detach()[..., :O].permute(0, 3, 1, 2), 'running_mean': bn_g.running_mean, 'running_var': bn_g.running_var}}
    if mode == 'tape':
        gyp = torch.zeros(y.shape)
        gyp[..., :O] = gy.permute(0, 2, 3, 1)
        y.backward(gyp.to(DEV))
        got['input_grad'] = {'dx': xg.grad.permute(0, 3, 1, 2)}
        got['param_grad'] = {'ct.weight': ct_g.weight.grad, 'bn.weight': bn_g.weight.grad, 'bn.bias': bn_g.bias.grad}
        assert CALLS.get('efgh_convt_im2col', 0) > before[1]
    assert CALLS.get('efgh_convt_col2im', 0) > before[0]                                 # the small form: one GEMM + the fold
    chain_check('layer O %d %dx%d %s' % (O, H, W, mode), got, ref)


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'separate'])
@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('H,W', HC.CHAIN_SHAPES)
def test_chain_heads_against_float64_modules(H, W, train, fused):
    from efgh_amd import ops
    from efgh_amd.nets import fn as FN
    from efgh_amd.nets import layers as LY
    sd, sm, x, gd, gm = HC.chain_heads_case(H, W)
    ref = HC.chain_heads_run(H, W, train, torch.float64)
    sd_g, sm_g = copy.deepcopy(sd).to(DEV).train(train), copy.deepcopy(sm).to(DEV).train(train)
    assert LY.convt_heads_fusable(sd_g, sm_g)
    xg = _nhwc(x).to(DEV).requires_grad_(train)
    names = ('efgh_heads_to_nchw', 'efgh_heads_bwd') if fused else ('efgh_nhwc_to_nchw', 'efgh_softmax2_to_nchw', 'efgh_softmax2_bwd',
                                                                     'efgh_nchw_to_nhwc')
    before = {n: CALLS.get(n, 0) for n in names}
    with torch.set_grad_enabled(train):
        ctx = LY.Ctx(train)
        if fused:
            hm = LY.run_convt_heads(ctx, sd_g, sm_g, xg)
            d, m = FN.HeadsToNchwFn.apply(hm) if train else ops.heads_to_nchw(hm)
        else:
            dimg, alias = LY.run_convt_bn_relu(ctx, sd_g, xg, skip_out=True)
            mask = LY.run_convt_bn_relu(ctx, sm_g, alias)
            d, m = (FN.NhwcToNchwFn.apply(dimg, 1), FN.Softmax2ToNchwFn.apply(mask)) if train else \
                (ops.nhwc_to_nchw(dimg, 1), ops.softmax2_to_nchw(mask))
    got = {'value': {'depth': d.detach(), 'mask': m.detach()}}
    for tag, seq in (('d.', sd_g), ('m.', sm_g)):
        for n, b in seq.named_buffers():
            if b.dtype == torch.float32:
                got['value'][tag + n] = b
    if train:
        ((d * gd.to(DEV)).sum() + (m * gm.to(DEV)).sum()).backward()
        got['input_grad'] = {'dx': xg.grad.permute(0, 3, 1, 2)}
        got['param_grad'] = {tag + n: p.grad for tag, seq in (('d.', sd_g), ('m.', sm_g)) for n, p in seq.named_parameters()}
    for n in names:
        if train or not n.endswith('bwd') and n != 'efgh_nchw_to_nhwc':
            assert CALLS.get(n, 0) > before[n], n
    chain_check('heads %dx%d %s %s' % (H, W, 'train' if train else 'eval', 'fused' if fused else 'separate'), got, ref)


# ------------------------------------------------------------------------------------------------ coverage
def test_all_eight_entry_points_and_both_routes_of_each_fold_ran():
    missing = [n for n in HC.ENTRY_POINTS if not CALLS.get(n)]
    assert not missing, missing
    for k in ('efgh_convt_col2im:vector', 'efgh_convt_col2im:scalar', 'efgh_convt_im2col:vector', 'efgh_convt_im2col:scalar'):
        assert CALLS.get(k), k
    print({n: CALLS[n] for n in sorted(CALLS) if n.startswith('efgh_convt') or n in HC.ENTRY_POINTS})
    for cls in sorted(HC.OBSERVED):
        v, label = HC.OBSERVED[cls]
        if cls == 'copy':
            print('%-12s %d differing elements' % (cls, v))
            assert v == 0
        else:
            print('%-12s largest (|got - ref| - floor) / (S U) = %.3f of %.3f  (%s)' % (cls, v, HC.CEIL[cls] / HC.U, label))
            assert v <= HC.CEIL[cls] / HC.U
    for fam in sorted(CHAIN_OBSERVED):
        v, label = CHAIN_OBSERVED[fam]
        print('chain %-12s largest rel_err %.3e of %.3e  (%s)' % (fam, v, HC.CHAIN_CEIL[fam], label))
