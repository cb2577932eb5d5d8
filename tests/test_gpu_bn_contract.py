"""The BatchNorm, activation and max-pool kernels against the float64 contract of tests/bn_contract.py: direct calls of the 15 C entry
points at the smallest shapes at which each mechanism can go wrong (channel lanes and guards, row groups, the two-stage statistics
fold, the unrolled fold of the backward sums, the grid-stride trips, the non-temporal instances at 384 MiB), with every activation,
BatchNorm parameter sets that differ per channel within one launch, inputs on which fp32 and float64 cannot legitimately take
different branches (the ambiguous set is asserted empty before a kernel runs), exact ties kept, and every output inside a larger
sentinel-filled buffer whose other elements must stay bit-unchanged.  The last test asserts that all 15 entry points ran, each
non-temporal one on both sides of its threshold, and prints the table the taus of bn_contract.TAU_BN were taken from.

The entry points are called through the ops.* wrappers where those expose the arguments (scale_shift_act, act_bn_bwd_reduce /
_apply, maxpool2_bwd) and through ops._L() where a wrapper allocates its own output (no sentinels) or hides `part`.

On the MI355X (58 tests), largest |got - ref| / S per class:  elementwise 1.99 x 2^-24, fp32 outputs of the float64 sums 2.00,
m1 / m2 1.85, efgh_col_stats 12.3, efgh_bn_finalize 2.12."""
import ctypes

import pytest
import torch

import bn_contract as BC
from bn_contract import ACT_NONE, ACT_RELU, ACTS, cmp, outside_unchanged, view2

pytestmark = pytest.mark.gpu

SENT = -7777.0
DEV = 'cuda'
CALLS = {}               # entry point -> the byte counts its non-temporal switch saw, one per call
POOLED_REPORT = {}       # parameter set -> largest m2 error of the pooled-from-y / the from-raw reduction over sum |d||xhat| / count
RATIO_REPORT = {}        # |beta| / |gamma| -> the same error of efgh_pool_bn_bwd_reduce_pooled on the one-signed case
_QUERIES = ('_groups', 'efgh_last_error', 'efgh_version')
_LARGE = {}              # generated large cases, shared by the tests of one shape


def _val(a):
    return a.value if hasattr(a, 'value') else a


def _switch_bytes(name, args):
    """the bytes efgh_stream_nt is asked about by an entry point that has a non-temporal instance (None: it has none)"""
    v = [_val(a) for a in args]
    if name == 'efgh_scale_shift_act':
        return v[8] * v[9] * 4
    if name == 'efgh_scale_shift_act_bits':
        return v[9] * v[10] * 4
    if name == 'efgh_maxpool2_affine':
        return v[6] * v[7] * v[8] * v[9] * 4
    if name == 'efgh_act_bn_bwd_reduce':
        return v[10] * v[11] * 4
    if name == 'efgh_act_bn_bwd_apply':
        return v[13] * v[14] * 4
    if name == 'efgh_pool_bn_bwd_reduce':
        return v[6] * v[7] * v[8] * v[9] * 4
    if name == 'efgh_pool_bn_bwd_reduce_pooled':
        return v[7] * (v[8] // 2) * (v[9] // 2) * v[10] * 4
    if name == 'efgh_pool_bn_bwd_apply':
        return v[9] * v[10] * v[11] * v[12] * 4
    return None


class _Proxy:
    """ops._L() stand-in: forwards every attribute of the library and records the calls of the efgh_* entry points"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith('efgh_') or any(q in name for q in _QUERIES):
            return f

        def call(*args):
            CALLS.setdefault(name, []).append(_switch_bytes(name, args))
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
    _LARGE.clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ buffers and raw calls
def P(buf, off=0):
    """device pointer to element `off` of a tensor (None -> NULL)"""
    return ctypes.c_void_p(0 if buf is None else buf.data_ptr() + buf.element_size() * off)


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


def _ops():
    from efgh_amd import _C, ops
    return ops, _C


def i32(v):
    return ctypes.c_int32(int(v))


def i64(v):
    return ctypes.c_int64(int(v))


def f32(v):
    return ctypes.c_float(float(v))


def lib_query(name, *args):
    ops, _C = _ops()
    return getattr(ops._L(), name)(*args)


def k_scale_shift_act(x, xoff, ldx, scale, shift, res, roff, ldr, y, yoff, ldy, M, C, a, slope, bits=None):
    ops, _C = _ops()
    ops.scale_shift_act(x, ldx, scale, shift, y, ldy, M, C, act=a, slope=slope, res=res, ldr=ldr, x_off=xoff, y_off=yoff, res_off=roff,
                        bits=bits)


def k_col_stats(x, xoff, M, C, ld, stats):
    ops, _C = _ops()
    _C.check(ops._L().efgh_col_stats(P(x, xoff), i64(M), i32(C), i64(ld), P(stats), ops._st()))


def k_bn_finalize(stats, G, C, count, gamma, beta, rmean, rvar, momentum, eps, scale, shift, sm, si):
    ops, _C = _ops()
    _C.check(ops._L().efgh_bn_finalize(P(stats), i32(G), i32(C), ctypes.c_double(count), P(gamma), P(beta), P(rmean), P(rvar),
                                       f32(momentum), f32(eps), P(scale), P(shift), P(sm), P(si), ops._st()))


def k_pool(name, x, y, B, H, W, C):
    ops, _C = _ops()
    _C.check(getattr(ops._L(), name)(P(x), P(y), i32(B), i32(H), i32(W), i32(C), ops._st()))


def k_maxpool2_affine(x, scale, shift, a, slope, y, B, H, W, C):
    ops, _C = _ops()
    _C.check(ops._L().efgh_maxpool2_affine(P(x), P(scale), P(shift), i32(a), f32(slope), P(y), i32(B), i32(H), i32(W), i32(C), ops._st()))


def k_maxpool2_bwd(x, dy, dx, B, H, W, C):
    ops, _C = _ops()
    ops.maxpool2_bwd(x.view(B, H, W, C), dy, dx)


def k_maxpool2_bwd_affine(x, scale, shift, a, slope, dy, dx, B, H, W, C):
    ops, _C = _ops()
    _C.check(ops._L().efgh_maxpool2_bwd_affine(P(x), P(scale), P(shift), i32(a), f32(slope), P(dy), P(dx), i32(B), i32(H), i32(W),
                                               i32(C), ops._st()))


def at(buf, off):
    """the tensor a wrapper takes the pointer of: `buf` from element `off` on (None stays None)"""
    return None if buf is None else buf[off:]


def k_reduce(dy, dyoff, lddy, y, yoff, ldy, raw, rawoff, ldraw, mean, invstd, psc, psh, M, C, a, slope, out):
    ops, _C = _ops()
    ops.act_bn_bwd_reduce(at(dy, dyoff), lddy, at(y, yoff), ldy, at(raw, rawoff), ldraw, mean, invstd, M, C, a, slope, out['part'],
                          out['s1'], out['s2'], out['m1'], out['m2'], pscale=psc, pshift=psh)


def k_apply(dy, dyoff, lddy, y, yoff, ldy, raw, rawoff, ldraw, mean, invstd, coef, m1, m2, psc, psh, M, C, a, slope, draw, drawoff,
            lddraw, dres, dresoff, lddres):
    ops, _C = _ops()
    ops.act_bn_bwd_apply(at(dy, dyoff), lddy, at(y, yoff), ldy, at(raw, rawoff), ldraw, mean, invstd, coef, m1, m2, M, C, a, slope,
                         at(draw, drawoff), lddraw, at(dres, dresoff), lddres, pscale=psc, pshift=psh)


def k_bwd_finalize_f32(stats, rows, C, count, out):
    ops, _C = _ops()
    _C.check(ops._L().efgh_bwd_finalize_f32(P(stats), i32(rows), i32(C), ctypes.c_double(count), P(out['s1']), P(out['s2']),
                                            P(out['m1']), P(out['m2']), ops._st()))


def k_pool_reduce(dyp, raw, p, B, H, W, C, a, slope, out, y_pool=None):
    ops, _C = _ops()
    if y_pool is not None:
        _C.check(ops._L().efgh_pool_bn_bwd_reduce_pooled(P(dyp), P(y_pool), P(raw), P(p['mean']), P(p['invstd']), P(p['scale']),
                                                         P(p['shift']), i32(B), i32(H), i32(W), i32(C), P(out['part']), P(out['s1']),
                                                         P(out['s2']), P(out['m1']), P(out['m2']), ops._st()))
    else:
        _C.check(ops._L().efgh_pool_bn_bwd_reduce(P(dyp), P(raw), P(p['mean']), P(p['invstd']), P(p['scale']), P(p['shift']), i32(B),
                                                  i32(H), i32(W), i32(C), i32(a), f32(slope), P(out['part']), P(out['s1']),
                                                  P(out['s2']), P(out['m1']), P(out['m2']), ops._st()))


def k_pool_apply(dyp, raw, p, m1, m2, B, H, W, C, a, slope, draw):
    ops, _C = _ops()
    _C.check(ops._L().efgh_pool_bn_bwd_apply(P(dyp), P(raw), P(p['mean']), P(p['invstd']), P(p['scale']), P(m1), P(m2), P(p['scale']),
                                             P(p['shift']), i32(B), i32(H), i32(W), i32(C), i32(a), f32(slope), P(draw), ops._st()))


# ------------------------------------------------------------------------------------------------ derived quantities
def channel_lanes(C):
    """float4 channel lanes of a reduction block (efgh_col_stats, the backward reductions): the power of two below 64 that holds C/4"""
    cl = 1
    while cl < 64 and cl * 4 < C:
        cl <<= 1
    return cl


def bwd_rows_per_group(M):
    """rows per partial of the backward reductions: M / 1024 rounded up to a multiple of 16, at least 16"""
    rows = ((M + 1023) // 1024 + 15) // 16 * 16
    return max(rows, 16)


def bwd_groups(M):
    r = bwd_rows_per_group(M)
    return (M + r - 1) // r


def grid_trips(quads):
    """trips of the grid-stride loop of an elementwise kernel: 256 threads per block, at most 16 384 blocks"""
    return -(-quads // (16384 * 256))


def sums_out(G, C):
    """outputs of a backward reduction, each behind / in front of sentinels: part [G][2][C] float64, s1, s2 [C] float, m1, m2 [C] double"""
    return dict(part=sentinel((G + 1) * 2 * C, torch.float64), s1=sentinel(C + 4), s2=sentinel(C + 4),
                m1=sentinel(C + 4, torch.float64), m2=sentinel(C + 4, torch.float64))


def check_sums(label, out, ref, bnd, count, C, full=True, m_out=True):
    """the four outputs of a backward reduction against the float64 sums `ref` [2][C] and their bounds; full: the second sum counts"""
    torch.cuda.synchronize()
    n = 2 if full else 1
    for k, name in list(enumerate(('s1', 's2')))[:n]:
        assert cmp('f64sum', label + ' ' + name, out[name][:C], ref[k], bnd[k]) == 0, (label, name)
        assert bool((out[name][C:] == SENT).all()), (label, name, 'tail')
    if m_out:
        for k, name in list(enumerate(('m1', 'm2')))[:n]:
            assert cmp('m', label + ' ' + name, out[name][:C], ref[k] / count, bnd[k] / count) == 0, (label, name)
            assert bool((out[name][C:] == SENT).all()), (label, name, 'tail')
    assert bool((out['part'][-2 * C:] == SENT).all()), (label, 'part tail')


def label_of(shape, a, slope):
    return '%s act %d slope %g' % ('x'.join(str(v) for v in shape), a, slope)


# ------------------------------------------------------------------------------------------------ forward, [M][C]
def check_forward_rows(c, M, C, a, slope, lab, stats=True, chunks=None):
    p, raw, res = c['p'], c['raw'], c['res']
    assert c['ambiguous'] == 0
    xbuf, x = place(raw, C + 8, 4)
    rbuf, r = (None, None) if res is None else place(res, C + 12, 8)
    ybuf, y = out_rows(M, C, C + 4, 8)
    before = ybuf.clone()
    k_scale_shift_act(xbuf, 4, C + 8, p['scale'], p['shift'], rbuf, 8, C + 12, ybuf, 8, C + 4, M, C, a, slope)
    torch.cuda.synchronize()
    bits = None
    if C % 32 == 0:
        y2buf, y2 = out_rows(M, C, C + 4, 8)
        bits = torch.full((M * C // 32 + 4,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
        k_scale_shift_act(xbuf, 4, C + 8, p['scale'], p['shift'], rbuf, 8, C + 12, y2buf, 8, C + 4, M, C, a, slope, bits=bits)
        torch.cuda.synchronize()
        assert torch.equal(y2buf.view(torch.int32), ybuf.view(torch.int32)), (lab, 'the bits form writes another y')
        assert bool((bits[M * C // 32:] == 0x5a5a5a5a).all()), (lab, 'bits tail')
    for r0, r1 in (chunks or BC.row_chunks(M, C)):
        ref, S, pre = BC.scale_shift_act(x[r0:r1], p['scale'], p['shift'], None if res is None else r[r0:r1], a, slope)
        assert cmp('elem', lab + ' scale_shift_act', y[r0:r1], ref, S) == 0, lab
        if bits is not None:
            # (the generator left no pre-activation near 0, so the sign of the fp32 result is the sign of the float64 one)
            assert torch.equal(bits[r0 * C // 32: r1 * C // 32], BC.pack_bits(ref > 0)), (lab, 'bits')
    assert outside_unchanged(ybuf, before, 8, C + 4, M, C) == 0, (lab, 'outside y')
    if not stats:
        return
    G = BC.col_stats_groups(M)
    st = sentinel((G + 1) * 2 * C)
    k_col_stats(xbuf, 4, M, C, C + 8, st)
    torch.cuda.synchronize()
    ref, mag = BC.col_stats(x)
    got = st[:G * 2 * C].view(G, 2, C)
    assert cmp('colstats', lab + ' col_stats', got, ref, mag) == 0, lab
    assert bool((st[G * 2 * C:] == SENT).all()), (lab, 'stats tail')
    for running, saved in ((True, True), (False, False), (True, False), (False, True)):
        stc = st.clone()                                           # (above 256 rows the first stage overwrites the partials)
        g = torch.Generator(device=DEV).manual_seed(M + C)
        rmean, rvar = ((0.3 * torch.randn(C, generator=g, device=DEV), 0.5 + torch.rand(C, generator=g, device=DEV)) if running
                       else (None, None))
        fin = BC.bn_finalize(got, float(M), p['gamma'], p['beta'], rmean, rvar, 0.1, BC.EPS)
        o = {k: sentinel(C + 4) for k in ('scale', 'shift', 'mean', 'invstd')}
        if running:
            o['rmean'], o['rvar'] = torch.cat([rmean, sentinel(4)]), torch.cat([rvar, sentinel(4)])
        k_bn_finalize(stc, G, C, float(M), p['gamma'], p['beta'], o.get('rmean'), o.get('rvar'), 0.1, BC.EPS, o['scale'], o['shift'],
                      o['mean'] if saved else None, o['invstd'] if saved else None)
        torch.cuda.synchronize()
        for k, t in o.items():
            if k in ('mean', 'invstd') and not saved:
                assert bool((t == SENT).all())
                continue
            assert cmp('finalize', lab + ' bn_finalize ' + k, t[:C], fin[k][0], fin[k][1]) == 0, (lab, k)
            assert bool((t[C:] == SENT).all()), (lab, k, 'tail')
        assert bool((stc[G * 2 * C:] == SENT).all()), (lab, 'stats tail after finalize')


@pytest.mark.parametrize('M,C', BC.ROW_CASES)
def test_forward_rows(M, C):
    assert channel_lanes(4) == 1 and channel_lanes(36) == 16 and channel_lanes(64) == 16 and channel_lanes(260) == 64
    assert -(-(260 // 4) // 64) == 2 and 260 // 4 - 64 == 1           # C = 260: a second channel block with one live lane
    assert [BC.col_stats_groups(m) for m in (1, 17, 513, 2083, 16400)] == [1, 1, 2, 5, 33]
    for i, (a, slope) in enumerate(ACTS):
        for kind in ('rows', 'rows_res'):
            c = BC.gen_case(kind, (M, C), a, slope, DEV)
            check_forward_rows(c, M, C, a, slope, label_of((M, C), a, slope) + (' res' if c['res'] is not None else ''),
                               stats=(i == 0 and kind == 'rows'))


@pytest.mark.parametrize('M', BC.FOLD_ROWS)
def test_statistics_on_both_sides_of_the_two_stage_fold(M):
    """G = 256 partial rows: one stage; G = 257: the first stage folds them into 16 (fp32) rows"""
    assert BC.col_stats_groups(M) == (256 if M == 131072 else 257)
    c = BC.gen_case('rows', (M, 8), ACT_NONE, 0.0, DEV)
    check_forward_rows(c, M, 8, ACT_NONE, 0.0, label_of((M, 8), 0, 0.0))


@pytest.mark.parametrize('C,ldx,xoff', BC.SCALAR_CASES)
def test_scale_shift_act_scalar_fallback(C, ldx, xoff):
    """C % 4 != 0, a pointer one float off a 16-byte boundary, an odd pitch: the scalar kernel, same contract"""
    M = BC.SCALAR_ROWS
    for a, slope in ACTS:
        c = BC.gen_case('rows_res', (M, C), a, slope, DEV)
        p = c['p']
        assert c['ambiguous'] == 0
        xbuf = sentinel(xoff + (M + 2) * ldx)
        x = view2(xbuf, xoff, ldx, M, C)
        x.copy_(c['raw'])
        rbuf, r = place(c['res'], C + 3, 0)
        ybuf, y = out_rows(M, C, C + 2, 5)
        before = ybuf.clone()
        k_scale_shift_act(xbuf, xoff, ldx, p['scale'], p['shift'], rbuf, 0, C + 3, ybuf, 5, C + 2, M, C, a, slope)
        torch.cuda.synchronize()
        ref, S, _ = BC.scale_shift_act(x, p['scale'], p['shift'], r, a, slope)
        lab = label_of((M, C, ldx, xoff), a, slope) + ' scalar'
        assert cmp('elem', lab, y, ref, S) == 0, lab
        assert outside_unchanged(ybuf, before, 5, C + 2, M, C) == 0, lab
        # without scale / shift / residual: a bare activation
        k_scale_shift_act(xbuf, xoff, ldx, None, None, None, 0, 0, ybuf, 5, C + 2, M, C, a, slope)
        torch.cuda.synchronize()
        ref, S, _ = BC.scale_shift_act(x, None, None, None, a, slope)
        assert cmp('elem', lab + ' bare', y, ref, S) == 0, lab


@pytest.mark.parametrize('a,slope', BC.LARGE_ACTS[BC.SCALAR_STRIDE])
def test_scale_shift_act_scalar_fallback_beyond_one_grid(a, slope):
    """the scalar kernel strides over elements, not quads: M*C above 16 384 x 256 for its second trip"""
    M, C = BC.SCALAR_STRIDE
    assert C % 4 != 0 and -(-M * C // (16384 * 256)) == 2
    c = BC.gen_case('rows_res', (M, C), a, slope, DEV)
    assert c['ambiguous'] == 0
    p = c['p']
    ybuf, y = out_rows(M, C, C + 2, 5)
    before = ybuf.clone()
    k_scale_shift_act(c['raw'], 0, C, p['scale'], p['shift'], c['res'], 0, C, ybuf, 5, C + 2, M, C, a, slope)
    torch.cuda.synchronize()
    lab = label_of((M, C), a, slope) + ' scalar'
    for r0, r1 in BC.row_chunks(M, C):
        ref, S, _ = BC.scale_shift_act(c['raw'][r0:r1], p['scale'], p['shift'], c['res'][r0:r1], a, slope)
        assert cmp('elem', lab, y[r0:r1], ref, S) == 0, lab
    assert outside_unchanged(ybuf, before, 5, C + 2, M, C) == 0, lab


def test_scale_shift_act_aliasing_the_model_uses():
    """in place (y == x, as layers.py calls it), and a residual that is the other channel slice of the output's own buffer"""
    M, C = BC.ALIAS_CASE
    for a, slope in ACTS:
        c = BC.gen_case('rows_res', (M, C), a, slope, DEV)
        assert c['ambiguous'] == 0
        p = c['p']
        buf = sentinel(4 + (M + 2) * 2 * C)
        xy, r = view2(buf, 4, 2 * C, M, C), view2(buf, 4 + C, 2 * C, M, C)
        xy.copy_(c['raw'])
        r.copy_(c['res'])
        x0, before = c['raw'].clone(), buf.clone()
        k_scale_shift_act(buf, 4, 2 * C, p['scale'], p['shift'], buf, 4 + C, 2 * C, buf, 4, 2 * C, M, C, a, slope)
        torch.cuda.synchronize()
        ref, S, _ = BC.scale_shift_act(x0, p['scale'], p['shift'], c['res'], a, slope)
        lab = label_of((M, C), a, slope) + ' in place, residual in the other slice'
        assert cmp('elem', lab, xy, ref, S) == 0, lab
        assert outside_unchanged(buf, before, 4, 2 * C, M, C) == 0, lab


def test_nan_stays_nan_under_every_activation():
    """a diverged network must not look healthy: NaN statistics or a NaN input leave NaN, not a clean 0, under ReLU too; the mask bit of
    a NaN is 0; every other element is what it was"""
    M, C = BC.NAN_CASE
    for a, slope in ACTS:
        c = BC.gen_case('rows', (M, C), a, slope, DEV)
        assert c['ambiguous'] == 0
        p = c['p']
        raw = c['raw'].clone()
        raw[3, 5] = raw[66, 63] = raw[10, 0] = float('nan')
        scale = p['scale'].clone()
        scale[17] = float('nan')                                   # a whole channel whose statistics are NaN
        y = sentinel(M * C).view(M, C)
        bits = torch.zeros(M * C // 32, dtype=torch.int32, device=DEV)
        k_scale_shift_act(raw, 0, C, scale, p['shift'], None, 0, 0, y, 0, C, M, C, a, slope, bits=bits)
        y1 = sentinel(M * C).view(M, C)
        k_scale_shift_act(raw, 0, C, scale, p['shift'], None, 0, 0, y1, 0, C, M, C, a, slope)
        torch.cuda.synchronize()
        ref, S, _ = BC.scale_shift_act(raw, scale, p['shift'], None, a, slope)
        bad = torch.isnan(ref)
        assert int(bad.sum()) == M + 3
        lab = label_of((M, C), a, slope) + ' NaN'
        for got in (y, y1):
            assert torch.equal(torch.isnan(got), bad), lab
            assert cmp('elem', lab, got[~bad], ref[~bad], S[~bad]) == 0, lab
        assert torch.equal(bits, BC.pack_bits(ref > 0)), lab
        assert not bool(BC.unpack_bits(bits, M, C)[bad].any()), lab


# ------------------------------------------------------------------------------------------------ backward, [M][C]
def backward_inputs(c, a, slope):
    """the activation a layer kept (fp32 of the reference forward) and the three mask sources' common answer"""
    p = c['p']
    ref, _, pre = BC.scale_shift_act(c['raw'], p['scale'], p['shift'], None, a, slope)
    return ref.float(), pre > 0


def check_reduce(c, M, C, a, slope, src, lab, full=True):
    p = c['p']
    G = bwd_groups(M)
    assert lib_query('efgh_bwd_groups', i64(M)) == G
    y32, pos = backward_inputs(c, a, slope)
    dybuf, dy = place(c['dy'], C + 4, 4)
    rawbuf, raw = place(c['raw'], C + 8, 8)
    out = sums_out(G, C)
    mean, invstd = (p['mean'], p['invstd']) if full else (None, None)
    if src == 'y':
        ybuf, _ = place(y32, C + 12, 4)
        k_reduce(dybuf, 4, C + 4, ybuf, 4, C + 12, rawbuf if full else None, 8, C + 8, mean, invstd, None, None, M, C, a, slope, out)
        pos = y32 > 0
    elif src == 'bits':
        bits = BC.pack_bits(pos)
        k_reduce(dybuf, 4, C + 4, bits, 0, 0, rawbuf if full else None, 8, C + 8, mean, invstd, None, None, M, C, a, slope, out)
    else:
        k_reduce(dybuf, 4, C + 4, None, 0, 0, rawbuf, 8, C + 8, mean, invstd, p['scale'], p['shift'], M, C, a, slope, out)
    s, bnd = BC.act_bn_bwd_reduce(dy, pos, raw, mean, invstd, a, slope)
    check_sums(lab + ' reduce/' + src, out, s, bnd, float(M), C, full=full)
    return s


def check_apply(c, M, C, a, slope, src, lab, form='full', chunks=None):
    """form: full (train BatchNorm, draw and dres) | draw (no dres) | dres (no draw) | coef (mean == NULL) | plain (no coef either)"""
    p = c['p']
    y32, pos = backward_inputs(c, a, slope)
    dybuf, dy = place(c['dy'], C + 4, 4)
    rawbuf, raw = place(c['raw'], C + 8, 8)
    g = torch.Generator(device=DEV).manual_seed(M + C)
    m1 = (0.05 * torch.randn(C, generator=g, device=DEV)).double()         # (any means: the apply pass takes them as inputs)
    m2 = (0.05 * torch.randn(C, generator=g, device=DEV)).double()
    train = form in ('full', 'draw', 'dres')
    want_draw, want_dres = form != 'dres', form in ('full', 'dres')
    dwbuf, dw = out_rows(M, C, C + 16, 12)                                  # (lddraw != lddy)
    drbuf, dr = out_rows(M, C, C + 8, 4)
    b_dw, b_dr = dwbuf.clone(), drbuf.clone()
    mean, invstd = (p['mean'], p['invstd']) if train else (None, None)
    coef = None if form == 'plain' else p['scale']
    rawarg, m1arg, m2arg = rawbuf if (train or src == 'raw') else None, m1 if train else None, m2 if train else None
    ysrc, yoff, ldy, psc, psh = None, 0, 0, None, None
    if src == 'y':
        ysrc, _ = place(y32, C + 12, 4)
        yoff, ldy, pos = 4, C + 12, y32 > 0
    elif src == 'bits':
        ysrc = BC.pack_bits(pos)
    else:
        psc, psh = p['scale'], p['shift']
    k_apply(dybuf, 4, C + 4, ysrc, yoff, ldy, rawarg, 8, C + 8, mean, invstd, coef, m1arg, m2arg, psc, psh, M, C, a, slope,
            dwbuf if want_draw else None, 12, C + 16, drbuf if want_dres else None, 4, C + 8)
    torch.cuda.synchronize()
    lab = lab + ' apply/%s/%s' % (src, form)
    for r0, r1 in (chunks or BC.row_chunks(M, C)):
        draw, S, dres, S_dres = BC.act_bn_bwd_apply(dy[r0:r1], pos[r0:r1], raw[r0:r1], mean, invstd, coef, m1, m2, a, slope)
        if want_draw:
            if form == 'plain':
                assert cmp('exact', lab, dw[r0:r1][S == 0], draw[S == 0], None) == 0, lab
            assert cmp('elem', lab + ' draw', dw[r0:r1], draw, S) == 0, lab
        if want_dres:
            copy = S_dres == 0
            assert cmp('exact', lab, dr[r0:r1][copy], dres[copy], None) == 0, (lab, 'dres is a copy where the derivative is 1 or 0')
            assert cmp('elem', lab + ' dres', dr[r0:r1], dres, S_dres) == 0, lab
    assert outside_unchanged(dwbuf, b_dw, 12, C + 16, M, C) == 0 and outside_unchanged(drbuf, b_dr, 4, C + 8, M, C) == 0, lab
    if not want_draw:
        assert torch.equal(dwbuf, b_dw), lab
    if not want_dres:
        assert torch.equal(drbuf, b_dr), lab


@pytest.mark.parametrize('M,C', BC.ROW_CASES)
def test_backward_rows(M, C):
    assert [bwd_groups(m) for m in (1, 17, 2083, 16400)] == [1, 2, 131, 513] and bwd_rows_per_group(16400) == 32
    # G = 131: ty = 0 .. 2 run the four-way unrolled trip of the fold (g + 96 < G), the other lanes only its tail
    assert sum(1 for ty in range(32) if ty + 96 < 131) == 32 and 128 + 3 == 131
    for i, (a, slope) in enumerate(ACTS):
        c = BC.gen_case('rows', (M, C), a, slope, DEV)
        assert c['ambiguous'] == 0
        lab = label_of((M, C), a, slope)
        for src in ['y', 'raw'] + (['bits'] if C % 32 == 0 else []):
            check_reduce(c, M, C, a, slope, src, lab)
            check_apply(c, M, C, a, slope, src, lab)
        check_reduce(c, M, C, a, slope, 'y', lab + ' (no mean)', full=False)
        for form in ('draw', 'dres', 'coef', 'plain'):
            check_apply(c, M, C, a, slope, ['y', 'raw'][i % 2], lab, form=form)
    # the fold of fp32 partial rows (what an MFMA epilogue leaves): G rows of this case
    G = bwd_groups(M)
    g = torch.Generator(device=DEV).manual_seed(G + C)
    st = torch.randn((G, 2, C), generator=g, device=DEV) * (1 + 30 * torch.rand(C, generator=g, device=DEV))
    out = sums_out(1, C)
    k_bwd_finalize_f32(st, G, C, float(M), out)
    s, bnd = BC.bwd_finalize_f32(st, float(M))
    check_sums(label_of((M, C), 0, 0) + ' bwd_finalize_f32', out, s, bnd, float(M), C)


# ------------------------------------------------------------------------------------------------ pooled launches
def pooled_outputs(c, a, slope):
    """the fp32 tensors a layer keeps: the full-resolution activation and the pooled one (fp32 of the reference)"""
    p = c['p']
    B, H, W, C = c['raw'].shape
    y = BC.scale_shift_act(c['raw'].view(-1, C), p['scale'], p['shift'], None, a, slope)[0].float().view(B, H, W, C)
    return y


def check_pool_forward(c, shape, a, slope, lab):
    B, H, W, C = shape
    p, raw, dyp = c['p'], c['raw'], c['dy_pool']
    Ho, Wo = H // 2, W // 2
    n = B * Ho * Wo * C
    yfull = pooled_outputs(c, a, slope)
    # plain max pool and its vertical half over the materialised activation: copies, bit-exact
    yp = sentinel(n + 64)
    k_pool('efgh_maxpool2', yfull, yp, B, H, W, C)
    yv = sentinel(B * Ho * W * C + 64)
    k_pool('efgh_maxpool_v2', yfull, yv, B, H, W, C)
    ya = sentinel(n + 64)
    k_maxpool2_affine(raw, p['scale'], p['shift'], a, slope, ya, B, H, W, C)
    dx = torch.cat([torch.zeros(B * H * W * C, device=DEV), sentinel(64)])         # (the caller zeroes dx: the odd rim stays zero)
    k_maxpool2_bwd(yfull, dyp, dx, B, H, W, C)
    dxa = sentinel(B * H * W * C + 64)
    k_maxpool2_bwd_affine(raw, p['scale'], p['shift'], a, slope, dyp, dxa, B, H, W, C)
    torch.cuda.synchronize()
    for t, k in ((yp, n), (yv, B * Ho * W * C), (ya, n), (dx, B * H * W * C), (dxa, B * H * W * C)):
        assert bool((t[k:] == SENT).all()), (lab, 'tail')
    yp, yv, ya = yp[:n].view(B, Ho, Wo, C), yv[:B * Ho * W * C].view(B, Ho, W, C), ya[:n].view(B, Ho, Wo, C)
    dx, dxa = dx[:B * H * W * C].view(B, H, W, C), dxa[:B * H * W * C].view(B, H, W, C)
    for b in range(B):
        s = slice(b, b + 1)
        assert cmp('exact', lab, yp[s], BC.maxpool2(yfull[s]), None) == 0, (lab, 'maxpool2')
        assert cmp('exact', lab, yv[s], BC.maxpool_v2(yfull[s]), None) == 0, (lab, 'maxpool_v2')
        ref, S = BC.maxpool2_affine(raw[s], p['scale'], p['shift'], a, slope)
        assert cmp('elem', lab + ' maxpool2_affine', ya[s], ref, S) == 0, (lab, 'maxpool2_affine')
        assert cmp('exact', lab, dx[s, :2 * Ho, :2 * Wo], BC.maxpool2_bwd(yfull[s], dyp[s]), None) == 0, (lab, 'maxpool2_bwd')
        assert cmp('exact', lab, dxa[s, :2 * Ho, :2 * Wo], BC.maxpool2_bwd_affine(raw[s], p['scale'], p['shift'], a, slope, dyp[s]),
                   None) == 0, (lab, 'maxpool2_bwd_affine')
    assert bool((dx[:, 2 * Ho:] == 0).all()) and bool((dx[:, :, 2 * Wo:] == 0).all()), (lab, 'the odd rim of dx must stay zero')
    assert bool((dxa[:, 2 * Ho:] == SENT).all()) and bool((dxa[:, :, 2 * Wo:] == SENT).all()), (lab, 'the odd rim is not written')


def pool_groups(B, H, W):
    return bwd_groups(B * ((H + 1) // 2) * ((W + 1) // 2))


def check_pool_reduce(c, shape, a, slope, lab, pooled=False):
    B, H, W, C = shape
    p, raw, dyp = c['p'], c['raw'], c['dy_pool']
    count = float(B * H * W)
    if not pooled:
        G = pool_groups(B, H, W)
        assert lib_query('efgh_pool_bwd_groups', i32(B), i32(H), i32(W)) == G
        out = sums_out(G, C)
        k_pool_reduce(dyp, raw, p, B, H, W, C, a, slope, out)
        s, bnd = BC.pool_bn_bwd_reduce(dyp, raw, p['mean'], p['invstd'], p['scale'], p['shift'], a, slope)
        check_sums(lab + ' pool_bn_bwd_reduce', out, s, bnd, count, C)
        return out, s, bnd
    assert a == ACT_RELU
    G = bwd_groups(B * (H // 2) * (W // 2))
    y_pool = torch.empty((B, H // 2, W // 2, C), device=DEV)
    for b in range(B):
        y_pool[b] = BC.maxpool2_affine(raw[b:b + 1], p['scale'], p['shift'], a, slope)[0][0].float()
    out = sums_out(G, C)
    k_pool_reduce(dyp, raw, p, B, H, W, C, a, slope, out, y_pool=y_pool)
    s, bnd = BC.pool_bn_bwd_reduce_pooled(dyp, y_pool, raw, p['mean'], p['invstd'], p['scale'], p['shift'])
    check_sums(lab + ' pool_bn_bwd_reduce_pooled', out, s, bnd, count, C)
    return out, s, bnd


def check_pool_apply(c, shape, a, slope, lab):
    B, H, W, C = shape
    p, raw, dyp = c['p'], c['raw'], c['dy_pool']
    g = torch.Generator(device=DEV).manual_seed(B * H * W + C)
    m1 = (0.05 * torch.randn(C, generator=g, device=DEV)).double()
    m2 = (0.05 * torch.randn(C, generator=g, device=DEV)).double()
    n = B * H * W * C
    dw = sentinel(n + 64)
    k_pool_apply(dyp, raw, p, m1, m2, B, H, W, C, a, slope, dw)
    torch.cuda.synchronize()
    assert bool((dw[n:] == SENT).all()), (lab, 'tail')
    dw = dw[:n].view(B, H, W, C)
    for b in range(B):
        s = slice(b, b + 1)
        ref, S = BC.pool_bn_bwd_apply(dyp[s], raw[s], p['mean'], p['invstd'], p['scale'], m1, m2, p['scale'], p['shift'], a, slope)
        assert cmp('elem', lab + ' pool_bn_bwd_apply', dw[s], ref, S) == 0, (lab, 'pool_bn_bwd_apply')


def report_pooled(c, shape, lab):
    """section 4 of the issue: the m2 of both pooled reductions against the from-raw float64 sum, over sum |d||xhat| / count, by
    parameter set"""
    B, H, W, C = shape
    p = c['p']
    count = float(B * H * W)
    out_y, _, _ = check_pool_reduce(c, shape, ACT_RELU, 0.0, lab, pooled=True)
    out_r, s, bnd = check_pool_reduce(c, shape, ACT_RELU, 0.0, lab)
    torch.cuda.synchronize()
    worst = 0.0
    for name, out in (('from y', out_y), ('from raw', out_r)):
        ratio = (out['m2'][:C] - s[1] / count).abs() / (bnd[1] / count + 1e-300)
        for k in range(6):
            sel = (p['sets'] == k) & (bnd[1] > 0)
            if bool(sel.any()):
                v = float(ratio[sel].max())
                key = (name, k)
                if v > POOLED_REPORT.get(key, (-1, ''))[0]:
                    POOLED_REPORT[key] = (v, lab)
                worst = max(worst, v)
    return worst


@pytest.mark.parametrize('shape', BC.POOL_CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_pooled_launches(shape):
    B, H, W, C = shape
    worst = 0.0
    for a, slope in ACTS:
        c = BC.gen_case('pool', shape, a, slope, DEV)
        assert c['ambiguous'] == 0
        lab = label_of(shape, a, slope)
        check_pool_forward(c, shape, a, slope, lab)
        check_pool_reduce(c, shape, a, slope, lab)
        check_pool_apply(c, shape, a, slope, lab)
        if a == ACT_RELU:
            worst = report_pooled(c, shape, lab)
    # both formulations of the pooled sums serve the same gradient: on the ordinary scale sum |d||xhat| they meet the m1 / m2 ceiling
    assert worst <= BC.CEIL['m'], (shape, 'm2 of a pooled reduction over sum |d||xhat| / count', worst)


def test_pooled_reduction_on_both_sides_of_its_fallback_bound():
    """efgh_pool_bn_bwd_reduce_pooled at |beta|/|gamma| = 1.9 (xhat from y_pool) and 6, 8, 64 (xhat from raw), with a one-signed pooled
    gradient - the rounding of beta is common to a channel's terms and does not average out: the mean of dpre*xhat stays within the
    m1 / m2 ceiling of the from-raw float64 sum, on sum |d||xhat| / count.  (Measured without the bound: 1.9 x 2^-24 at 2, 3.9 at 4,
    50 at 64 - a bound of 8 or more fails here, one of 4 does not: at 3 - 4 the error is within a rounding of the ceiling; with every channel from raw the 1.9 channels would still pass, which is what the
    traffic argument, not this test, decides.)"""
    shape = BC.POOL_RATIO
    B, H, W, C = shape
    c = BC.gen_case('pool_ratio', shape, ACT_RELU, 0.0, DEV)
    assert c['ambiguous'] == 0 and bool((c['dy_pool'] >= 0).all())
    p = c['p']
    fr = BC.pooled_from_raw(p['mean'], p['invstd'], p['scale'], p['shift'])
    assert torch.equal(fr, p['ratio'] > BC.POOLED_BETA_GAMMA) and bool(fr.any()) and bool((~fr).any())
    lab = label_of(shape, ACT_RELU, 0.0) + ' one-signed'
    out, _, _ = check_pool_reduce(c, shape, ACT_RELU, 0.0, lab, pooled=True)
    s, bnd = BC.pool_bn_bwd_reduce(c['dy_pool'], c['raw'], p['mean'], p['invstd'], p['scale'], p['shift'], ACT_RELU, 0.0)
    count = float(B * H * W)
    ratio = (out['m2'][:C] - s[1] / count).abs() / (bnd[1] / count + 1e-300)
    for r in sorted(set(BC.RATIOS)):
        sel = (p['ratio'] == r) & (bnd[1] > 0)
        assert bool(sel.any()), r
        RATIO_REPORT[r] = float(ratio[sel].max())
        assert RATIO_REPORT[r] <= BC.CEIL['m'], (r, RATIO_REPORT[r] / BC.U)


# ------------------------------------------------------------------------------------------------ grid-stride and non-temporal sizes
def large_rows(shape, a, slope):
    key = ('rows', shape, a, slope)
    if key not in _LARGE:
        _LARGE.clear()
        torch.cuda.empty_cache()
        if shape == BC.ROWS_NT:            # the 384 MiB tensor of the pooled non-temporal case, as rows
            c = BC.gen_case('pool', BC.POOL_NT, a, slope, DEV)
            _LARGE[key] = dict(p=c['p'], raw=c['raw'].view(*shape), dy=BC._randn(shape, 11, DEV), res=None, ambiguous=c['ambiguous'])
        else:
            _LARGE[key] = BC.gen_case('rows', shape, a, slope, DEV)
    return _LARGE[key]


def large_pool(shape, a, slope):
    key = ('pool', shape, a, slope)
    if key not in _LARGE:
        _LARGE.clear()
        torch.cuda.empty_cache()
        _LARGE[key] = BC.gen_case('pool', shape, a, slope, DEV)
    return _LARGE[key]


_ROWS_LARGE = [(sh, a, s, part) for sh in (BC.ROWS_STRIDE, BC.ROWS_NT) for a, s in BC.LARGE_ACTS[sh]
               for part in ('forward', 'reduce', 'apply')]


@pytest.mark.parametrize('shape,a,slope,part', _ROWS_LARGE, ids=lambda v: str(v).replace(' ', ''))
def test_rows_beyond_one_grid_and_at_the_non_temporal_threshold(shape, a, slope, part):
    M, C = shape
    assert grid_trips(M * C // 4) >= 2                                  # the grid-stride loop takes more than one trip
    assert (M * C * 4 >= BC.NT_BYTES) == (shape == BC.ROWS_NT) and (shape != BC.ROWS_NT or M * C * 4 == BC.NT_BYTES)
    c = large_rows(shape, a, slope)
    assert c['ambiguous'] == 0
    lab = label_of(shape, a, slope)
    src = 'bits' if shape == BC.ROWS_NT else 'raw'
    if part == 'forward':
        check_forward_rows(c, M, C, a, slope, lab)
    elif part == 'reduce':
        check_reduce(c, M, C, a, slope, src, lab)
    else:
        check_apply(c, M, C, a, slope, src, lab)


_POOL_LARGE = [(BC.POOL_STRIDE, 'forward'), (BC.POOL_STRIDE, 'reduce'), (BC.POOL_STRIDE, 'apply'),
               (BC.POOL_NT, 'forward'), (BC.POOL_NT, 'reduce'), (BC.POOL_NT, 'apply'), (BC.POOL_NT_POOLED, 'pooled')]


@pytest.mark.parametrize('shape,part', _POOL_LARGE, ids=lambda v: str(v).replace(' ', ''))
def test_pooled_beyond_one_grid_and_at_the_non_temporal_threshold(shape, part):
    B, H, W, C = shape
    a, slope = BC.LARGE_ACTS[shape][0]
    assert grid_trips(B * (H // 2) * (W // 2) * C // 4) >= 2
    nbytes = B * H * W * C * 4
    assert {BC.POOL_STRIDE: nbytes < BC.NT_BYTES, BC.POOL_NT: nbytes == BC.NT_BYTES, BC.POOL_NT_POOLED: nbytes == 4 * BC.NT_BYTES}[shape]
    c = large_pool(shape, a, slope)
    assert c['ambiguous'] == 0
    lab = label_of(shape, a, slope)
    if part == 'forward':
        check_pool_forward(c, shape, a, slope, lab)
    elif part == 'reduce':
        check_pool_reduce(c, shape, a, slope, lab)
        if a == ACT_RELU:
            check_pool_reduce(c, shape, a, slope, lab, pooled=True)
    elif part == 'apply':
        check_pool_apply(c, shape, a, slope, lab)
    else:
        check_pool_reduce(c, shape, a, slope, lab, pooled=True)


# ------------------------------------------------------------------------------------------------ coverage and the tau table
def test_every_entry_point_ran_and_the_tau_table():
    _LARGE.clear()
    torch.cuda.empty_cache()
    missing = [e for e in BC.ENTRY_POINTS if e not in CALLS]
    assert not missing, 'entry points never called (this test sums up the whole module: run the module, not the test): %s' % missing
    for e in BC.NT_ENTRY_POINTS:
        sizes = CALLS[e]
        assert any(s < BC.NT_BYTES for s in sizes) and any(s >= BC.NT_BYTES for s in sizes), \
            '%s was not called on both sides of the non-temporal threshold' % e
    print('\nclass      observed max |got - ref| / S   ceiling     tau        case')
    for cls in ('elem', 'f64sum', 'm', 'colstats', 'finalize'):
        v, lab = BC.OBSERVED[cls]
        print('%-10s %.3e (%6.2f x 2^-24)      %.3e   %.3e  %s' % (cls, v, v / BC.U, BC.CEIL[cls], BC.TAU_BN[cls], lab))
        assert BC.TAU_BN[cls] <= BC.CEIL[cls]
    print('m2 of the pooled reductions against the from-raw float64 sum, over sum |d||xhat| / count (x 2^-24), by parameter set:')
    names = ['ordinary', 'gamma == 0', 'gamma < 0', 'gamma 1e-3, beta 1', 'constant channel', 'mean/std = 30']
    for (path, k), (v, lab) in sorted(POOLED_REPORT.items()):
        print('  %-9s %-20s %10.3f   %s' % (path, names[k], v / BC.U, lab))
    for r, v in sorted(RATIO_REPORT.items()):
        print('  from y / raw at |beta|/|gamma| = %-5g %10.3f   %s one-signed' % (r, v / BC.U, 'x'.join(map(str, BC.POOL_RATIO))))
    print('calls: ' + ', '.join('%s %d' % (e, len(CALLS[e])) for e in BC.ENTRY_POINTS))
