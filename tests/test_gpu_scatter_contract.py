"""The BCL splat and its backward, the adjoint of the neighbour gather (gather and atomic scatter) and the segment reductions with their
backward passes against the float64 contract of tests/scatter_contract.py: direct calls of the ten C entry points through ops._L()
on generated arrays (no lattice build) at the smallest shapes at which each mechanism can go wrong - every lane mapping of the splat
(16, 32, 64 and the automatic choice), chunk counts that do not divide the lanes and both sides of every limit, vertex counts around a
block and around the band mapping of the blocks, list lengths around one trip of each mapping, empty lists next to long ones, both
values of normalize, pitches larger than the rows; every table width of the adjoint with none, one, many and alias_cap alias records;
the segment maximum with empty segments, ties, -inf and NaN in both forms.  Every output lies inside a larger sentinel-filled buffer
whose other elements must stay bit-unchanged; inputs are padded with values that would show in the result if they were read.  The
ceilings are derived in the contract, not measured.  The last test asserts that all ten entry points ran and prints the largest
observed |got - ref| / (ceiling x S) per class.

On the MI355X (71 tests), largest |got - ref| / (ceiling x S) per class:  splat 0.50 (32 lanes, 17 chunks, normalize 0), wsum 0.31,
splat backward 0.26, adjoint gather 0.17 (C 512, 64 alias records), atomic scatter 0.75 (C 512, H 1; the order of the atomics varies),
segment mean 0.15, its backward 0.49; the segment maximum and its backward are bit-exact."""
import pytest
import torch

import scatter_contract as SC
from bn_contract import outside_unchanged, view2
from scatter_contract import cmp

pytestmark = pytest.mark.gpu

SENT = -7777.0
POISON = 1e30            # padding of the inputs: shows in any sum that reads it
DEV = 'cuda'
CALLS = {}
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


def sentinel(n, dtype=torch.float32, value=SENT):
    return torch.full((int(n),), value, dtype=dtype, device=DEV)


def place(t, ld, off, tail=2, value=SENT):
    """t [M][C] (CPU or GPU) inside a 1-D buffer filled with `value`: pitch ld, first element at `off`, `tail` rows behind"""
    M, C = t.shape
    buf = sentinel(off + (M + tail) * ld, t.dtype, value)
    view2(buf, off, ld, M, C).copy_(t)
    return buf


def out_rows(M, C, ld, off, tail=2, dtype=torch.float32):
    buf = sentinel(off + (M + tail) * ld, dtype)
    return buf, view2(buf, off, ld, M, C)


def dev(t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).contiguous().to(DEV)


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def sync_ok(rc):
    assert rc == 0, (rc, L().efgh_last_error())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ splat forward
class SplatArrays:
    """one generated case on the device: feat at pitch Cf + 4 with poisoned pad columns"""

    def __init__(self, a):
        self.a, self.H, self.n, self.Cf = a, a['H'], a['n'], a['Cf']
        self.ldf = self.Cf + 4
        self.feat = place(a['feat'], self.ldf, 8, value=POISON)
        self.emg = dev(a['emg'])
        self.bary, self.lst, self.vseg = dev(a['bary_pm']), dev(a['lst']), dev(a['vseg'])
        self.C = self.Cf + (4 if a['emg'] is not None else 0)
        self.avg = max(1, 4 * self.n // self.H)

    def run(self, lanes, normalize, avg_len=None):
        """-> (splat buffer, wsum buffer, their views, rc)"""
        sb, sv = out_rows(self.H, self.C, self.C, 8)
        wb = sentinel(3 + self.H + 5)
        rc = L().efgh_splat_gather(P(self.emg), P(self.feat, 8), self.ldf, self.Cf, P(self.bary), P(self.lst), P(self.vseg), self.H,
                                   self.avg if avg_len is None else avg_len, lanes, normalize, P(sb, 8), P(wb, 3), st())
        torch.cuda.synchronize()
        return sb, wb, sv, wb[3:3 + self.H], rc


def _check_splat(label, arr, refs, lanes):
    for nz in (0, 1):
        sb, wb, sv, wv, rc = arr.run(lanes, nz)
        assert rc == 0, (label, rc)
        r = refs[nz]
        lab = '%s normalize %d' % (label, nz)
        assert cmp('splat', lab, sv.cpu(), r['ref'], r['bound']) == 0, lab
        assert cmp('splat_wsum', lab, wv.cpu(), r['wsum'], r['wsum_bound']) == 0, lab
        empty = (r['L'] == 0).to(DEV)
        assert bool((sv[empty] == 0).all()) and bool((wv[empty] == 0).all()), lab       # exact zeros, with either normalize
        assert outside_unchanged(sb, sentinel(sb.numel()), 8, arr.C, arr.H, arr.C) == 0, lab
        assert outside_unchanged(wb, sentinel(wb.numel()), 3, arr.H, 1, arr.H) == 0, lab
        sb2, wb2, _, _, rc = arr.run(lanes, nz)
        assert rc == 0 and bits_equal(sb, sb2) and bits_equal(wb, wb2), lab + ': two runs differ'


_LANE_CH = sorted({c[:2] for c in SC.splat_cases()})


@pytest.mark.parametrize('lanes,CH', _LANE_CH)
def test_splat_gather_every_mapping_chunk_count_vertex_count_and_list_length(lanes, CH):
    cases = [c for c in SC.splat_cases() if c[:2] == (lanes, CH)]
    assert cases
    seen = set()
    for _, _, emg, Cf, H in cases:
        a, margin, refs = SC.gen_splat_case(CH, emg, Cf, H)
        assert margin >= SC.MIN_TERM
        seen |= set(a['lengths'])
        _check_splat('lanes %d CH %d emg %d H %d' % (lanes, CH, emg, H), SplatArrays(a), refs, lanes)
    want = set(SC.PROFILE) - {129}
    assert want <= seen and any(129 <= v <= 132 for v in seen), sorted(want - seen)


@pytest.mark.parametrize('CH', [32, 33])
@pytest.mark.parametrize('avg_len', [32, 33])
def test_splat_gather_automatic_mapping_is_the_one_the_header_names(CH, avg_len):
    a, _, refs = SC.gen_splat_case(CH, 0, 4 * CH, 139)
    arr = SplatArrays(a)
    want = 32 if (CH <= 32 and avg_len <= 32) else 64
    for nz in (0, 1):
        sb, wb, sv, wv, rc = arr.run(0, nz, avg_len=avg_len)
        assert rc == 0
        eb, ewb, _, _, rc = arr.run(want, nz)
        assert rc == 0 and bits_equal(sb, eb) and bits_equal(wb, ewb), (CH, avg_len, want)
        assert cmp('splat', 'lanes 0 CH %d avg_len %d' % (CH, avg_len), sv.cpu(), refs[nz]['ref'], refs[nz]['bound']) == 0


# ------------------------------------------------------------------------------------------------ splat backward
@pytest.mark.parametrize('n,Cf', SC.SPLAT_BWD_CASES)
def test_splat_bwd(n, Cf):
    a = SC.gen_splat_bwd_case(n, Cf)
    H = a['H']
    g = torch.Generator().manual_seed(n)
    bary, off = dev(a['bary_pm']), dev(a['off_pm'])
    for coff in (0, 4):
        C = coff + Cf + 4                                   # the slice [coff, coff + Cf) ends before the row does
        gs = SC.signed((H, C), g)
        gsd = dev(gs)
        for nz in (0, 1):
            wsum = SC.splat(None, a['feat'], Cf, a['bary_pm'], a['lst'], a['vseg'], H, nz)['wsum'].float()
            ld = Cf + 4
            buf, view = out_rows(n, Cf, ld, 4)
            sync_ok(L().efgh_splat_bwd(P(gsd), C, coff, P(dev(wsum)), Cf, P(bary), P(off), n, P(buf, 4), ld, nz, st()))
            ref, bound = SC.splat_bwd(gs, coff, wsum, Cf, a['bary_pm'], a['off_pm'], nz)
            lab = 'n %d Cf %d coff %d normalize %d' % (n, Cf, coff, nz)
            assert cmp('splat_bwd', lab, view.cpu(), ref, bound) == 0, lab
            assert outside_unchanged(buf, sentinel(buf.numel()), 4, ld, n, Cf) == 0, lab


# ------------------------------------------------------------------------------------------------ adjoint gather / atomic scatter
@pytest.mark.parametrize('C', SC.ADJ_C)
def test_table_gather_transposed_and_scatter_add(C):
    for _, H, na, cap, fill in [c for c in SC.adj_cases() if c[0] == C]:
        nbr, alist, src, dst0 = SC.gen_adj_case(C, H, na, cap, fill)
        lab = 'C %d H %d n_alias %d cap %d' % (C, H, na, cap)
        nbr_d, src_d = dev(nbr), dev(src)
        n_alias = torch.tensor([na], dtype=torch.int32, device=DEV)
        r = SC.table_adjoint(src, nbr, C)
        assert float(r['alias'].sum()) == na
        outs = []
        for perm in (False, True):
            al = alist.clone()
            if perm and na > 1:
                al[:na] = alist[:na][torch.randperm(na, generator=torch.Generator().manual_seed(na))]
            buf, view = out_rows(H, C, C, 4)
            sync_ok(L().efgh_table_gather_transposed(P(src_d), P(nbr_d), H, C, P(dev(al)), P(n_alias), cap, P(buf, 4), st()))
            assert cmp('adjoint', lab, view.cpu(), r['ref'], r['bound']) == 0, lab
            assert outside_unchanged(buf, sentinel(buf.numel()), 4, C, H, C) == 0, lab
            outs.append(buf)
        assert bits_equal(outs[0], outs[1]), lab + ': the order of the alias records shows'
        # the atomic scatter over the same table, into a non-zero dst
        buf = place(dst0, C, 4)
        before = buf.clone()
        sync_ok(L().efgh_table_scatter_add(P(src_d), P(nbr_d), H, 15, C, P(buf, 4), st()))
        r2 = SC.table_adjoint(src, nbr, C, dst0)
        assert cmp('scatter_add', lab, view2(buf, 4, C, H, C).cpu(), r2['ref'], r2['bound']) == 0, lab
        assert outside_unchanged(buf, before, 4, C, H, C) == 0, lab


# ------------------------------------------------------------------------------------------------ segment maximum
def _colmax(form, xbuf, xoff, ld, C, seg_d, nseg, M, want_arg):
    """form: 'one', or the rows_hint of the two-stage form -> (y buffer, arg buffer or None)"""
    yb = sentinel(5 + nseg * C + 7)
    ab = sentinel(2 + nseg * C + 7, torch.int32, -7777) if want_arg else None
    if form == 'one':
        rc = L().efgh_segment_colmax(P(xbuf, xoff), ld, C, P(seg_d), nseg, P(yb, 5), P(ab, 2), st())
    else:
        ws = sentinel(L().efgh_segment_workspace(C, nseg) // 4 + 2, value=POISON)        # a partial that is read unwritten would win
        rc = L().efgh_segment_colmax_ws(P(xbuf, xoff), ld, C, P(seg_d), nseg, form, P(yb, 5), P(ab, 2), P(ws), st())
    sync_ok(rc)
    return yb, ab


# the one-stage kernel; the two-stage form with the slices sized from the rows (3 slices of a 300-row segment); the same with a hint
# that gives up to 78 slices, so that a 17-row segment has fewer rows than slices and most of its slices are empty
SEG_FORMS = {'one-stage': 'one', 'two-stage': None, 'two-stage-many-slices': 1 << 20}


@pytest.mark.parametrize('form', list(SEG_FORMS))
@pytest.mark.parametrize('C', SC.SEG_C)
def test_segment_colmax_and_its_backward(C, form):
    """value and row bit-equal to the contract in every form (so the forms are bit-equal to each other), with and without argrow;
    then the backward from this form's own argrow, the empty segments included"""
    x, seg = SC.gen_segmax(C, 40 + C)
    M, nseg, ld, xoff = x.shape[0], len(seg) - 1, C + 3, 6
    xbuf = place(x, ld, xoff, value=float('nan'))           # a read outside the rows or in the pad columns turns the result into NaN
    seg_d = torch.tensor(seg, dtype=torch.int32, device=DEV)
    y_ref, arg_ref = SC.segment_colmax(x, seg)
    assert bool((arg_ref[[0, 4, 12]] == -1).all()) and int((arg_ref < 0).sum()) == 3 * C
    how = SEG_FORMS[form] or M
    arg = None
    for want_arg in (True, False):
        lab = 'C %d %s arg %d' % (C, form, want_arg)
        yb, ab = _colmax(how, xbuf, xoff, ld, C, seg_d, nseg, M, want_arg)
        assert cmp('colmax', lab, yb[5:5 + nseg * C].view(nseg, C).cpu(), y_ref) == 0, lab
        assert outside_unchanged(yb, sentinel(yb.numel()), 5, C, nseg, C) == 0, lab
        if want_arg:
            arg = ab[2:2 + nseg * C].view(nseg, C)
            assert cmp('colmax', lab, arg.cpu(), arg_ref) == 0, lab
            assert bool((ab[:2] == -7777).all()) and bool((ab[2 + nseg * C:] == -7777).all()), lab
    # the backward from the forward's own argrow (equal to the contract's, asserted above: every row is -1 or inside [0, M))
    assert int(arg.max()) < M and int(arg.min()) >= -1
    dy = torch.randn(nseg, C)
    ld2, off2 = C + 2, 5
    buf, view = out_rows(M, C, ld2, off2)
    want = buf.clone()
    view2(want, off2, ld2, M, C).copy_(SC.segment_colmax_bwd(dy, arg_ref, view.cpu()))
    sync_ok(L().efgh_segment_colmax_bwd(P(dev(dy)), P(arg.contiguous()), nseg, C, P(buf, off2), ld2, st()))
    assert bits_equal(buf, want), 'C %d: dx differs from the prefilled buffer somewhere else than at the winners' % C
    assert int((buf != SENT).sum()) == int((arg_ref >= 0).sum())


# ------------------------------------------------------------------------------------------------ segment mean
@pytest.mark.parametrize('C,P_,nseg', SC.SEG_MEAN)
def test_segment_colmean_both_forms_and_its_backward(C, P_, nseg):
    g = torch.Generator().manual_seed(C + P_)
    x = torch.randn((nseg * P_, C), generator=g)
    ld, xoff = (4 if C == 3 else C + 1), 4
    xbuf = place(x, ld, xoff, value=float('nan'))
    ref, bound = SC.segment_colmean(x, P_, nseg)
    for form in ('one', 'two'):
        yb = sentinel(3 + nseg * C + 6)
        if form == 'one':
            rc = L().efgh_segment_colmean(P(xbuf, xoff), ld, C, P_, nseg, P(yb, 3), st())
        else:
            ws = sentinel(L().efgh_segment_workspace(C, nseg) // 8 + 2, torch.float64, POISON)
            rc = L().efgh_segment_colmean_ws(P(xbuf, xoff), ld, C, P_, nseg, P(yb, 3), P(ws), st())
        sync_ok(rc)
        lab = 'C %d P %d nseg %d %s-stage' % (C, P_, nseg, form)
        assert cmp('colmean', lab, yb[3:3 + nseg * C].view(nseg, C).cpu(), ref, bound) == 0, lab
        assert outside_unchanged(yb, sentinel(yb.numel()), 3, C, nseg, C) == 0, lab
    dy = torch.randn((nseg, C), generator=g)
    buf, view = out_rows(nseg * P_, C, ld, 2)
    sync_ok(L().efgh_segment_colmean_bwd(P(dev(dy)), P_, nseg, C, P(buf, 2), ld, st()))
    gref, gbound = SC.segment_colmean_bwd(dy, P_)
    assert cmp('colmean_bwd', 'C %d P %d nseg %d' % (C, P_, nseg), view.cpu(), gref, gbound) == 0
    assert outside_unchanged(buf, sentinel(buf.numel()), 2, ld, nseg * P_, C) == 0


# ------------------------------------------------------------------------------------------------ calls the header forbids
def test_forbidden_calls_return_an_error_and_write_nothing():
    """every buffer is large enough for the call taken at its word, so a check that went missing would show as a changed sentinel
    or a zero return code, not as a fault"""
    H, n, W = 8, 16, 520
    g = torch.Generator().manual_seed(3)
    a = SC.gen_splat([8] * H, 4, True, 1)
    feat = dev(SC.signed((n + 4, W + 8), g))
    emg, bary, lst, vseg, off = dev(a['emg']), dev(a['bary_pm']), dev(a['lst']), dev(a['vseg']), dev(a['off_pm'])
    out, wsum = sentinel((H + 4) * (W + 8)), sentinel(H + 8)

    def splat(emg_, ldf, Cf, lanes):
        return L().efgh_splat_gather(P(emg_), P(feat), ldf, Cf, P(bary), P(lst), P(vseg), H, 8, lanes, 1, P(out), P(wsum), st())
    bad = {
        'lanes 32 with CH 33': splat(emg, W + 8, 128, 32), 'lanes 16 with CH 17': splat(emg, W + 8, 64, 16),
        'lanes 8': splat(emg, W + 8, 4, 8), 'Cf 512': splat(None, W + 8, 512, 64), 'Cf % 4': splat(emg, W + 8, 6, 64),
        'ldf % 4': splat(emg, W + 6, 8, 64),
    }
    gs, gfeat = dev(SC.signed((H + 4, 16), g)), sentinel((n + 4) * 16)
    bad['coff + Cf > C'] = L().efgh_splat_bwd(P(gs), 8, 4, P(dev(torch.ones(H))), 8, P(bary), P(off), n, P(gfeat), 16, 1, st())
    nbr, alist = SC.gen_table(H, 2, 5)
    src, dst = dev(SC.signed((H + 1, 15 * W), g)), sentinel((H + 2) * W)
    n_alias = torch.tensor([2], dtype=torch.int32, device=DEV)
    bad['adjoint C 516'] = L().efgh_table_gather_transposed(P(src), P(dev(nbr)), H, 516, P(dev(alist)), P(n_alias), 2, P(dst), st())
    bad['alias_cap 0'] = L().efgh_table_gather_transposed(P(src), P(dev(nbr)), H, 8, P(dev(alist)), P(n_alias), 0, P(dst), st())
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad.values()), bad
    for name, buf in (('splat', out), ('wsum', wsum), ('gfeat', gfeat), ('dst', dst)):
        assert bool((buf == SENT).all()), name


# ------------------------------------------------------------------------------------------------ coverage
def test_every_entry_point_ran_and_the_observed_ratios():
    missing = [e for e in SC.ENTRY_POINTS if not CALLS.get(e)]
    assert not missing, missing
    print()
    for cls, (ratio, case) in sorted(SC.OBSERVED.items()):
        print('%-12s largest |got - ref| / (CEIL x S) = %.4f   %s' % (cls, ratio, case))
        assert ratio <= 1.0, cls
    assert {'splat', 'splat_wsum', 'splat_bwd', 'adjoint', 'scatter_add', 'colmean', 'colmean_bwd'} <= set(SC.OBSERVED)
