"""float64 reference of the point-cloud side of the E, H and G nets (test helper): the BCL splat and its backward, the adjoint of the
blur's neighbour gather (as a gather and as an atomic scatter) and the per-sample segment reductions with their backward passes -
the ten entry points of include/efgh_hip.h listed in ENTRY_POINTS, written from the header and the comments above each kernel,
independent of the kernel bodies.

Every function takes the fp32 / int32 tensors a kernel gets (any device), computes in float64 and returns the result with the scale
S of its error bound.  Error model, element by element, as in gemm_contract.py, with U = 2^-24:

    |got - ref| <= CEIL * S + DELTA

S is the reference's own expression on magnitudes.  The ceilings follow from the arithmetic; nothing here is measured:

  splat         ref[h][c] = (sum_{f in list(h)} bary[f] * row[f >> 2][c]) * nrm_h, nrm_h = 1 / (sum bary + 1e-5) or 1, row = [emg | feat].
                normalize: (2 L_h + 5) U - L_h products and adds in any order, the L_h adds of the density, the add of 1e-5, a division
                (<= 2.5 ulp) and the last multiply.  normalize == 0: (L_h + 1) U (the products and adds alone; the factor 1 is exact).
                wsum[h]: L_h U sum |bary|.  An empty list: a row of zeros and wsum 0.
  splat_bwd     ref[p][c] = sum_r bary[p][r] * nrm(wsum[off[p][r]]) * gsplat[off[p][r]][coff + c] with the fp32 wsum the kernel is given:
                9 U (add of 1e-5, division, two products, three adds)
  adjoint       ref[h][c] = sum_{(m, t < 15): nbr[m][t] == h} src[m][t C + c], alias-marked entries included: (14 + a_h) U sum |term|,
                a_h = alias records on h
  scatter_add   the same sum on top of dst, atomically in any order: count_h U (|dst0| + sum |term|)
  colmean       2 U sum |x| / P (a float64 sum, one cast);  colmean_bwd  2 U |dy| / P
  colmax        bit-exact in value and row; colmax_bwd a bit-exact copy that leaves every other element of dx unchanged

Semantics of the segment maximum, stated once:
  winner     the first strictly greatest row of the segment
  all -inf   a column of all -inf gives -inf and the segment's first row
  NaN        any NaN in the column gives NaN and the row of the first NaN (torch.max on the CPU)
  empty      an empty segment gives y = -inf and argrow = -1; the backward writes nothing for it"""
import numpy as np
import torch

from gemm_contract import DELTA, flat        # noqa: F401  (flat: re-exported for the test modules)

ENTRY_POINTS = [
    'efgh_splat_gather', 'efgh_splat_bwd', 'efgh_table_gather_transposed', 'efgh_table_scatter_add',
    'efgh_segment_colmax', 'efgh_segment_colmax_ws', 'efgh_segment_colmean', 'efgh_segment_colmean_ws',
    'efgh_segment_colmax_bwd', 'efgh_segment_colmean_bwd',
]
U = 2.0 ** -24
NORM_EPS = 1e-5
OBSERVED = {}            # class -> (largest |got - ref| / (CEIL * S), the case that produced it): filled by cmp()
MIN_TERM = 16.0          # input condition: every single term of a tested sum is at least this many times the element's bound
MAX_LIST = 300           # longest vertex list of the generated cases


# ------------------------------------------------------------------------------------------------ splat
def _entries(lst, vseg, H):
    """-> (vertex of every list entry, its flat position f), walking vseg's (start, length) windows of `lst`"""
    vs = vseg[:H].long()
    L = vs[:, 1]
    hid = torch.repeat_interleave(torch.arange(H, device=lst.device), L)
    first = torch.cumsum(L, 0) - L
    pos = vs[hid, 0] + torch.arange(int(L.sum()), device=lst.device) - first[hid]
    return hid, lst.long()[pos], L


def _row_amin(dst, rows, src):
    """dst[rows[i]] = min(dst[rows[i]], src[i]), in place"""
    idx = rows if src.dim() == 1 else rows[:, None].expand_as(src)
    return dst.scatter_reduce_(0, idx, src, 'amin', include_self=True)


def splat(emg, feat, Cf, bary_pm, lst, vseg, H, normalize):
    """efgh_splat_gather: emg [n][4] or None, feat [rows >= n][>= Cf], bary_pm [n][4], lst / vseg as the lattice build leaves them
    -> dict(ref [H][C], bound [H][C] = CEIL * S, wsum [H], wsum_bound [H], L [H], min_term [H][C] (inf for an empty list))"""
    hid, f, L = _entries(lst, vseg, H)
    p = f >> 2
    b = bary_pm.reshape(-1).double()[f]
    rows = feat[:, :Cf].double()[p]
    if emg is not None:
        rows = torch.cat([emg.double()[p], rows], 1)
    C = rows.shape[1]
    term = b[:, None] * rows
    ref = torch.zeros((H, C), dtype=torch.float64, device=feat.device).index_add_(0, hid, term)
    S = torch.zeros_like(ref).index_add_(0, hid, term.abs())
    w = torch.zeros(H, dtype=torch.float64, device=feat.device).index_add_(0, hid, b)
    wabs = torch.zeros_like(w).index_add_(0, hid, b.abs())
    mt = _row_amin(torch.full_like(ref, float('inf')), hid, term.abs())
    Ld = L.double()
    if normalize:
        nrm = 1.0 / (w + NORM_EPS)
        ref, S, mt = ref * nrm[:, None], S * nrm.abs()[:, None], mt * nrm.abs()[:, None]
        ceil = (2 * Ld + 5) * U
    else:
        ceil = (Ld + 1) * U
    return dict(ref=ref, bound=ceil[:, None] * S, wsum=w, wsum_bound=Ld * U * wabs, L=L, min_term=mt,
                min_bary=_row_amin(torch.full_like(w, float('inf')), hid, b.abs()))


def splat_bwd(gsplat, coff, wsum, Cf, bary_pm, off_pm, normalize):
    """efgh_splat_bwd: gsplat [H][C], wsum [H] fp32 as the forward left it -> (ref [n][Cf], bound = 9 U S)"""
    g = gsplat[:, coff:coff + Cf].double()
    o = off_pm.long()
    wgt = bary_pm.double()
    if normalize:
        wgt = wgt / (wsum.double()[o] + NORM_EPS)
    n = o.shape[0]
    ref = torch.zeros((n, Cf), dtype=torch.float64, device=gsplat.device)
    S = torch.zeros_like(ref)
    for r in range(4):
        t = wgt[:, r, None] * g[o[:, r]]
        ref += t
        S += t.abs()
    return ref, 9 * U * S


# ------------------------------------------------------------------------------------------------ neighbour table
def table_adjoint(src, nbr, C, dst0=None):
    """efgh_table_gather_transposed (dst0 None) / efgh_table_scatter_add (on top of dst0): src [H][15 C], nbr [H][16]
    -> dict(ref [H][C], bound [H][C], count [H] terms per row, alias [H] alias records per row, min_term [H][C])"""
    H = nbr.shape[0]
    dev = src.device
    ref = torch.zeros((H, C), dtype=torch.float64, device=dev)
    S = torch.zeros_like(ref)
    mt = torch.full_like(ref, float('inf'))
    count = torch.zeros(H, dtype=torch.float64, device=dev)
    alias = torch.zeros_like(count)
    s3 = src.double().view(H, 15, C)
    mask = nbr[:, 15].long()
    for t in range(15):
        tgt = nbr[:, t].long()
        m = torch.nonzero(tgt >= 0).reshape(-1)
        term = s3[m, t]
        ref.index_add_(0, tgt[m], term)
        S.index_add_(0, tgt[m], term.abs())
        _row_amin(mt, tgt[m], term.abs())
        one = torch.ones(m.numel(), dtype=torch.float64, device=dev)
        count.index_add_(0, tgt[m], one)
        alias.index_add_(0, tgt[m], one * ((mask[m] >> t) & 1).double())
    if dst0 is None:
        return dict(ref=ref, bound=((14 + alias) * U)[:, None] * S, count=count, alias=alias, min_term=mt)
    d0 = dst0.double()
    return dict(ref=ref + d0, bound=(count * U)[:, None] * (d0.abs() + S), count=count, alias=alias, min_term=mt)


# ------------------------------------------------------------------------------------------------ segment reductions
def segment_colmax(x, seg):
    """x [M][C] fp32 (a view), seg: nseg + 1 row bounds -> (y [nseg][C] fp32: the winning element itself, argrow [nseg][C] int32)"""
    seg = [int(v) for v in seg]
    nseg, C = len(seg) - 1, x.shape[1]
    y = torch.full((nseg, C), float('-inf'), dtype=torch.float32, device=x.device)
    arg = torch.full((nseg, C), -1, dtype=torch.int64, device=x.device)
    for s in range(nseg):
        a, b = seg[s], seg[s + 1]
        if b <= a:
            continue                                                    # empty: -inf and -1
        xs = x[a:b]
        nan = torch.isnan(xs)
        m = torch.where(nan, torch.full_like(xs, float('-inf')), xs).amax(0)
        first_max = (xs == m[None]).to(torch.uint8).argmax(0)           # the first row that attains the maximum (row 0 when all are -inf)
        first_nan = nan.to(torch.uint8).argmax(0)
        row = torch.where(nan.any(0), first_nan, first_max)
        arg[s] = row + a
        y[s] = xs.gather(0, row[None])[0]
    return y, arg.to(torch.int32)


def segment_colmean(x, P, nseg):
    """x [nseg * P][C] -> (ref [nseg][C], bound)"""
    v = x.double().view(nseg, P, -1)
    return v.sum(1) / P, 2 * U * v.abs().sum(1) / P


def segment_colmax_bwd(dy, arg, dx0):
    """dx0 [M][C] as the caller prefilled it -> dx (fp32, exact): dy at the winners, everything else as it was"""
    dx = dx0.clone()
    ok = arg >= 0
    cols = torch.arange(arg.shape[1], device=arg.device)[None].expand_as(arg)
    dx[arg.long()[ok], cols[ok]] = dy[ok]
    return dx


def segment_colmean_bwd(dy, P):
    """-> (ref [nseg * P][C], bound)"""
    ref = (dy.double() / P).repeat_interleave(P, 0)
    return ref, 2 * U * ref.abs()


# ------------------------------------------------------------------------------------------------ comparison
def cmp(cls, label, got, ref, bound=None):
    """-> number of elements with |got - ref| > bound + DELTA (bound = CEIL * S, element by element); records the largest
    |got - ref| / bound of the class in OBSERVED.  bound None: bit-exact (ref fp32 / int32; two NaNs in one place are equal)"""
    if bound is None:
        a, b = got.contiguous(), ref.to(got.dtype).contiguous()
        if a.dtype == torch.float32:
            both_nan = torch.isnan(a) & torch.isnan(b)
            return int(((a.view(torch.int32) != b.view(torch.int32)) & ~both_nan).sum())
        return int((a != b).sum())
    g = got.double()
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float('inf')))
    ratio = float(((err - DELTA).clamp_min(0) / (bound + 1e-300)).max()) if err.numel() else 0.0
    if ratio > OBSERVED.get(cls, (-1.0, ''))[0]:
        OBSERVED[cls] = (ratio, label)
    return int((err > bound + DELTA).sum())


def condition_margin(min_term, bound):
    """the input condition: smallest (single term of a sum) / (the element's bound) over the elements that have terms"""
    has = torch.isfinite(min_term)
    if not bool(has.any()):
        return float('inf')
    return float((min_term[has] / (bound[has] + 1e-300)).min())


# ------------------------------------------------------------------------------------------------ inputs
def signed(shape, g):
    """|x| in [1, 2] with a random sign"""
    return (1.0 + torch.rand(shape, generator=g)) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


# list lengths dealt to consecutive vertices: an empty list next to the longest, both sides of 16 / 32 / 64 entries (one trip of each
# lane mapping), several trips (129, 300); neighbours in a wave always differ
PROFILE = [300, 0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129]


def list_lengths(H, shift=0):
    """H list lengths from PROFILE (rotated by `shift`), the sum made a multiple of 4 (a point has four entries) by lengthening
    the first list of 129 or, without one, the longest list below MAX_LIST - 3; H == 1: one list of a multiple of 4"""
    L = [PROFILE[(h + shift) % len(PROFILE)] for h in range(H)]
    if H == 1:
        return [max(4, L[0] // 4 * 4)]
    pad = -sum(L) % 4
    if pad:
        k = L.index(129) if 129 in L else max((h for h in range(H) if L[h] <= MAX_LIST - 3), key=lambda h: L[h])
        L[k] += pad
    if sum(L) == 0:
        L[0] = 4
    return L


def gen_splat(lengths, Cf, emg, seed, extra_rows=3):
    """splat arrays without a lattice build: off_pm [n][4] deals the 4 n flat positions to the vertices at random, lengths[h] of them
    to vertex h; list / vseg are its stable inverse (ascending f = 4 p + r per vertex) with gaps between the windows, as a real build
    leaves them (the gaps hold valid positions of OTHER vertices: an entry read from a gap gives a wrong sum, not a fault);
    bary in [0.25, 1], |feat|, |emg| in [1, 2] -> dict of CPU tensors (feat has `extra_rows` more rows than points)"""
    g = torch.Generator().manual_seed(seed)
    H = len(lengths)
    L = torch.tensor(lengths, dtype=torch.int64)
    total = int(L.sum())
    assert total % 4 == 0 and total > 0 and max(lengths) <= MAX_LIST
    n = total // 4
    off = torch.empty(total, dtype=torch.int64)
    off[torch.randperm(total, generator=g)] = torch.repeat_interleave(torch.arange(H), L)
    gaps = torch.randint(0, 8, (H,), generator=g)
    gaps[0] += 5
    start = torch.cumsum(L + gaps, 0) - L
    lst = torch.randint(0, total, (int(start[-1] + L[-1]) + 9,), generator=g)
    order = torch.sort(off, stable=True).indices                       # ascending f within a vertex
    first = torch.cumsum(L, 0) - L
    hid = off[order]
    lst[start[hid] + torch.arange(total) - first[hid]] = order
    return dict(H=H, n=n, Cf=Cf, lengths=lengths, off_pm=off.view(n, 4).to(torch.int32), bary_pm=0.25 + 0.75 * torch.rand((n, 4), generator=g),
                lst=lst.to(torch.int32), vseg=torch.stack([start, L], 1).to(torch.int32), feat=signed((n + extra_rows, Cf), g),
                emg=signed((n, 4), g) if emg else None)


def gen_table(H, n_alias, seed, fill=0.6, alias_rows=None):
    """neighbour table without a lattice build: nbr [H][16], nbr[h][0] = h, one random partial injection per t in 1..7 mirrored into
    15 - t (so the unmarked part is symmetric under t <-> 15 - t), -1 elsewhere; `n_alias` absent entries (m, t >= 1) pointed at
    arbitrary vertices (the first three at one target) and marked as the build marks a real aliased hit: bit t of column 15 and a
    record (m * 16 + t, target) in alist, in shuffled order -> (nbr int32 [H][16], alist int32 [max(n_alias, 1) or alias_rows][2])"""
    rs = np.random.RandomState(seed)
    nbr = np.full((H, 16), -1, np.int32)
    nbr[:, 0] = np.arange(H)
    nbr[:, 15] = 0
    for t in range(1, 8):
        a = np.nonzero(rs.rand(H) < fill)[0]
        b = rs.permutation(H)[:len(a)]
        nbr[a, t] = b
        nbr[b, 15 - t] = a
    hh, tt = np.nonzero(nbr[:, 1:15] < 0)
    assert len(hh) >= n_alias, 'not enough absent entries for the alias records'
    pick = rs.choice(len(hh), size=n_alias, replace=False) if n_alias else []
    recs = []
    for i, k in enumerate(pick):
        m, t = int(hh[k]), int(tt[k]) + 1
        target = int(rs.randint(0, H)) if i >= 3 else H // 2
        nbr[m, t] = target
        nbr[m, 15] |= 1 << t
        recs.append((m * 16 + t, target))
    rs.shuffle(recs)
    alist = np.zeros((alias_rows or max(n_alias, 1), 2), np.int32)
    if recs:
        alist[:len(recs)] = np.asarray(recs, np.int32).reshape(-1, 2)
    return torch.from_numpy(nbr), torch.from_numpy(alist)


# ------------------------------------------------------------------------------------------------ the cases of the GPU module
SPLAT_LANES = (16, 32, 64)
# 16-byte chunks per row, CH = (emg ? 1 : 0) + Cf / 4: 1, 2, 3, 5 do not divide the lanes; 16 | 17, 32 | 33 the limits of the 16- and the
# 32-lane mapping; 63, 64 one chunk per lane; 65 the second chunk with one lane; 127, 128 the widest rows (Cf = 508)
SPLAT_CH = (1, 2, 3, 5, 9, 16, 17, 32, 33, 63, 64, 65, 127, 128)
SPLAT_CH_ALL_H = (1, 3, 16, 32, 65, 128)       # these run at every H of splat_H, the others at the two largest


def splat_H(lanes):
    """vertex counts of a mapping, VPB = 256 / lanes vertices per block: block counts 1, 2, 9, 10 and 18 (the band mapping of the
    blocks rounds the grid up to a multiple of 8) and a last block with one, all and some vertices"""
    v = 256 // lanes
    return [1, v - 1, v, v + 1, 8 * v + 1, 9 * v, 17 * v + 3]


def splat_variants(CH):
    """(emg, Cf) that give CH chunks: without emg Cf = 4 CH <= 508, with emg Cf = 4 (CH - 1) > 0"""
    return [(e, 4 * (CH - e)) for e in (0, 1) if 0 < 4 * (CH - e) <= 508]


def splat_cases():
    """(lanes, CH, emg, Cf, H) of every forward case"""
    out = []
    for lanes in SPLAT_LANES:
        for CH in SPLAT_CH:
            if (lanes == 16 and CH > 16) or (lanes == 32 and CH > 32):
                continue
            Hs = splat_H(lanes) if CH in SPLAT_CH_ALL_H else splat_H(lanes)[-2:]
            out += [(lanes, CH, e, Cf, H) for e, Cf in splat_variants(CH) for H in Hs]
    return out


def splat_seed(CH, emg, H):
    return 1000 * CH + 7 * H + emg


def gen_splat_case(CH, emg, Cf, H, normalize_for_condition=(0, 1)):
    """the arrays of one forward case, regenerated with the next seed until the input condition holds for both values of normalize
    -> (arrays, smallest margin, {normalize: the reference of splat()})"""
    seed = splat_seed(CH, emg, H)
    for attempt in range(16):
        a = gen_splat(list_lengths(H, shift=H + CH), Cf, bool(emg), seed + 100003 * attempt)
        margin, refs = float('inf'), {}
        for nz in normalize_for_condition:
            r = refs[nz] = splat(a['emg'], a['feat'], Cf, a['bary_pm'], a['lst'], a['vseg'], H, nz)
            margin = min(margin, condition_margin(r['min_term'], r['bound']), condition_margin(r['min_bary'], r['wsum_bound']))
        if margin >= MIN_TERM:
            return a, margin, refs
    raise AssertionError('no inputs that meet the input condition: CH %d emg %d H %d' % (CH, emg, H))


SPLAT_BWD_CASES = [(1, 4), (3, 340), (65, 36), (257, 128)]        # (n, Cf): one thread, 255 of a block, 585 and 8224 threads


def gen_splat_bwd_case(n, Cf):
    """n points on max(2, n / 2) vertices, the 4 n entries dealt at random"""
    H = max(2, n // 2)
    lengths = np.random.RandomState(n).multinomial(4 * n, [1.0 / H] * H).tolist()
    return gen_splat(lengths, Cf, False, 7 * n + Cf, extra_rows=0)
ADJ_C = (4, 64, 68, 128, 132, 256, 260, 512)        # 16 | 32 | 64 lanes per row, and the second chunk above 256
# H -> [(n_alias, alias_cap, fill)]: none, one, 40 with several on one target, exactly alias_cap
ADJ_H = {1: [(0, 4, 0.6), (1, 4, 0.3)], 3: [(0, 1, 0.6), (6, 6, 0.5)], 4: [(1, 16, 0.6), (16, 16, 0.4)], 5: [(0, 4096, 0.6), (40, 64, 0.15)],
         33: [(1, 4096, 0.6), (40, 4096, 0.6), (64, 64, 0.6)]}


def adj_cases():
    return [(C, H, na, cap, fill) for C in ADJ_C for H, plans in ADJ_H.items() for na, cap, fill in plans]


def gen_adj_case(C, H, na, cap, fill):
    """-> (nbr, alist [cap][2], src [H][15 C], dst0 [H][C]) of one adjoint case (CPU)"""
    nbr, alist = gen_table(H, na, seed=131 * H + na, fill=fill, alias_rows=cap)
    g = torch.Generator().manual_seed(17 * C + H + na)
    return nbr, alist, signed((H, 15 * C), g), signed((H, C), g)


SEG_C = (1, 3, 31, 32, 33, 128, 257)
# segments of the maximum: empty first / middle / last, one row, fewer rows than slices, 17, 2049, and the carriers of the planted values
SEG_LENS = [0, 1, 3, 17, 0, 2049, 17, 17, 300, 300, 300, 1, 0]
SEG_MEAN = [(3, 7, 2), (4, 513, 1), (33, 64, 3), (64, 1000, 8)]      # (C, P, nseg)


def gen_segmax(C, seed):
    """x [M][C] (CPU, fp32) over SEG_LENS with the planted edge values, seg bounds.  Planted (column 0 and column C - 1):
      segment 3   column 0 all -inf; column C - 1 -inf but for one row
      segment 5   the maximum 9 at rows +5 and +6 (neighbouring row lanes) and +261 (the row lane of +5 again, whatever power of two up to
                  256 the lanes count, and the same slice of three) in column 0, at rows +100 and +1900 (two slices) in column C - 1
      segment 6   NaN in the first row (column 0) and in the last row (column C - 1)
      segment 7   NaNs at rows +3, +9, +12 of column 0
      segment 8   the maximum at +10 and a NaN at +250 (another slice) in column 0; the NaN at +10 and the maximum at +250 in column C - 1
      segment 9   NaNs at +250 and +20 in column 0
      segment 10  column 0 all -inf but a NaN at +299
      segment 11  its single element NaN (column C - 1)"""
    g = torch.Generator().manual_seed(seed)
    seg = [0] + [int(v) for v in np.cumsum(SEG_LENS)]
    x = torch.randn((seg[-1], C), generator=g)
    nan, ninf, last = float('nan'), float('-inf'), C - 1
    a = seg[3]
    x[a:seg[4], 0] = ninf
    if C > 1:
        x[a:seg[4], last] = ninf
        x[a + 11, last] = -3.0
    a = seg[5]
    x[a + 100, last] = 9.0
    x[a + 1900, last] = 9.0
    x[a + 5, 0] = 9.0
    x[a + 6, 0] = 9.0
    x[a + 261, 0] = 9.0
    a = seg[6]
    x[seg[7] - 1, last] = nan
    x[a, 0] = nan
    a = seg[7]
    x[a + 3, 0] = x[a + 9, 0] = x[a + 12, 0] = nan
    a = seg[8]
    x[a + 10, last], x[a + 250, last] = nan, 50.0
    x[a + 10, 0], x[a + 250, 0] = 50.0, nan
    a = seg[9]
    x[a + 250, 0] = x[a + 20, 0] = nan
    a = seg[10]
    x[a:seg[11], 0] = ninf
    x[a + 299, 0] = nan
    x[seg[11], last] = nan
    return x, seg
