"""float64 reference of the gather-GEMM contract (test helper): efgh_gemm_desc, efgh_gather_gemm and the weight gradient with its
out descriptor (include/efgh_hip.h), written once from the header and independent of every kernel that serves a launch.

A launch is described by the arguments of ops.gather_gemm / ops.gather_wgrad (a dict, see bind), which mirror the
descriptor field by field.  Everything works on torch tensors of any device and computes in float64, row chunk by row chunk, so that
a full-size launch never holds more than a few hundred MB of float64 at once.

Error bound, element by element:  |got - ref| <= tau[family] * S + DELTA, where S is the same contraction on absolute values,
|A_in| @ |W|^T (weight gradient: |G|^T @ |A_in|), carried through the epilogue (|scale|, |bias|, |shift|, |residual|)."""
import inspect

import torch

MODE_BLUR_R = 4          # ops.MODE_BLUR_R: a radius-r blur through a [M][ld] table (efgh_blur_r_gemm / efgh_blur_r_wgrad)

# tau per family: at most 4x the largest |got - ref| / S observed over every launch of the runs of tests/test_gpu_launch_contract.py
# on an MI355X (the observed maximum in the comment; the kernels are deterministic, every run reproduced it to the last digit).
TAU = {
    'fp32': 1.6e-5,          # 4.16e-06 over 1873 launches, K <= 6720: exact fp32 (gather-GEMM, thin, 4-channel, small-channel, blur)
    'wino1d': 2.5e-4,        # 6.36e-05 over 268 launches, K <= 4608: Winograd F(4,3) along the rows (weight gradient: row_scale)
    'wino2d': 7.8e-5,        # 1.97e-05 over 312 launches, K <= 4608: Winograd F(4x4,3x3), exact fp32 plane GEMMs
    'wino2d_split': 1.1e-5,  # 2.98e-06 over 108 launches, K <= 4608: Winograd F(4x4,3x3), plane GEMMs on the three-way bf16 split
    # the column sums of an epilogue, relative to the sum of the magnitudes of their terms (the partials are fp32 sums over rows)
    'stats': 2.4e-5,         # 6.13e-06 over 690 launches: forward statistics, sum v and sum v^2 of the pre-activation value
    'bn_sums': 8.0e-8,       # 2.02e-08 over 46 launches: stats_mode 1, sum g and sum g * xhat
}
DELTA = 1e-30            # absolute floor: an exact zero must come out as (almost) zero
CHUNK_ELEMS = 1 << 23    # gathered operand elements per row chunk (x 8 bytes float64)


def family_of(calls):
    """the accuracy family of a launch from the C entry points it called"""
    calls = set(calls)
    if calls & {'efgh_plane_gemm_x6', 'efgh_plane_wgrad_x6_batched'}:
        return 'wino2d_split'
    if any(c.startswith('efgh_wino2d_') for c in calls):
        return 'wino2d'
    if calls & {'efgh_wino_conv3x3', 'efgh_wino_conv3x3_hpool', 'efgh_wino_wgrad'}:
        return 'wino1d'
    return 'fp32'


def bind(fn, args, kwargs):
    """the arguments of a call of `fn` (ops.gather_gemm / ops.gather_wgrad) as one dict, defaults filled in"""
    b = inspect.signature(fn).bind(*args, **kwargs)
    b.apply_defaults()
    return dict(b.arguments)


def flat(t):
    """1-D float32 / int32 view of t's storage from t's first element to the end of the storage (what a raw pointer can reach)"""
    n = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
    return torch.as_strided(t, (n,), (1,), t.storage_offset())


def take(f, idx):
    """f[idx] with the bounds checked on the host first (an out-of-range index on the device would abort the process)"""
    return f[_in_range(idx, f)]


def _in_range(idx, f):
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= f.numel()):
        raise IndexError(f'write set out of range: [{int(idx.min())}, {int(idx.max())}] of {f.numel()}')
    return idx


def _act(v, act, slope):
    if act == 1:
        return v.clamp_min(0)
    if act == 2:
        return torch.where(v > 0, v, v * slope)
    return v


# ------------------------------------------------------------------------------------------------ row addressing
def out_rows(L, ms):
    """output (pixel) row of GEMM rows ms: the placement (i*osh + oh0, j*osw + ow0) of a [B][Ho][Wo] image in mode 1, else m"""
    if L['mode'] != 1:
        return ms
    B, Hin, Win, Hv, Wv, sh, sw, dh, dw, Ho, Wo, osh, osw, oh0, ow0 = L['geom']
    j = ms % Wv
    r = ms // Wv
    i = r % Hv
    b = r // Hv
    return (b * Ho + (i * osh + oh0)) * Wo + (j * osw + ow0)


def src_rows(L, ms, z=0):
    """-> (offset [k][T] int64 of the first float of tap t of row m in flat(A), valid [k][T] bool: False = the tap reads zeros)"""
    mode, T, lda = L['mode'], L['T'], L['lda']
    dev = ms.device
    base = L.get('a_off', 0) + z * (L['batch'][1] if L.get('batch') else 0)
    if mode == 0:
        return (base + ms * lda)[:, None], torch.ones((ms.numel(), 1), dtype=torch.bool, device=dev)
    if mode == 1:
        B, Hin, Win, Hv, Wv, sh, sw, dh, dw = L['geom'][:9]
        j = ms % Wv
        r = ms // Wv
        i = r % Hv
        b = r // Hv
        dh = torch.as_tensor(list(dh), dtype=torch.int64, device=dev)
        dw = torch.as_tensor(list(dw), dtype=torch.int64, device=dev)
        ih = (i * sh)[:, None] + dh[None, :]
        iw = (j * sw)[:, None] + dw[None, :]
        ok = (ih >= 0) & (ih < Hin) & (iw >= 0) & (iw < Win)
        row = (b[:, None] * Hin + ih.clamp(0, Hin - 1)) * Win + iw.clamp(0, Win - 1)
        return base + row * lda, ok
    if mode == 3:
        B, Hin, Win, Hv, Wv = L['geom'][:5]
        b = ms // Wv
        j = ms % Wv
        t = torch.arange(T, dtype=torch.int64, device=dev)
        row = (b * Hin * Win + j)[:, None] + t[None, :] * Win
        return base + row * lda, torch.ones((ms.numel(), T), dtype=torch.bool, device=dev)
    tab = L['table']
    if mode == MODE_BLUR_R:
        r = take(tab, ms)[:, :T].to(torch.int64)
        ok = r >= 0
    else:                                   # mode 2: [M][16] table, problem z reads columns z*batch_stride_table ..
        bst = L['batch'][4] if (L.get('batch') and len(L['batch']) > 4) else 0
        tf = flat(tab)
        col = torch.arange(T, dtype=torch.int64, device=dev)
        r = take(tf, (ms * 16)[:, None] + z * bst + col[None, :]).to(torch.int64)
        ok = r >= 0
        if L.get('alias_mask'):
            bits = take(tf, ms * 16 + 15).to(torch.int64)
            ok = ok & (((bits[:, None] >> (z * bst + col[None, :])) & 1) == 0)
    return base + r.clamp_min(0) * lda, ok


def gather_a(L, ms, z=0, A=None):
    """-> (X [k][T*C] float64, Xabs [k][T*C]: the operand rows a launch multiplies, and the magnitudes its rounding scales with)"""
    A = L['A'] if A is None else A
    C = L['C']
    off, ok = src_rows(L, ms, z)
    Af = flat(A)
    c = torch.arange(C, dtype=torch.int64, device=off.device)
    idx = torch.where(ok[:, :, None], off[:, :, None] + c[None, None, :], torch.zeros((), dtype=torch.int64, device=off.device))
    X = take(Af, idx).double()
    X = torch.where(ok[:, :, None], X, torch.zeros((), dtype=X.dtype, device=X.device))
    lazy = L.get('lazy')
    if lazy is None:
        Xa = X.abs()
    else:                                  # A is the RAW BatchNorm output; the launch reads act(A*scale + shift), padding stays zero
        sc, sh = lazy.scale.double()[:C], lazy.shift.double()[:C]
        Y = X * sc + sh
        Xa = torch.where(ok[:, :, None], (X * sc).abs() + sh.abs(), torch.zeros((), dtype=X.dtype, device=X.device))
        X = torch.where(ok[:, :, None], _act(Y, lazy.act, lazy.slope), torch.zeros((), dtype=X.dtype, device=X.device))
    k = ms.numel()
    return X.reshape(k, -1), Xa.reshape(k, -1)


def weight_rows(L, z=0):
    """packed W [N][T*C] float64 of problem z"""
    K = L['T'] * L['C']
    Wf = flat(L['Wp'])
    bsw = L['batch'][2] if L.get('batch') else 0
    return Wf[z * bsw: z * bsw + L['N'] * K].double().view(L['N'], K)


def nbatch(L):
    b = L.get('batch')
    return b[0] if b else 1


def chunk_rows(L, K):
    return max(256, min(65536, CHUNK_ELEMS // max(K, 1)))


# ------------------------------------------------------------------------------------------------ forward
def forward_rows(L, ms, z=0, A=None, residual=None):
    """reference of GEMM rows ms of problem z -> dict(v: epilogue result [k][N], vs: the bound's scale of v, pre: acc + bias (what the
    statistics sum), pre_s: its scale, orow: output rows)"""
    X, Xa = gather_a(L, ms, z, A)
    W = weight_rows(L, z)
    acc = X @ W.t()
    S = Xa @ W.abs().t()
    N = L['N']
    dev = acc.device
    one = lambda v, d: (v.double()[:N] if v is not None else torch.full((N,), d, dtype=torch.float64, device=dev))
    bias, scale, shift = one(L.get('bias'), 0.0), one(L.get('scale'), 1.0), one(L.get('shift'), 0.0)
    pre = acc + bias
    pre_s = S + bias.abs()
    v = pre * scale + shift
    vs = pre_s * scale.abs() + shift.abs()
    orow = out_rows(L, ms)
    res = L.get('residual') if residual is None else residual
    if res is not None:
        rf = flat(res)
        n = torch.arange(N, dtype=torch.int64, device=dev)
        r = take(rf, (L['res_off'] + orow * L['ldr'])[:, None] + n[None, :]).double()
        v = v + r
        vs = vs + r.abs()
    v = _act(v, L.get('act', 0), L.get('slope', 0.0))
    return dict(v=v, vs=vs, pre=pre, pre_s=pre_s, orow=orow)


def out_index(L, orow, z=0):
    """flat(out) offsets [k][N] of output rows orow of problem z"""
    n = torch.arange(L['N'], dtype=torch.int64, device=orow.device)
    bso = L['batch'][3] if L.get('batch') else 0
    return (L['out_off'] + z * bso + orow * L['ldo'])[:, None] + n[None, :]


def m_launch(L):
    M = L['M']
    if L.get('M_dev') is not None:
        M = min(M, int(L['M_dev'].reshape(-1)[0]))
    return M


def check_forward(L, got_flat, before_flat, tau, A=None, residual=None):
    """compare one gather_gemm launch with the reference, every row.  got_flat / before_flat: flat(out) after / before the launch;
    A / residual: snapshots taken before the launch when they share storage with `out` (flat, from the operand's first element).
    -> dict(ratio: max |got - ref| / S, bad: elements over the bound, wild: elements outside the write set that changed,
            stats: (ratio, bad) of the statistics epilogue or None)"""
    M = m_launch(L)
    N = L['N']
    dev = got_flat.device
    written = torch.zeros(got_flat.numel(), dtype=torch.bool, device=dev)
    ratio, bad = 0.0, 0
    pool = L.get('pool')
    st_acc = None
    if L.get('stats') is not None:
        st_acc = [torch.zeros(N, dtype=torch.float64, device=dev) for _ in range(3)]   # sum v, sum v^2, sum |v|
    K = L['T'] * L['C']
    ch = chunk_rows(L, K)
    for z in range(nbatch(L)):
        if pool:
            B, Hin, Win, Hv, Wv = L['geom'][:5]
            Ho, Wo = L['geom'][9], L['geom'][10]
            Hp, Wp_ = (Ho // 2, Wo // 2) if pool is True else (Ho, Wo // 2)
            total = B * Hp * Wp_
            for q0 in range(0, total, max(1, ch // 4)):
                q = torch.arange(q0, min(total, q0 + max(1, ch // 4)), dtype=torch.int64, device=dev)
                qj, qr = q % Wp_, q // Wp_
                qi, qb = qr % Hp, qr // Hp
                win = [(0, 0), (0, 1), (1, 0), (1, 1)] if pool is True else [(0, 0), (0, 1)]
                vs, bs = [], []
                for di, dj in win:
                    ii = qi * 2 + di if pool is True else qi
                    ms = (qb * Hv + ii) * Wv + qj * 2 + dj
                    f = forward_rows(L, ms, z, A, residual)
                    vs.append(f['v'])
                    bs.append(f['vs'])
                ref = torch.stack(vs).amax(0)
                bnd = torch.stack(bs).amax(0)
                idx = out_index(L, q, z)
                ratio, bad = _cmp(got_flat, idx, ref, bnd, tau, ratio, bad)
                written[idx.reshape(-1)] = True
            continue
        for m0 in range(0, M, ch):
            m1 = min(M, m0 + ch)
            ms = torch.arange(m0, m1, dtype=torch.int64, device=dev)
            idx_all = out_index(L, out_rows(L, ms), z)
            written[_in_range(idx_all, written).reshape(-1)] = True
            f = forward_rows(L, ms, z, A, residual)
            idx = out_index(L, f['orow'], z)
            ratio, bad = _cmp(got_flat, idx, f['v'], f['vs'], tau, ratio, bad)
            if st_acc is not None:
                p = f['pre']
                st_acc[0] += p.sum(0)
                st_acc[1] += (p * p).sum(0)
                st_acc[2] += p.abs().sum(0)
    wild = int((got_flat.view(torch.int32)[~written] != before_flat.view(torch.int32)[~written]).sum())
    res = dict(ratio=ratio, bad=bad, wild=wild, stats=None)
    if st_acc is not None:
        part = L['stats'].double().reshape(-1, 2, N)
        g1, g2 = part[:, 0].sum(0), part[:, 1].sum(0)
        e1, e2 = (g1 - st_acc[0]).abs(), (g2 - st_acc[1]).abs()
        rel = torch.maximum(e1 / (st_acc[2] + DELTA), e2 / (st_acc[1] + DELTA))
        res['stats'] = (float(rel.max()) / TAU['stats'], int((rel > TAU['stats']).sum()))
    return res


def _cmp(got_flat, idx, ref, bnd, tau, ratio, bad):
    got = take(got_flat, idx).double()
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float('inf')))
    ratio = max(ratio, float((err / (bnd + DELTA / tau)).max()) if err.numel() else 0.0)
    bad += int((err > tau * bnd + DELTA).sum())
    return ratio, bad


def check_bn_bwd(L, out_flat, partials):
    """stats_mode 1: the [rows][2][N] partials a launch returned against sum g and sum g*(raw - mean)*invstd over the rows it wrote,
    g = out * act'(raw*pscale + pshift) (bn_y: act'(y)), taken of the launch's own output -> (ratio, bad)"""
    src = L['bn_bwd']
    M, N = m_launch(L), L['N']
    dev = out_flat.device
    s = torch.zeros((2, N), dtype=torch.float64, device=dev)
    bnd = torch.zeros((2, N), dtype=torch.float64, device=dev)
    ch = chunk_rows(L, N)
    rawf = flat(src.raw)
    ldraw = src.raw.stride(-2)
    n = torch.arange(N, dtype=torch.int64, device=dev)
    mean, invstd = src.mean.double()[:N], src.invstd.double()[:N]
    for m0 in range(0, M, ch):
        ms = torch.arange(m0, min(M, m0 + ch), dtype=torch.int64, device=dev)
        orow = out_rows(L, ms)
        g = take(out_flat, out_index(L, orow)).double()
        raw32 = take(rawf, orow[:, None] * ldraw + n[None, :])
        if src.y is not None:
            y = take(flat(src.y), orow[:, None] * src.y.stride(-2) + n[None, :])
            pre = y
        else:
            # the sign of raw*pscale + pshift with ONE rounding (fmaf in the kernel): exact product and sum in float64, same sign
            pre = raw32.double() * src.psc.double()[:N] + src.psh.double()[:N]
        d = torch.ones_like(g) if src.act == 0 else torch.where(pre > 0, torch.ones_like(g), torch.full_like(g, src.slope if src.act == 2 else 0.0))
        gd = g * d
        xhat = (raw32.double() - mean) * invstd
        s[0] += gd.sum(0)
        s[1] += (gd * xhat).sum(0)
        bnd[0] += gd.abs().sum(0)
        bnd[1] += (gd * xhat).abs().sum(0)
    got = partials.double().reshape(-1, 2, N).sum(0)
    rel = (got - s).abs() / (bnd + DELTA)
    return float(rel.max()) / TAU['bn_sums'], int((rel > TAU['bn_sums']).sum())


# ------------------------------------------------------------------------------------------------ weight gradient
def wgrad_ref(L):
    """dW [N][T][C] float64 = sum_m G[orow(m)][n] * A_in[row(m,t)][c], and its bound's scale |G|^T @ |A_in|"""
    M, N, T, C = L['M'], L['N'], L['T'], L['C']
    K = T * C
    dev = L['A'].device
    ref = torch.zeros((N, K), dtype=torch.float64, device=dev)
    S = torch.zeros((N, K), dtype=torch.float64, device=dev)
    Gf = flat(L['G'])
    n = torch.arange(N, dtype=torch.int64, device=dev)
    ch = chunk_rows(L, K + N)
    for m0 in range(0, M, ch):
        ms = torch.arange(m0, min(M, m0 + ch), dtype=torch.int64, device=dev)
        X, Xa = gather_a(L, ms)
        orow = out_rows(L, ms)
        G = take(Gf, orow[:, None] * L['ldg'] + n[None, :]).double()
        ref += G.t() @ X
        S += G.abs().t() @ Xa
    return ref.view(N, T, C), S.view(N, T, C)


def unpack_index(unpack, dev):
    """flat(dW) offsets [N][T][C] of the caller's layout W[n*sn + c*sc + taps[t]*st] (efgh_wgrad_out_desc)"""
    dW, N, T, C, Cp, sn, sc, st, taps, acc = unpack
    n = torch.arange(N, dtype=torch.int64, device=dev)
    c = torch.arange(C, dtype=torch.int64, device=dev)
    t = torch.as_tensor([int(x) for x in taps][:T], dtype=torch.int64, device=dev)
    return n[:, None, None] * sn + t[None, :, None] * st + c[None, None, :] * sc


def row_scale(S):
    """[N][9][C] -> the bound's scale of a 1-D Winograd weight gradient: its output transform (A3^T) forms the three kw taps of a
    kernel row from the same six products, so each inherits the rounding of the largest of them - an element whose own |G|^T |A| is
    tiny (its taps meet padding or zeros of a ReLU map) is not more exact than its row neighbours (measured: 3e-7 absolute next
    to S = 1.2e-5, 6e-7 of the launch's largest S)"""
    N, T, C = S.shape
    return S.view(N, 3, 3, C).amax(2, keepdim=True).expand(N, 3, 3, C).reshape(N, T, C)


def check_wgrad(L, done, tau, dW_before=None, rows=False):
    """compare one gather_wgrad call: done (its return value) -> the caller's layout through `unpack` (+= before when it accumulates),
    else the packed dWp [N][T][C].  rows: the bound's scale per kernel row (row_scale; 1-D Winograd).
    -> dict(ratio, bad, wild: elements of the caller's buffer outside the set that changed)"""
    ref, S = wgrad_ref(L)
    if rows:
        S = row_scale(S)
    dev = ref.device
    wild = 0
    if done:
        up = L['unpack']
        dW, N, T, C, acc = up[0], up[1], up[2], up[3], up[9]
        idx = unpack_index(up, dev)
        got = take(flat(dW), idx).double()
        r, s = ref[:N, :T, :C], S[:N, :T, :C]
        if acc:
            b = take(flat(dW_before), idx).double()
            r, s = r + b, s + b.abs()
        mask = torch.ones(flat(dW).numel(), dtype=torch.bool, device=dev)
        mask[idx.reshape(-1)] = False          # (in range: take() above)
        wild = int((flat(dW).view(torch.int32)[mask] != flat(dW_before).view(torch.int32)[mask]).sum())
    else:
        N, T, C = L['N'], L['T'], L['C']
        got = flat(L['dWp'])[:N * T * C].double().view(N, T, C)
        r, s = ref, S
    err = (got - r).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float('inf')))
    return dict(ratio=float((err / (s + DELTA / tau)).max()), bad=int((err > tau * s + DELTA).sum()), wild=wild)
