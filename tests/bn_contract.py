"""float64 reference of the HBM-bound passes around the GEMMs (test helper): BatchNorm statistics / finalize / apply, the activation,
MaxPool2d(2,2) and their backward passes - the 15 entry points of include/efgh_hip.h listed in ENTRY_POINTS, written once from the
header and the comments above each kernel, independent of the kernel bodies.

Every function takes the fp32 tensors a kernel gets ([M][C] or [B][H][W][C] views, any strides, any device), computes in float64
and returns the result with the scale S of its error bound.  Error model, element by element, as in gemm_contract.py:

    |got - ref| <= TAU_BN[class] * S + DELTA

S is the same expression on magnitudes: |x||scale| + |shift| + |res| (times max(1, |slope|)) for an output of the apply kernels,
|coef| (|dpre| + |m1| + |xhat||m2|) for draw, the sum of |term| for a column sum, (sum |term|) / count for m1 / m2.  Copies (pooling
maxima, pooled gradients routed to the winner, dres where the derivative is 1 or 0) are bit-exact.

Semantics, stated once:
  activation   ReLU v > 0 ? v : 0;  leaky v > 0 ? v : v*slope;  derivative 1 / 0 / slope on the same strict > 0
  pool winner  the first strictly greatest element in (h, w) scan order (first_max: explicit strict comparisons)
  floor pool   odd trailing rows / columns get no pooled gradient; efgh_pool_bn_bwd_apply still gives them coef*(-m1 - xhat*m2)
  mask source  efgh_act_bn_bwd_reduce / _apply: y (y > 0), the sign bits (ldy == 0), or raw*pscale + pshift > 0
  forms        mean == NULL: xhat := 0 - only the first sum counts, draw = coef*dpre (dpre without coef); dres optional, draw optional
               when dres is given
  pooled-from-y  d = dy_pool where y_pool > 0, xhat = (y_pool - beta)/gamma with beta = mean*pscale + pshift, gamma = pscale/invstd;
               from raw at the window's first element where gamma == 0, and from raw at the window's winner where
               |beta| > POOLED_BETA_GAMMA * |gamma| (there the rounding of y_pool would cost |beta|/|gamma| roundings of xhat)"""
import numpy as np
import torch

from gemm_contract import DELTA, flat

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
ENTRY_POINTS = [
    'efgh_col_stats', 'efgh_bn_finalize', 'efgh_scale_shift_act', 'efgh_scale_shift_act_bits',
    'efgh_maxpool2', 'efgh_maxpool_v2', 'efgh_maxpool2_affine', 'efgh_maxpool2_bwd', 'efgh_maxpool2_bwd_affine',
    'efgh_act_bn_bwd_reduce', 'efgh_act_bn_bwd_apply', 'efgh_bwd_finalize_f32',
    'efgh_pool_bn_bwd_reduce', 'efgh_pool_bn_bwd_reduce_pooled', 'efgh_pool_bn_bwd_apply',
]
# entry points with a non-temporal instance, and the bytes their switch looks at (common.h: efgh_stream_nt, bytes >= 384 << 20)
NT_BYTES = 384 << 20
NT_ENTRY_POINTS = ['efgh_scale_shift_act', 'efgh_scale_shift_act_bits', 'efgh_maxpool2_affine', 'efgh_act_bn_bwd_reduce',
                   'efgh_act_bn_bwd_apply', 'efgh_pool_bn_bwd_reduce', 'efgh_pool_bn_bwd_reduce_pooled', 'efgh_pool_bn_bwd_apply']

U = 2.0 ** -24
# ceilings that follow from the arithmetic (they hold whatever is measured)
CEIL = {
    'elem': 8 * U,        # at most three fp32 roundings of values of size S; contraction may remove some
    'f64sum': 4 * U,      # fp32 outputs of the float64-accumulated sums: two roundings in xhat, one in the product's operand, the cast
    'm': 3 * U,           # m1 / m2 (float64): their terms are fp32 products
    'colstats': 512 * U,  # efgh_col_stats: fp32 accumulation, 512 rows per partial
    # efgh_bn_finalize computes in float64 from the fp32 partials and rounds its outputs: invstd (1), scale = gamma*invstd (2),
    # shift = beta - (float)mean*scale (3); above 256 partial rows the first stage leaves fp32 sums (1 more, carried through S)
    'finalize': 4 * U,
}
# tau per class: at most 4x the largest |got - ref| / S observed on an MI355X over every case of tests/test_gpu_bn_contract.py (the
# observed maximum and its case in the comment; the kernels are deterministic), never above the ceiling of the class
TAU_BN = {
    'elem': 4.7e-7,       # 1.188e-07 (1.99 x 2^-24): efgh_scale_shift_act with a residual, 2083 x 260, leaky slope 0
    'f64sum': CEIL['f64sum'],   # 1.193e-07 (2.00 x 2^-24): sum dpre*xhat of efgh_pool_bn_bwd_reduce, 1x2x2x4, ReLU; 4x is above the ceiling
    'm': CEIL['m'],       # 1.102e-07 (1.85 x 2^-24): m2 of efgh_pool_bn_bwd_reduce_pooled, 1x3x2x64; 4x is above the ceiling
    'colstats': 2.9e-6,   # 7.332e-07 (12.3 x 2^-24): efgh_col_stats, 16 400 x 4 (one channel lane: 256 row lanes, then the fp32 tree)
    'finalize': CEIL['finalize'],   # 1.262e-07 (2.12 x 2^-24): running mean of efgh_bn_finalize, 70 000 x 256 (137 partial rows); 4x is above the ceiling
}
OBSERVED = {}            # class -> (largest |got - ref| / S, the case that produced it): filled by cmp(), printed by the last GPU test
CHUNK = 1 << 22          # elements per row chunk of the large cases (x 8 bytes float64 per temporary)


# ------------------------------------------------------------------------------------------------ semantics
def act(v, a, slope):
    z = torch.zeros((), dtype=v.dtype, device=v.device)
    if a == ACT_RELU:
        return torch.where((v > 0) | torch.isnan(v), v, z)          # (a NaN stays a NaN under every activation)
    if a == ACT_LEAKY:
        return torch.where(v > 0, v, v * slope)
    return v


def dact(pos, a, slope):
    """derivative of the activation where pos = (pre-activation > 0)"""
    one = torch.ones((), dtype=torch.float64, device=pos.device)
    if a == ACT_RELU:
        return torch.where(pos, one, one * 0)
    if a == ACT_LEAKY:
        return torch.where(pos, one, one * float(slope))
    return one.expand(pos.shape)


def f32(v):
    """a Python float as the kernel receives it (a float argument)"""
    return float(np.float32(v))


def first_max(e4):
    """e4 [4][...]: the window in scan order (0,0) (0,1) (1,0) (1,1) -> (index of the first strictly greatest element, its value)"""
    best = torch.zeros(e4.shape[1:], dtype=torch.int64, device=e4.device)
    cur = e4[0]
    for q in (1, 2, 3):
        gt = e4[q] > cur
        best = torch.where(gt, torch.full_like(best, q), best)
        cur = torch.where(gt, e4[q], cur)
    return best, cur


def windows(x):
    """[B][H][W][C] -> [4][B][H/2][W/2][C]: the four elements of every floor window, scan order"""
    Ho, Wo = x.shape[1] // 2, x.shape[2] // 2
    xx = x[:, :2 * Ho, :2 * Wo]
    return torch.stack([xx[:, 0::2, 0::2], xx[:, 0::2, 1::2], xx[:, 1::2, 0::2], xx[:, 1::2, 1::2]])


def unwindows(w4, H, W):
    """[4][B][Ho][Wo][C] -> [B][H][W][C], zero on the odd rim"""
    _, B, Ho, Wo, C = w4.shape
    x = torch.zeros((B, H, W, C), dtype=w4.dtype, device=w4.device)
    x[:, 0:2 * Ho:2, 0:2 * Wo:2] = w4[0]
    x[:, 0:2 * Ho:2, 1:2 * Wo:2] = w4[1]
    x[:, 1:2 * Ho:2, 0:2 * Wo:2] = w4[2]
    x[:, 1:2 * Ho:2, 1:2 * Wo:2] = w4[3]
    return x


def one_hot_window(best):
    q = torch.arange(4, device=best.device).view(4, *([1] * best.dim()))
    return best.unsqueeze(0) == q


def pack_bits(pos):
    """[M][C] bool -> int32 words: bit e % 32 of word e / 32 = pos of element e = r*C + c"""
    w = (pos.reshape(-1, 32).to(torch.int64) << torch.arange(32, dtype=torch.int64, device=pos.device)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_bits(bits, M, C):
    w = bits.to(torch.int64).reshape(-1, 1)
    return ((w >> torch.arange(32, dtype=torch.int64, device=bits.device)) & 1).reshape(-1)[:M * C].reshape(M, C) != 0


def row_chunks(M, C):
    step = max(1, CHUNK // max(C, 1))
    return [(r, min(M, r + step)) for r in range(0, M, step)]


# ------------------------------------------------------------------------------------------------ forward
def col_stats_groups(M):
    return (M + 511) // 512


def col_stats(x):
    """efgh_col_stats: x [M][C] -> (sums [G][2][C] of x and x^2 over rows 512 g .. 512 g + 511, the same of |x| and x^2)"""
    M, C = x.shape
    G = col_stats_groups(M)
    ref = torch.zeros((G, 2, C), dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(ref)
    step = max(512, CHUNK // C // 512 * 512)
    for r0 in range(0, M, step):
        v = x[r0:r0 + step].double()
        k = v.shape[0]
        if k % 512:
            v = torch.cat([v, torch.zeros((512 - k % 512, C), dtype=v.dtype, device=v.device)])
        v = v.view(-1, 512, C)
        g0 = r0 // 512
        ref[g0:g0 + v.shape[0], 0] = v.sum(1)
        ref[g0:g0 + v.shape[0], 1] = (v * v).sum(1)
        mag[g0:g0 + v.shape[0], 0] = v.abs().sum(1)
    mag[:, 1] = ref[:, 1]
    return ref, mag


def bn_finalize(stats, count, gamma, beta, rmean, rvar, momentum, eps):
    """efgh_bn_finalize: stats [G][2][C] -> {name: (value, S)} for scale, shift, mean, invstd and (rmean given) rmean, rvar"""
    st = stats.double()
    s, q = st[:, 0].sum(0), st[:, 1].sum(0)
    sa, qa = st[:, 0].abs().sum(0), st[:, 1].abs().sum(0)
    g, b = gamma.double(), beta.double()
    mom, eps = f32(momentum), f32(eps)
    mean, S_mean = s / count, sa / count
    var = (q / count - mean * mean).clamp_min(0)
    S_var = qa / count + 2 * mean.abs() * S_mean
    invstd = 1.0 / torch.sqrt(var + eps)
    S_inv = invstd + 0.5 * invstd ** 3 * S_var
    scale, S_scale = g * invstd, g.abs() * S_inv
    shift, S_shift = b - mean * scale, b.abs() + mean.abs() * S_scale + S_mean * scale.abs()
    out = dict(scale=(scale, S_scale), shift=(shift, S_shift), mean=(mean, S_mean), invstd=(invstd, S_inv))
    if rmean is not None:
        k = count / (count - 1) if count > 1 else 1.0
        out['rmean'] = ((1 - mom) * rmean.double() + mom * mean, (1 - mom) * rmean.double().abs() + mom * S_mean)
        out['rvar'] = ((1 - mom) * rvar.double() + mom * var * k, (1 - mom) * rvar.double().abs() + mom * S_var * k)
    return out


def scale_shift_act(x, scale, shift, res, a, slope):
    """efgh_scale_shift_act(_bits): -> (y, S, pre); the mask bit of an element is y > 0 (a NaN stays NaN, its bit is 0)"""
    pre = x.double()
    S = pre.abs()
    if scale is not None:
        pre, S = pre * scale.double(), S * scale.double().abs()
    if shift is not None:
        pre, S = pre + shift.double(), S + shift.double().abs()
    if res is not None:
        pre, S = pre + res.double(), S + res.double().abs()
    slope = f32(slope)
    if a == ACT_LEAKY:
        S = S * max(1.0, abs(slope))
    return act(pre, a, slope), S, pre


def maxpool2(x):
    return first_max(windows(x.double()))[1]


def maxpool_v2(x):
    Ho = x.shape[1] // 2
    a, c = x[:, 0:2 * Ho:2].double(), x[:, 1:2 * Ho:2].double()
    return torch.where(c > a, c, a)


def _affine_windows(x, scale, shift, a, slope):
    w = windows(x.double())
    pre = w * scale.double() + shift.double()
    S = w.abs() * scale.double().abs() + shift.double().abs()
    if a == ACT_LEAKY:
        S = S * max(1.0, abs(f32(slope)))
    return w, pre, act(pre, a, f32(slope)), S


def maxpool2_affine(x, scale, shift, a, slope):
    """-> (max over the window of act(x*scale + shift), S: the largest of the window's four)"""
    _, _, e, S = _affine_windows(x, scale, shift, a, slope)
    return first_max(e)[1], S.amax(0)


def maxpool2_bwd(x, dy):
    """-> dx on the pooled region [B][2 (H/2)][2 (W/2)][C] (the odd rim is not written): dy at the window's winner, 0 elsewhere"""
    best, _ = first_max(windows(x.double()))
    z = torch.zeros((), dtype=torch.float64, device=x.device)
    return unwindows(torch.where(one_hot_window(best), dy.double().unsqueeze(0), z), 2 * (x.shape[1] // 2), 2 * (x.shape[2] // 2))


def maxpool2_bwd_affine(x, scale, shift, a, slope, dy):
    _, _, e, _ = _affine_windows(x, scale, shift, a, slope)
    best, _ = first_max(e)
    z = torch.zeros((), dtype=torch.float64, device=x.device)
    return unwindows(torch.where(one_hot_window(best), dy.double().unsqueeze(0), z), 2 * (x.shape[1] // 2), 2 * (x.shape[2] // 2))


# ------------------------------------------------------------------------------------------------ backward
def mask_of(y=None, bits=None, raw=None, pscale=None, pshift=None):
    """where the activation's pre-activation counts as > 0, from one of the three sources"""
    if bits is not None:
        return bits
    if y is not None:
        return y > 0
    return raw.double() * pscale.double() + pshift.double() > 0


def act_bn_bwd_reduce(dy, pos, raw, mean, invstd, a, slope):
    """-> (sums [2][C]: sum dpre, sum dpre*xhat; bound [2][C]: the sums of |term|).  mean None: xhat := 0"""
    M, C = dy.shape
    s = torch.zeros((2, C), dtype=torch.float64, device=dy.device)
    bnd = torch.zeros_like(s)
    for r0, r1 in row_chunks(M, C):
        dpre = dy[r0:r1].double() * dact(pos[r0:r1], a, f32(slope))
        s[0] += dpre.sum(0)
        bnd[0] += dpre.abs().sum(0)
        if mean is not None:
            t = dpre * ((raw[r0:r1].double() - mean.double()) * invstd.double())
            s[1] += t.sum(0)
            bnd[1] += t.abs().sum(0)
    return s, bnd


def act_bn_bwd_apply(dy, pos, raw, mean, invstd, coef, m1, m2, a, slope):
    """rows of one chunk -> (draw, S_draw, dres = dpre, S_dres: 0 where dres is a copy of dy or a zero)"""
    d = dact(pos, a, f32(slope))
    dpre = dy.double() * d
    S_dres = torch.where((d == 1) | (d == 0), torch.zeros_like(dpre), dpre.abs())
    if mean is not None:
        xhat = (raw.double() - mean.double()) * invstd.double()
        draw = coef.double() * (dpre - m1 - xhat * m2)
        S = coef.double().abs() * (dpre.abs() + m1.abs() + xhat.abs() * m2.abs())
    elif coef is not None:
        draw, S = coef.double() * dpre, coef.double().abs() * dpre.abs()
    else:
        draw, S = dpre, S_dres
    return draw, S, dpre, S_dres


def bwd_finalize_f32(stats, count):
    """stats [rows][2][C] fp32 -> (sums [2][C], bound [2][C]); the means are sums / count"""
    st = stats.double()
    return st.sum(0), st.abs().sum(0)


def _pool_dpre(dy_pool, raw, pscale, pshift, a, slope):
    w, pre, e, _ = _affine_windows(raw, pscale, pshift, a, slope)
    best, _ = first_max(e)
    z = torch.zeros((), dtype=torch.float64, device=raw.device)
    dpre = torch.where(one_hot_window(best), dy_pool.double().unsqueeze(0) * dact(pre > 0, a, f32(slope)), z)
    return w, dpre


def pool_bn_bwd_reduce(dy_pool, raw, mean, invstd, pscale, pshift, a, slope):
    """-> (sums [2][C], bound [2][C]) over all B*H*W positions (dpre = 0 outside the winners); batch by batch"""
    C = raw.shape[-1]
    s = torch.zeros((2, C), dtype=torch.float64, device=raw.device)
    bnd = torch.zeros_like(s)
    for b in range(raw.shape[0]):
        w, dpre = _pool_dpre(dy_pool[b:b + 1], raw[b:b + 1], pscale, pshift, a, slope)
        t = dpre * ((w - mean.double()) * invstd.double())
        s[0] += dpre.sum((0, 1, 2, 3))
        s[1] += t.sum((0, 1, 2, 3))
        bnd[0] += dpre.abs().sum((0, 1, 2, 3))
        bnd[1] += t.abs().sum((0, 1, 2, 3))
    return s, bnd


def pooled_from_raw(mean, invstd, pscale, pshift):
    """the channels of efgh_pool_bn_bwd_reduce_pooled whose xhat comes from raw: gamma == 0 or |beta| > POOLED_BETA_GAMMA |gamma|"""
    beta = mean.double() * pscale.double() + pshift.double()
    return (pscale == 0) | (beta.abs() * invstd.double().abs() > POOLED_BETA_GAMMA * pscale.double().abs())


def pool_bn_bwd_reduce_pooled(dy_pool, y_pool, raw, mean, invstd, pscale, pshift, from_raw=None):
    """the same sums of a ReLU layer from the pooled gradient and the pooled activation.  from_raw [C] bool: the channels whose xhat
    comes from raw at the window's winner (gamma == 0: its first element); None: those of pooled_from_raw.
    -> (sums [2][C], bound [2][C] on this formulation: |d| (|y| + |beta|) / |gamma| per term, |d||xhat| for a from-raw channel)"""
    C = raw.shape[-1]
    mu, inv, psc, psh = mean.double(), invstd.double(), pscale.double(), pshift.double()
    beta = mu * psc + psh
    flat0 = psc == 0
    fr = pooled_from_raw(mean, invstd, pscale, pshift) if from_raw is None else (from_raw | flat0)
    rg = torch.where(flat0, torch.zeros_like(psc), inv / torch.where(flat0, torch.ones_like(psc), psc))
    s = torch.zeros((2, C), dtype=torch.float64, device=raw.device)
    bnd = torch.zeros_like(s)
    z = torch.zeros((), dtype=torch.float64, device=raw.device)
    for b in range(raw.shape[0]):
        y, g = y_pool[b].double(), dy_pool[b].double()
        d = torch.where(y > 0, g, z)
        xh, xs = (y - beta) * rg, (y.abs() + beta.abs()) * rg.abs()
        if bool(fr.any()):
            w, _, e, _ = _affine_windows(raw[b:b + 1], pscale, pshift, ACT_RELU, 0.0)
            best, _ = first_max(e)
            wr = torch.where(one_hot_window(best), w, z).sum(0)[0]             # raw at the winner (gamma == 0: the first element)
            xr = (wr - mu) * inv
            xh, xs = torch.where(fr, xr, xh), torch.where(fr, xr.abs(), xs)
        s[0] += d.sum((0, 1))
        s[1] += (d * xh).sum((0, 1))
        bnd[0] += d.abs().sum((0, 1))
        bnd[1] += (d.abs() * xs).sum((0, 1))
    return s, bnd


def pool_bn_bwd_apply(dy_pool, raw, mean, invstd, coef, m1, m2, pscale, pshift, a, slope):
    """one batch slice -> (draw [B][H][W][C], S): coef*(dpre - m1 - xhat*m2), dpre = 0 outside the winners and on the odd rim"""
    B, H, W, C = raw.shape
    _, dpre4 = _pool_dpre(dy_pool, raw, pscale, pshift, a, slope)
    dpre = unwindows(dpre4, H, W)
    xhat = (raw.double() - mean.double()) * invstd.double()
    draw = coef.double() * (dpre - m1 - xhat * m2)
    return draw, coef.double().abs() * (dpre.abs() + m1.abs() + xhat.abs() * m2.abs())


# ------------------------------------------------------------------------------------------------ comparison
def cmp(cls, label, got, ref, S):
    """-> number of elements over TAU_BN[cls] * S + DELTA; records the largest |got - ref| / S of the class in OBSERVED.
    cls 'exact': bit-exact (got is fp32, ref the float64 value of an fp32 number)"""
    if cls == 'exact':
        return int((got.contiguous().view(torch.int32) != ref.float().contiguous().view(torch.int32)).sum())
    g = got.double()
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float('inf')))
    ratio = float(((err - DELTA).clamp_min(0) / (S + 1e-300)).max()) if err.numel() else 0.0
    if ratio > OBSERVED.get(cls, (-1.0, ''))[0]:
        OBSERVED[cls] = (ratio, label)
    return int((err > TAU_BN[cls] * S + DELTA).sum())


def view2(buf, off, ld, M, C):
    """[M][C] view of rows of pitch ld from element `off` of the 1-D buffer `buf` (bounds checked: what a raw pointer would reach)"""
    f = flat(buf)
    assert off >= 0 and M >= 1 and off + (M - 1) * ld + C <= f.numel(), 'view out of range'
    return torch.as_strided(f, (M, C), (ld, 1), f.storage_offset() + off)


def outside_unchanged(buf, before, off, ld, M, C):
    """elements of `buf` outside rows [M][C] of pitch ld at `off` whose bits differ from `before`"""
    a, b = buf.view(torch.int32), before.view(torch.int32)
    end = off + (M - 1) * ld + C
    n = int((a[:off] != b[:off]).sum()) + int((a[end:] != b[end:]).sum())
    if ld > C and M > 1:
        n += int((view2(a, off + C, ld, M - 1, ld - C) != view2(b, off + C, ld, M - 1, ld - C)).sum())
    return n


# ------------------------------------------------------------------------------------------------ inputs
EPS = 1e-5
# BatchNorm parameter sets, one per channel within a launch: channel c takes set PATTERN[c % 8]
ORDINARY, GAMMA0, GAMMA_NEG, SMALL_GAMMA, CONSTANT, OFFSET = range(6)
PATTERN = [ORDINARY, GAMMA0, GAMMA_NEG, SMALL_GAMMA, ORDINARY, CONSTANT, OFFSET, ORDINARY]
# efgh_pool_bn_bwd_reduce_pooled takes xhat from raw where |beta| > POOLED_BETA_GAMMA * |gamma| (EFGH_POOLED_BETA_GAMMA of backward.hip).
# Measured on the MI355X without the bound (4x32x32x64, every channel at one |beta|/|gamma|, a one-signed pooled gradient - the
# rounding of beta is common to a channel's terms): m2 is 0.96-1.46 x 2^-24 of sum |d||xhat| / count off at |beta|/|gamma| = 1,
# 1.73-1.89 at 2, 1.97-2.87 at 3, 2.94-3.88 at 4, 6.9 at 8, 50 at 64, 301 at 1000 (from raw: <= 0.82 up to 3, 1.56 at 4); the ceiling of m1 / m2
# is 3 x 2^-24, so the bound is 2
POOLED_BETA_GAMMA = 2.0
AMB_REL = 1e-3           # a pre-activation / a window's top two closer than this (x S) could be decided differently in fp32
PUSH = 0.25


def bn_params(C, seed, device, pattern=None):
    """per-channel BatchNorm state of a launch -> dict(gamma, beta, mean, std, invstd, scale, shift, sets), fp32 on `device`"""
    g = torch.Generator().manual_seed(seed)
    pattern = PATTERN if pattern is None else pattern
    sets = torch.tensor([pattern[c % len(pattern)] for c in range(C)])
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    mean = 0.1 * torch.randn(C, generator=g)
    std = 0.8 + 0.4 * torch.rand(C, generator=g)
    gamma = torch.where(sets == GAMMA0, torch.zeros(C), gamma)
    beta = torch.where(sets == GAMMA0, torch.full((C,), 0.3), beta)
    gamma = torch.where(sets == GAMMA_NEG, -gamma, gamma)
    gamma = torch.where(sets == SMALL_GAMMA, torch.full((C,), 1e-3), gamma)
    beta = torch.where(sets == SMALL_GAMMA, torch.ones(C), beta)
    std = torch.where(sets == CONSTANT, torch.zeros(C), std)
    mean = torch.where(sets == CONSTANT, torch.full((C,), 2.0 ** -6), mean)
    gamma = torch.where(sets == CONSTANT, torch.ones(C), gamma)
    beta = torch.where(sets == CONSTANT, torch.where(torch.arange(C) % 16 < 8, torch.full((C,), 0.5), torch.full((C,), -0.5)), beta)
    mean = torch.where(sets == OFFSET, 30 * std, mean)
    invstd = (1.0 / torch.sqrt(std.double() ** 2 + EPS)).float()
    scale = gamma * invstd
    shift = beta - mean * scale
    out = dict(gamma=gamma, beta=beta, mean=mean, std=std, invstd=invstd, scale=scale, shift=shift)
    out = {k: v.float().to(device) for k, v in out.items()}
    out['sets'] = sets.to(device)
    return out


def _randn(shape, seed, device):
    """seeded N(0,1) fp32, generated on `device` in slices (the large cases never exist on the host)"""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(shape, generator=g, device=device, dtype=torch.float32)


def ambiguous(raw, scale, shift, res, a, slope, pool):
    """-> (elements whose float64 pre-activation has |pre| < AMB_REL * S, [pool] windows whose top two float64 activated values differ by
    less than AMB_REL * S without being equal): bool masks shaped like raw / like the pooled map.  pool: raw is [B][H][W][C]"""
    _, S, pre = scale_shift_act(raw, scale, shift, res, ACT_NONE, 0.0)
    near0 = pre.abs() < AMB_REL * S
    if not pool:
        return near0, None
    _, _, e, S4 = _affine_windows(raw, scale, shift, a, slope)
    v = e.sort(dim=0, descending=True).values
    return near0, (v[0] - v[1] < AMB_REL * S4.amax(0)) & (v[0] != v[1])


def settle(raw, scale, shift, res, a, slope, pool):
    """move the elements of `raw` (fp32, in place) on which an fp32 kernel and the float64 reference could legitimately take
    different branches: a pre-activation within AMB_REL * S of 0 goes PUSH away from 0 (raw -+ PUSH / scale); in a pooled window
    whose top two activated values are within AMB_REL * S of each other without being equal, the first of the two goes PUSH above
    the other.  Exact ties stay.  -> the size of the ambiguous set that is left (the caller asserts 0)"""
    sc, sh = scale.double(), shift.double()
    live = (sc != 0).expand(raw.shape)
    for _ in range(8):
        near0, tie = ambiguous(raw, scale, shift, res, a, slope, pool)
        n = int((near0 & live).sum()) + (int(tie.sum()) if tie is not None else 0)
        if n == 0:
            break
        pre = raw.double() * sc + sh + (res.double() if res is not None else 0)
        sgn = torch.where(pre < 0, -torch.ones_like(pre), torch.ones_like(pre))
        new = torch.where(near0 & live, raw.double() + sgn * PUSH / torch.where(sc == 0, torch.ones_like(sc), sc), raw.double())
        raw.copy_(new.float())
        if not pool:
            continue
        w, pre4, e, _ = _affine_windows(raw, scale, shift, a, slope)
        _, tie = ambiguous(raw, scale, shift, res, a, slope, pool)
        order = e.sort(dim=0, descending=True, stable=True).indices
        first = torch.minimum(order[0], order[1])                           # the first of the top two, scan order
        top = e.amax(0)
        t = top + PUSH                                                      # its new activated value (not one next to 0)
        t = torch.where(t.abs() < PUSH / 2, t + PUSH, t)
        s = f32(slope)
        want = torch.where((t > 0) | torch.tensor(a != ACT_LEAKY or s <= 0, device=t.device), t, t / (s if s > 0 else 1.0))
        hit = one_hot_window(first) & tie.unsqueeze(0) & (sc != 0)
        w = torch.where(hit, w + (want.unsqueeze(0) - pre4) / torch.where(sc == 0, torch.ones_like(sc), sc), w)
        B, H, W, C = raw.shape
        raw[:, :2 * (H // 2), :2 * (W // 2)] = unwindows(w, 2 * (H // 2), 2 * (W // 2)).float()
    near0, tie = ambiguous(raw, scale, shift, res, a, slope, pool)
    return int((near0 & live).sum()) + (int(tie.sum()) if tie is not None else 0)


def gen_rows(M, C, seed, device, a, slope, with_res=False, pattern=None):
    """inputs of an [M][C] launch: BatchNorm state p, raw (settled), dy, res"""
    p = bn_params(C, seed, device, pattern)
    res = _randn((M, C), seed + 2, device) if with_res else None
    raw = torch.empty((M, C), dtype=torch.float32, device=device)
    left = 0
    for r0, r1 in row_chunks(M, C):
        raw[r0:r1] = _randn((r1 - r0, C), seed * 1000003 + r0, device) * p['std'] + p['mean']
        left += settle(raw[r0:r1], p['scale'], p['shift'], None if res is None else res[r0:r1], a, slope, False)
    return dict(p=p, raw=raw, dy=_randn((M, C), seed + 1, device), res=res, ambiguous=left)


def gen_pool(B, H, W, C, seed, device, a, slope, pattern=None, ties=False, params=None):
    """inputs of a pooled launch: BatchNorm state p, raw [B][H][W][C] (settled), dy_pool; ties: the exact ties of plant_ties"""
    p = bn_params(C, seed, device, pattern) if params is None else params
    raw = torch.empty((B, H, W, C), dtype=torch.float32, device=device)
    left = 0
    for b in range(B):
        raw[b] = _randn((H, W, C), seed * 1000003 + b, device) * p['std'] + p['mean']
        if ties and b == 0:
            plant_ties(raw[b], p)
        left += settle(raw[b:b + 1], p['scale'], p['shift'], None, a, slope, True)
    return dict(p=p, raw=raw, dy_pool=_randn((B, H // 2, W // 2, C), seed + 1, device), ambiguous=left)


def plant_ties(img, p):
    """exact ties, decided identically in fp32 and float64, in the windows (0,0) .. (0,3) of an [H][W][C] image (H >= 2, W >= 8) for
    every channel with scale != 0, as pre-activation targets: four equal values; two equal maxima at window positions 1 and 2;
    two equal maxima at 0 and 3; all four non-positive (ReLU: four zeros; leaky: two equal slope-scaled negatives on top)"""
    sc, sh = p['scale'].double(), p['shift'].double()
    ok = sc != 0
    T = [[1.5, 1.5, 1.5, 1.5], [-1.0, 2.0, 2.0, 0.5], [2.5, -0.5, 1.0, 2.5], [-2.0, -1.0, -1.0, -3.0]]
    for j, t in enumerate(T):
        for q, v in enumerate(t):
            h, w = q // 2, 2 * j + q % 2
            tgt = ((v - sh) / torch.where(ok, sc, torch.ones_like(sc))).float()
            img[h, w] = torch.where(ok, tgt, img[h, w])


# ------------------------------------------------------------------------------------------------ the cases of the GPU module
ACTS = [(ACT_NONE, 0.0), (ACT_RELU, 0.0), (ACT_LEAKY, 0.2), (ACT_LEAKY, 0.0)]
# rows x channels of the [M][C] launches.  C: 4 = one quad lane; 36 = 9 quads in 16 lanes (the c < C guard); 260 = 64 lanes and a
# second channel block with one live lane; 32 / 96 = the sign-bits forms.  M: 1; 17 = two groups, the second with one row; 2083 =
# 131 groups (the unrolled fold runs for some lanes only); 16 400 = 32 rows per group, 513 groups
ROW_CASES = [(1, 4), (17, 36), (17, 64), (2083, 32), (2083, 260), (16400, 96), (16400, 4), (131, 64)]
ROWS_STRIDE = (70000, 256)       # above 16 384 x 256 quads: the grid-stride loop takes a second trip (72 MB)
SCALAR_STRIDE = (1398200, 3)     # above 16 384 x 256 elements: the second trip of the scalar fallback of efgh_scale_shift_act (17 MB)
# (B, H, W, C) of the pooled launches
POOL_CASES = [(1, 2, 2, 4), (3, 2, 3, 36), (1, 3, 2, 64), (3, 5, 7, 260), (1, 8, 6, 32), (3, 8, 6, 96), (2, 2, 8, 64)]
POOL_TIES = (2, 2, 8, 64)        # the case that carries the planted exact ties
POOL_RATIO = (4, 32, 32, 256)    # channels at |beta| / |gamma| = RATIOS: either side of the bound of efgh_pool_bn_bwd_reduce_pooled
RATIOS = [1.9, 6.0, 64.0, 8.0]       # 2 is the bound; measured without it: 1.9 x 2^-24 at 2, 3.9 - 4.5 at 6, 6.9 at 8, 50 at 64 (ceiling 3)
POOL_STRIDE = (17, 64, 64, 1024)  # 17 * 32 * 32 windows x 256 quads > 16 384 x 256 (285 MB)
POOL_NT = (96, 64, 64, 256)      # B*H*W*C*4 = 384 MiB exactly: the non-temporal instances
ROWS_NT = (393216, 256)          # the same tensor as [M][C] rows (a settled pooled case is a settled rows case): M*C*4 = 384 MiB
POOL_NT_POOLED = (96, 128, 128, 256)   # efgh_pool_bn_bwd_reduce_pooled switches on the POOLED size: raw is 1.5 GiB
assert ROWS_NT == (POOL_NT[0] * POOL_NT[1] * POOL_NT[2], POOL_NT[3])
# the other generated cases of the module: the two-stage fold, the scalar fallback, the aliasing and the NaN case
FOLD_ROWS = [131072, 131073]
SCALAR_CASES = [(3, 3, 0), (1, 1, 0), (3, 5, 2), (8, 8, 1), (8, 9, 0)]       # (C, ldx, offset of x in floats)
SCALAR_ROWS, ALIAS_CASE, NAN_CASE = 301, (517, 64), (67, 64)


def case_seed(shape, a, slope):
    return (sum(int(v) * k for v, k in zip(shape, (1, 131, 17161, 2248091))) + 7 * a + int(slope * 10)) % (2 ** 31)


# the cases above 256 MB run one activation each, SCALAR_STRIDE two (every activation runs at every other shape; the activation is a
# run-time argument of one instance, so the size and the activation do not interact)
LARGE_ACTS = {ROWS_STRIDE: ACTS, SCALAR_STRIDE: [(ACT_RELU, 0.0), (ACT_LEAKY, 0.2)], POOL_STRIDE: [(ACT_LEAKY, 0.2)],
              POOL_NT: [(ACT_RELU, 0.0)], ROWS_NT: [(ACT_RELU, 0.0)], POOL_NT_POOLED: [(ACT_RELU, 0.0)]}


def host_cases():
    """(kind, shape, act, slope) of every generated case of the GPU module but the two largest by size (the 384 MiB tensor of the
    non-temporal instances, POOL_NT / ROWS_NT, and the 1.5 GiB one of POOL_NT_POOLED): the host test generates them on the CPU"""
    out = []
    for sh in ROW_CASES:
        out += [('rows', sh, a, s) for a, s in ACTS] + [('rows_res', sh, a, s) for a, s in ACTS]
    out += [('rows', (M, 8), ACT_NONE, 0.0) for M in FOLD_ROWS]
    for sh in sorted({(SCALAR_ROWS, c[0]) for c in SCALAR_CASES}) + [ALIAS_CASE]:
        out += [('rows_res', sh, a, s) for a, s in ACTS]
    out += [('rows', NAN_CASE, a, s) for a, s in ACTS]
    out += [('rows', ROWS_STRIDE, a, s) for a, s in LARGE_ACTS[ROWS_STRIDE]]
    out += [('rows_res', SCALAR_STRIDE, a, s) for a, s in LARGE_ACTS[SCALAR_STRIDE]]
    for sh in POOL_CASES:
        out += [('pool', sh, a, s) for a, s in ACTS]
    out += [('pool_ratio', POOL_RATIO, ACT_RELU, 0.0)]
    out += [('pool', POOL_STRIDE, a, s) for a, s in LARGE_ACTS[POOL_STRIDE]]
    return out


def ratio_params(C, seed, device):
    """ordinary statistics with gamma in (1, 0.1, -1) and beta = +- ratio * |gamma|, ratio = RATIOS[c % 4]; the channels at 6 and 8 all have
    gamma = 1, beta > 0 (measured the worst of the six combinations; the rounding of beta differs from channel to channel, so it takes
    many channels to meet a bad one) -> bn_params' dict + ratio"""
    p = bn_params(C, seed, 'cpu', pattern=[ORDINARY])
    c = torch.arange(C)
    gamma = torch.tensor([1.0, 0.1, -1.0])[(c // 4) % 3]
    ratio = torch.tensor(RATIOS)[c % 4]
    gamma = torch.where((ratio == 6.0) | (ratio == 8.0), torch.ones(C), gamma)
    beta = torch.where(((c // 12) % 2 == 0) | (ratio == 6.0) | (ratio == 8.0), ratio, -ratio) * gamma.abs()
    p['gamma'], p['beta'], p['ratio'] = gamma, beta, ratio
    p['scale'] = gamma * p['invstd']
    p['shift'] = beta - p['mean'] * p['scale']
    return {k: v.to(device) for k, v in p.items()}


def gen_case(kind, shape, a, slope, device):
    seed = case_seed(shape, a, slope)
    if kind == 'pool_ratio':
        c = gen_pool(*shape, seed, device, a, slope, params=ratio_params(shape[3], seed, device))
        c['dy_pool'] = c['dy_pool'].abs()           # one-signed: the rounding of beta, common to a channel's terms, does not average out
        return c
    if kind == 'pool':
        return gen_pool(*shape, seed, device, a, slope, ties=tuple(shape) == POOL_TIES)
    return gen_rows(*shape, seed, device, a, slope, with_res=kind == 'rows_res')
