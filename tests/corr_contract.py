"""float64 reference of the F correlation head (test helper): the 13 entry points of csrc/corr.hip and the correlation kernels of
csrc/backward.hip, written once from the comments at the top of corr.hip and from the reference expression (nets/fnet.py:57-81,
torch_utils.py:271-284), independent of the kernel bodies and of oracle/.  unfold / einsum / matmul only.

Feature maps are channels-last [B][h][w][16]; every sample is evaluated on its own.  Every function takes the fp32 tensors a kernel
gets (any device), computes in float64 and returns the value with the scale S of its error bound.  Error model, element by element,
as in gemm_contract.py and bn_contract.py:

    |got - ref| <= tau[class] * S + DELTA,        tau[class] <= ceiling(class, shape, route)

S is the same expression on magnitudes: |x|/d for a normalised value, the sum of |rp||cam_n| / 16 for a logit, the sums of |dl||rp|
and |dl||cam_n| for the two correlation gradients, the three |terms| of the fold of the pad, |dxn|/d + [tie] sum|dxn x| / (d^2 k) for
the gradient of the normalisation.  The score carries S_logit / 4 (the largest slope of the sigmoid) and its own two roundings.
The minimum / maximum, the re-layouts that only copy, and every padding element are exact: bit-equal, padding exactly zero.

Semantics, stated once:
  d            max - min of the sample, the difference of the two fp32 numbers of mm taken in float64
  pad          [mirror(last off columns) | x/d | first off columns | zeros up to wpitch], off = int(wr / 8)
  logit        sum over rows y, camera columns x, channels c of rp[b][y][j+x][c] * cam_n[b][y][x][c], divided by 16
  ties         max() / min() hand their gradient to every element that attains the extremum, in equal parts; -0.0 == +0.0
  unspecified  d = 0 (the reference divides by zero too) and NaN inputs (fminf / fmaxf drop a NaN where torch propagates it)"""
import torch

from gemm_contract import DELTA

ENTRY_POINTS = [
    'efgh_minmax', 'efgh_corr_pad', 'efgh_corr1d', 'efgh_corr_pack_cam', 'efgh_corr_fold', 'efgh_corr_planes', 'efgh_corr_unplanes',
    'efgh_corr_toeplitz', 'efgh_corr1d_bwd', 'efgh_corr_unpad', 'efgh_norm_bwd',
]
JT = 4                   # shifts per thread of the VALU forward (corr.hip)
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ route geometry (ops.corr_head)
def ceil4(v):
    return (v + 3) // 4 * 4


def geometry(h, wc, wr):
    """the sizes the head derives from a shape: off, wp, nj, and the MFMA forward's segw, nseg (padded), nseg_real, nsplit, T"""
    off = int(wr / 8)
    wp = wr + 2 * off
    segw = (wc + 31) // 32
    nseg_real = (wc + segw - 1) // segw
    nsplit = max(d for d in range(1, 17) if h % d == 0)
    return dict(off=off, wp=wp, nj=wp - wc + 1, segw=segw, nseg=ceil4(nseg_real), nseg_real=nseg_real, nsplit=nsplit, T=h // nsplit)


def minmax_groups(n):
    return min(1024, max(1, (n + 2047) // 2048))


# ------------------------------------------------------------------------------------------------ ceilings
# They follow from the arithmetic and hold whatever is measured.  A sum of K fp32 terms, in any order, is off by at most
# (K - 1) u sum|term| to first order (u = 2^-24); a term that was itself rounded r times adds r u.
CEIL_ELEM = 4 * U        # x/d: the fp32 d (1), the quotient (1); as x * (1/d) in efgh_corr_planes: d, the reciprocal, the product (3); +1
CEIL_UNPAD = 3 * U       # three terms: two additions; the issue's "three roundings"
CEIL_SIGMOID = 5 * U     # relative to the score s: expf within 1 ulp (2 u of e, so 2 u (1 - s) of s), 1 + e (1), the quotient (1); +1
C_OPERANDS = 12          # per term of a sum: rp (2) and cam_n (3) as rounded above, the product (1), the 16-channel tree of the VALU
#                          kernel (5), the scale by 1/16 (exact); +1


def ceil_logit(mfma, h, wc, wr):
    """VALU: the thread's chain over the wc camera columns, then efgh_corr1d's chain over the h rows.  MFMA: the GEMM's depth
    T * segw * 16 in whatever order the kernel takes it, then the nsplit * nseg partials efgh_corr_fold adds"""
    g = geometry(h, wc, wr)
    K = g['T'] * g['segw'] * 16 + g['nsplit'] * g['nseg'] if mfma else wc + h
    return (K + C_OPERANDS) * U


def ceil_corr_bwd(mfma, h, wc, wr):
    """-> (ceiling of dcam_n, ceiling of drp).  VALU: one chain over the nj shifts, resp. over the at most min(wc, nj) camera columns
    a padded column meets.  MFMA: the depth of the two plane GEMMs, wp and wc rounded up to 4"""
    g = geometry(h, wc, wr)
    if mfma:
        return (ceil4(g['wp']) + C_OPERANDS) * U, (ceil4(wc) + C_OPERANDS) * U
    return (g['nj'] + C_OPERANDS) * U, (min(wc, g['nj']) + C_OPERANDS) * U


def ceil_norm(n):
    """T = sum dxn * x: a thread's chain of ceil(n / (G * 256)) products, the 64-lane tree (6), the four waves (3), the float64 fold
    and its cast (1), the product (1); then d (1), d * d (2 with d's), T / d^2 (1), / k (1), dxn / d (1), the difference (1); +1"""
    return (-(-n // (minmax_groups(n) * 256)) + 19) * U


# tau per class: at most 4x the largest |got - ref| / S observed on an MI355X over every case of tests/test_gpu_corr_contract.py
# (the observed maximum and its case in the comment; the kernels are deterministic), and never above the ceiling of the case: cmp()
# takes the smaller of the two.  None would mean not measured: the ceiling alone holds.
TAU = {
    'elem': CEIL_ELEM,        # 6.623e-08 (1.11 x 2^-24): efgh_corr_planes with mm on the padded rp of 2x7x33x85; 4x is above the ceiling
    'logit': 3.6e-7,          # 9.145e-08 (1.53 x 2^-24): eval 1x2x5x900 on the MFMA route (nj = 1120)
    'sigmoid': CEIL_SIGMOID,  # 1.164e-07 (1.95 x 2^-24): eval 1x2x5x900 on the VALU route; 4x is above the ceiling
    'corr_bwd': 2.3e-6,       # 5.843e-07 (9.80 x 2^-24): dcam_n of training 1x2x5x900 on the MFMA route (plane GEMM of depth 1124)
    'unpad': CEIL_UNPAD,      # 5.960e-08 (1.00 x 2^-24): training 1x32x64x264; 4x is above the ceiling
    'norm': 3.1e-7,           # 7.790e-08 (1.31 x 2^-24): ops.norm_bwd alone, n = 2052 (two groups), extremum in the first element
}
OBSERVED = {}            # class -> (largest |got - ref| / S, the case that produced it): filled by cmp(), printed by the last GPU test


def tau_of(cls, ceiling):
    return ceiling if TAU[cls] is None else min(TAU[cls], ceiling)


def exact(got, ref):
    """number of elements of the fp32 `got` whose bits differ from the float64 value `ref` of an fp32 number"""
    return int((got.contiguous().view(torch.int32) != ref.float().contiguous().view(torch.int32)).sum())


def cmp(cls, label, got, ref, S, ceiling, extra=None):
    """-> number of elements over min(TAU[cls], ceiling) * S (+ extra) + DELTA; records the largest (|got - ref| - extra) / S of the
    class in OBSERVED.  `extra` is a bound carried in from an earlier stage (the score: tau_logit * S_logit / 4)"""
    g = got.double()
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float('inf')))
    slack = DELTA if extra is None else extra + DELTA
    ratio = float(((err - slack).clamp_min(0) / (S + 1e-300)).max()) if err.numel() else 0.0
    if ratio > OBSERVED.get(cls, (-1.0, ''))[0]:
        OBSERVED[cls] = (ratio, label)
    return int((err > tau_of(cls, ceiling) * S + slack).sum())


# ------------------------------------------------------------------------------------------------ forward
def minmax(x):
    """efgh_minmax: x [B][...] -> mm [B][2] fp32 (min, max) per sample; exact (a zero's sign is not specified: -0.0 == +0.0)"""
    f = x.reshape(x.shape[0], -1)
    return torch.stack([f.amin(1), f.amax(1)], 1)


def _d(mm):
    return mm[:, 1].double() - mm[:, 0].double()


def normalise(x, mm):
    """x [B][h][w][C] -> x / d in float64, and its magnitude"""
    v = x.double() / _d(mm).view(-1, 1, 1, 1)
    return v, v.abs()


def normalise_pad(rng, mm, off, wpitch):
    """efgh_corr_pad: rng [B][h][w][C] -> rp [B][h][wpitch][C] = [mirror(last off) | x/d | first off | zeros up to wpitch]"""
    B, h, w, C = rng.shape
    assert 0 <= off <= w and wpitch >= w + 2 * off
    xn, _ = normalise(rng, mm)
    left = torch.flip(xn[:, :, w - off:], dims=[2])
    zeros = torch.zeros((B, h, wpitch - w - 2 * off, C), dtype=torch.float64, device=rng.device)
    ref = torch.cat([left, xn, xn[:, :, :off], zeros], 2)
    return ref, ref.abs()


def _windows(rp, wc):
    """rp [B][h][wp][C] -> [B][h][nj][C][wc]: the wc padded columns under shift j (a view)"""
    return rp.unfold(2, wc, 1)


def logits_from(rp, cam_n):
    """rp [B][h][wp][C], cam_n [B][h][wc][C] (float64) -> (logit [B][nj], S)"""
    wc = cam_n.shape[2]
    ref = torch.einsum('byjcx,byxc->bj', _windows(rp, wc), cam_n) / 16
    S = torch.einsum('byjcx,byxc->bj', _windows(rp.abs(), wc), cam_n.abs()) / 16
    return ref, S


def logits(cam, rng):
    """the head's logit from the raw fp32 feature maps: cam [B][h][wc][16], rng [B][h][wr][16] -> (logit [B][nj], S)"""
    wr = rng.shape[2]
    off = int(wr / 8)
    rp, _ = normalise_pad(rng, minmax(rng), off, wr + 2 * off)
    cam_n, _ = normalise(cam, minmax(cam))
    return logits_from(rp, cam_n)


def score(logit, S_logit):
    """-> (sigmoid(logit), the part of the bound that scales with tau_logit: S_logit / 4, the part that scales with tau_sigmoid)"""
    s = torch.sigmoid(logit)
    return s, S_logit / 4, s


# ------------------------------------------------------------------------------------------------ backward
def dl_toeplitz(dl, rows_x, rows_m):
    """Tm [B][m][x] = dl[b][m - x], zero outside [0, nj): m < rows_m = nj + rows_x - 1, x < rows_x"""
    B, nj = dl.shape
    assert rows_m == nj + rows_x - 1
    z = torch.zeros((B, rows_x - 1), dtype=dl.dtype, device=dl.device)
    return torch.cat([z, dl, z], 1).unfold(1, rows_x, 1).flip(-1)


def corr_bwd(rp, cam_n, dl):
    """rp [B][h][wp][C], cam_n [B][h][wc][C], dl [B][nj] (float64) -> (dcam_n, S, drp, S):
    dcam_n[b][y][x][c] = sum_j dl[b][j] rp[b][y][j+x][c],  drp[b][y][m][c] = sum_x dl[b][m-x] cam_n[b][y][x][c]"""
    wc, wp = cam_n.shape[2], rp.shape[2]
    dcam = torch.einsum('bj,byjcx->byxc', dl, _windows(rp, wc))
    S_dcam = torch.einsum('bj,byjcx->byxc', dl.abs(), _windows(rp.abs(), wc))
    Tm = dl_toeplitz(dl, wc, wp)
    drp = torch.einsum('bmx,byxc->bymc', Tm, cam_n)
    S_drp = torch.einsum('bmx,byxc->bymc', Tm.abs(), cam_n.abs())
    return dcam, S_dcam, drp, S_drp


def unpad(drp, w, off):
    """efgh_corr_unpad: drp [B][h][w + 2 off][C] -> drng_n [B][h][w][C]: drp[xs + off] (+ drp[w-1-xs] if w-1-xs < off)
    (+ drp[xs + off + w] if xs < off)"""
    def fold(v):
        o = v[:, :, off:off + w].clone()
        o[:, :, w - off:] += torch.flip(v[:, :, :off], dims=[2])
        o[:, :, :off] += v[:, :, off + w:off + w + off]
        return o
    return fold(drp), fold(drp.abs())


def norm_bwd(x, dxn, mm):
    """efgh_norm_bwd: dx = dxn/d - [x == max] T/(d^2 k_max) + [x == min] T/(d^2 k_min), T = sum dxn * x over the sample"""
    B = x.shape[0]
    xf, gf = x.reshape(B, -1).double(), dxn.reshape(B, -1).double()
    d = _d(mm).view(B, 1)
    at_max, at_min = xf == mm[:, 1].double().view(B, 1), xf == mm[:, 0].double().view(B, 1)
    kmax, kmin = at_max.sum(1, keepdim=True).double(), at_min.sum(1, keepdim=True).double()
    T, Tabs = (gf * xf).sum(1, keepdim=True), (gf * xf).abs().sum(1, keepdim=True)
    ref = gf / d - at_max * (T / (d * d * kmax)) + at_min * (T / (d * d * kmin))
    S = gf.abs() / d + at_max * (Tabs / (d * d * kmax)) + at_min * (Tabs / (d * d * kmin))
    return ref.reshape(x.shape), S.reshape(x.shape)


# ------------------------------------------------------------------------------------------------ re-layouts
def planes(x, mm, w, wP):
    """efgh_corr_planes: x [B][h][pitch >= w][16] -> [B][h * 16][wP], out[b][y*16 + c][m] = x[b][y][m][c] (* 1/d with mm), 0 for
    m >= w.  Without mm a copy (exact); with mm class 'elem'"""
    B, h = x.shape[:2]
    v = x[:, :, :w].double()
    if mm is not None:
        v = v / _d(mm).view(B, 1, 1, 1)
    out = torch.zeros((B, h, 16, wP), dtype=torch.float64, device=x.device)
    out[..., :w] = v.permute(0, 1, 3, 2)
    return out.reshape(B, h * 16, wP)


def unplanes(inp, h, w):
    """efgh_corr_unplanes: in [B][h * 16][wP >= w] -> [B][h][w][16] (a copy)"""
    B, _, wP = inp.shape
    return inp.reshape(B, h, 16, wP)[..., :w].permute(0, 1, 3, 2).double()


def toeplitz(dl, rows, cols, colsP, transpose):
    """efgh_corr_toeplitz: T[b][r][c] = dl[b][c - r] (transpose 0) or dl[b][r - c] (1); zero outside [0, nj) and for c >= cols"""
    B, nj = dl.shape
    r = torch.arange(rows, device=dl.device).view(rows, 1)
    c = torch.arange(colsP, device=dl.device).view(1, colsP)
    j = (r - c) if transpose else (c - r)
    ok = (c < cols) & (j >= 0) & (j < nj)
    return torch.where(ok.unsqueeze(0), dl.double()[:, j.clamp(0, nj - 1)], torch.zeros((), dtype=torch.float64, device=dl.device))


def pack_cam(cam, mm, segw, nseg, nsplit):
    """efgh_corr_pack_cam: Wc[b][ks][s][yy][x*16 + c] = cam[b][ks*T + yy][s*segw + x][c] / d, 0 beyond the camera width"""
    B, h, wc, C = cam.shape
    T = h // nsplit
    v, _ = normalise(cam, mm)
    full = torch.zeros((B, h, nseg * segw, C), dtype=torch.float64, device=cam.device)
    full[:, :, :wc] = v
    out = full.reshape(B, nsplit, T, nseg, segw * C).permute(0, 1, 3, 2, 4).contiguous()
    return out, out.abs()


# ------------------------------------------------------------------------------------------------ inputs
LO, HI = -2.0, 3.0


def quantised(shape, seed, mean):
    """fp32 values on quarter steps in [LO, HI], mean about `mean`: the clamp makes both extrema ties"""
    g = torch.Generator().manual_seed(seed)
    return ((torch.randn(shape, generator=g) + mean) * 4).round().div(4).clamp(LO, HI)


def feature_map(B, h, w, seed, means, plateau_first):
    """[B][h][w][16] with ties at both extrema, sample b drawn around means[min(b, 1)].  Sample 0: a plateau block of identical
    values holding the minimum, a third of the sample (its first or its last rows); sample 1: the maximum alone in the last element,
    the minimum alone in the first; later samples: as drawn"""
    x = torch.stack([quantised((h, w, 16), seed + b, means[min(b, 1)]) for b in range(B)])
    f = x.view(B, -1)
    n = f.shape[1]
    f[:, 0], f[:, n - 1] = LO, HI                       # every sample has d > 0, whatever was drawn
    if plateau_first:
        f[0, 1:1 + n // 3] = LO                         # (rows x columns x channels are contiguous)
    else:
        f[0, n - 1 - n // 3:n - 1] = LO
    if B > 1:
        f[1, 0], f[1, n - 1] = LO - 0.25, HI + 0.25
    return x


def head_inputs(B, h, wc, wr, seed=0):
    """-> (cam [B][h][wc][16], rng [B][h][wr][16], ds [B][nj]) fp32 on the CPU.  The means are non-zero, so that the sums do not
    cancel, and sized so that the logits stay within a few units (a saturated sigmoid would hand the backward a zero gradient):
    with values of mean mu after the division by d, a sample's logit is about h wc mu^2; where a third of each map is the plateau
    a = LO / d (the camera's last rows, the range image's first), about h wc mu (2 a + mu) / 3"""
    hw = h * wc
    means = (min(0.75, 50.0 / hw), min(0.75, 5.0 * (2.0 / hw) ** 0.5))
    g = geometry(h, wc, wr)
    cam = feature_map(B, h, wc, 1000 + 10 * seed, means, False)
    rng = feature_map(B, h, wr, 2000 + 10 * seed, means, True)
    ds = quantised((B, g['nj']), 3000 + seed, 0.5)
    return cam, rng, ds


CASES = [                # (B, h, wc, wr), tests/test_gpu_corr_contract.py and tests/test_corr_contract_host.py
    (2, 1, 1, 8), (1, 3, 10, 8), (2, 3, 5, 24), (2, 7, 33, 85), (2, 8, 32, 85), (1, 17, 65, 150), (3, 12, 37, 150), (1, 32, 64, 264),
    (1, 2, 5, 900), (1, 9, 21, 85),
]
