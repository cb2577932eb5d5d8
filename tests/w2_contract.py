"""float64 reference of the transforms of the 2-D Winograd F(4x4,3x3) layers (test helper): efgh_wino2d_input, efgh_wino2d_input_act,
efgh_wino2d_dy and the two fused gradient-side forms efgh_wino2d_bwd_transforms(_pooled) of include/efgh_hip.h, written from the header
and DESIGN.md (interpolation points 0, +-3/4, +-3/2, inf), independent of the kernel bodies.  The first stage of the fused forms - the
BatchNorm-backward draw, the activation, the pooling winner, the mask sources - is bn_contract's; nothing of it is restated here.

Tile geometry:  TH = ceil(H/4), TW = ceil(W/4);  tile t = (b*TH + ty)*TW + tx;  its window is rows 4ty-1 .. 4ty+4 and columns
4tx-1 .. 4tx+4 of image b, everything outside the image is zero;  V[t][6i+j][c] = (B^T d B)[i][j] over the window,
Gy[t][6i+j][n] = (G4 d4 G4^T)[i][j] over the tile's own 4x4 (window rows / columns 1..4).

Every reference takes fp32 tensors of any strides ([B][H][W][C] views), computes in float64 and returns the value with the scale S of
its bound.  Error model, element by element, as in bn_contract.py:

    |got - ref| <= TAU_W2[class] * S + DELTA

S is the same transform on magnitudes, |B^T| S_in |B| or |G4| S_in |G4^T|, with S_in = |A| (input), the activation's S (input_act),
|G| (dy), S_draw of bn_contract (the fused forms).  dres is bn_contract's: bit-exact where the derivative is 1 or 0, class 'elem' else.

A reference is evaluated for one CHUNK = (b, ty0, ty1) of whole tile rows of one image (tile_row_chunks), so that a launch at the
non-temporal threshold never holds more than a few hundred MB of float64."""
import math
from fractions import Fraction

import torch

import bn_contract as BC
from bn_contract import U
from gemm_contract import DELTA

ENTRY_POINTS = ['efgh_wino2d_input', 'efgh_wino2d_input_act', 'efgh_wino2d_dy', 'efgh_wino2d_bwd_transforms',
                'efgh_wino2d_bwd_transforms_pooled']            # each has a non-temporal instance: T*36*N*4 >= BC.NT_BYTES

# ------------------------------------------------------------------------------------------------ the matrices
_a, _b = Fraction(3, 4), Fraction(3, 2)
_a2, _b2, _1, _0 = _a * _a, _b * _b, Fraction(1), Fraction(0)


def _mat(rows):
    return torch.tensor([[float(v) for v in r] for r in rows], dtype=torch.float64)


BT = _mat([[_a2 * _b2, _0, -(_a2 + _b2), _0, _1, _0],
           [_0, -_a * _b2, -_b2, _a, _1, _0],
           [_0, _a * _b2, -_b2, -_a, _1, _0],
           [_0, -_a2 * _b, -_a2, _b, _1, _0],
           [_0, _a2 * _b, -_a2, -_b, _1, _0],
           [_0, _a2 * _b2, _0, -(_a2 + _b2), _0, _1]])
_POINTS = [_0, _a, -_a, _b, -_b]                                             # and infinity
_F = [Fraction(64, 81), Fraction(-128, 243), Fraction(-128, 243), Fraction(32, 243), Fraction(32, 243)]     # 1 / prod (p - p')
assert all(1 / f == math.prod(p - q for q in _POINTS if q != p) for p, f in zip(_POINTS, _F))
G4 = _mat([[f * p ** k for k in range(4)] for p, f in zip(_POINTS, _F)] + [[_0, _0, _0, _1]])              # 6 x 4: F(3,4), gradient side
G3 = _mat([[f * p ** k for k in range(3)] for p, f in zip(_POINTS, _F)] + [[_0, _0, _1]])                  # 6 x 3: F(4,3), weight side
AT4 = _mat([[p ** k for p in _POINTS] + [_1 if k == 3 else _0] for k in range(4)])                         # 4 x 6: F(4,3) output
AT3 = _mat([[p ** k for p in _POINTS] + [_1 if k == 2 else _0] for k in range(3)])                         # 3 x 6: F(3,4) output (dW)

# ------------------------------------------------------------------------------------------------ the bound
# Ceilings from counting roundings (each of relative size U = 2^-24 against the magnitudes it acts on, so it adds U * S at most):
#   one 1-D B^T pass    v = (d4 - k d2) +- p (d3 - k d1): k d2, the difference | k d1, the difference, the product by p | the sum:
#                       2 on one half of S, 3 on the other, 1 on both -> at most 4 (v0, v5: 2 products, 2 sums -> 4 as well)
#   one 1-D G4 pass     u = ((g0 + k g2) +- (p g1 + q g3)) * f: k g2, the sum | p g1, q g3 (each on its own term), the sum |
#                       the outer sum, the product by f, and f itself (64/81, 128/243, 32/243 are no fp32 numbers: one more
#                       relative U) -> 2 + 1 + 1 + 1 = at most 5
#   the second pass works on the first one's rounded values: its error goes through |B^T| (|G4|), i.e. it stays the same multiple
#   of S, and the second pass adds its own.  Contraction into fused multiply-adds only removes roundings.
#   input of the passes  efgh_wino2d_input / _dy: exact (0).  _input_act: one fused multiply-add and the product by the slope (2).
#                       The fused forms: the float64 draw is rounded to fp32 once (1); its float64 arithmetic is second order.
#   The 0.01 U on top is the second-order slack ((11 U)^2 and the float64 roundings of draw are far below it).
CEIL = {
    'v': 8.01 * U,          # efgh_wino2d_input                 0 + 4 + 4
    'v_act': 10.01 * U,     # efgh_wino2d_input_act             2 + 4 + 4
    'gy': 10.01 * U,        # efgh_wino2d_dy                    0 + 5 + 5
    'vd': 9.01 * U,         # Vd of the two fused forms         1 + 4 + 4
    'gyd': 11.01 * U,       # Gy of the two fused forms         1 + 5 + 5
}
# tau per class: at most 4x the largest |got - ref| / S observed on an MI355X over every case of tests/test_gpu_w2_contract.py (the
# observed maximum and its case in the comment; the kernels are deterministic), never above the ceiling of the class - and 4x every
# observed maximum below is above its ceiling, so each tau is its ceiling
TAU_W2 = {
    'v': CEIL['v'],           # 2.124e-07 (3.56 x 2^-24): efgh_wino2d_input, 1x680x1028, C 64
    'v_act': CEIL['v_act'],   # 2.065e-07 (3.46 x 2^-24): efgh_wino2d_input_act, 1x680x1028, C 64, leaky 0.2
    'gy': CEIL['gy'],         # 2.563e-07 (4.30 x 2^-24): efgh_wino2d_dy, 1x680x1028, N 64
    'vd': CEIL['vd'],         # 2.652e-07 (4.45 x 2^-24): Vd of efgh_wino2d_bwd_transforms_pooled, 1x680x1028, N 64, leaky 0.2
    'gyd': CEIL['gyd'],       # 3.546e-07 (5.95 x 2^-24): Gy of efgh_wino2d_bwd_transforms_pooled, 1x528x1324, N 64, leaky 0.2
}
OBSERVED = {}            # class -> (largest |got - ref| / S, the case that produced it): filled by cmp()


def cmp(cls, label, got, ref, S, factor=1.0, table=None):
    """-> number of elements over factor * TAU_W2[cls] * S + DELTA (a non-finite `got` counts as over).  The classes of bn_contract
    ('exact', 'elem') go to bn_contract.cmp.  factor 2: two results that are each inside tau (the agreement of two forms; those
    comparisons are not recorded in OBSERVED, which holds distances to float64 only)"""
    if cls not in TAU_W2:
        return BC.cmp(cls, label, got, ref, S)
    g = got.double()
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float('inf')))
    if factor == 1.0:
        obs = OBSERVED if table is None else table
        ratio = float(((err - DELTA).clamp_min(0) / (S + 1e-300)).max()) if err.numel() else 0.0
        if ratio > obs.get(cls, (-1.0, ''))[0]:
            obs[cls] = (ratio, label)
    return int((err > factor * TAU_W2[cls] * S + DELTA).sum())


# ------------------------------------------------------------------------------------------------ geometry
def geo(B, H, W):
    """-> (TH, TW, T)"""
    TH, TW = -(-H // 4), -(-W // 4)
    return TH, TW, B * TH * TW


def nt_bytes(B, H, W, N):
    """what efgh_stream_nt is asked about by every entry point here: the bytes of one Winograd-domain tensor"""
    return geo(B, H, W)[2] * 36 * N * 4


def tile_row_chunks(B, H, W, N):
    """[(b, ty0, ty1)]: whole tile rows of one image, at most bn_contract.CHUNK Winograd-domain elements each"""
    TH, TW, _ = geo(B, H, W)
    step = max(1, BC.CHUNK // (TW * 36 * N))
    return [(b, r, min(TH, r + step)) for b in range(B) for r in range(0, TH, step)]


def tiles_of(chunk, H, W):
    """-> (t0, t1): the tiles of a chunk are contiguous"""
    b, r0, r1 = chunk
    TH, TW = -(-H // 4), -(-W // 4)
    return (b * TH + r0) * TW, (b * TH + r1) * TW


def rows_of(chunk, H):
    """-> (y0, y1): the image rows the chunk's tiles own"""
    return 4 * chunk[1], min(4 * chunk[2], H)


def _window_rows(chunk, H):
    return max(4 * chunk[1] - 1, 0), min(4 * chunk[2] + 1, H)


def _windows(v, y_first, chunk, H, W):
    """v: float64 [rows][W][C], image rows from y_first on (at least the chunk's window rows) -> [ty1 - ty0][TW][C][6][6], zeros outside
    the image"""
    _, r0, r1 = chunk
    TW = -(-W // 4)
    lo, hi = 4 * r0 - 1, 4 * r1 + 1
    a, e = _window_rows(chunk, H)
    pad = torch.zeros((hi - lo, 4 * TW + 2, v.shape[-1]), dtype=torch.float64, device=v.device)
    pad[a - lo:e - lo, 1:1 + W] = v[a - y_first:e - y_first]
    return pad.unfold(0, 6, 4).unfold(1, 6, 4)


def _bt(w):
    M = BT.to(w.device)
    return torch.einsum('ik,ytckl,jl->ytijc', M, w, M).reshape(-1, 36, w.shape[2])


def _g4(w):
    M = G4.to(w.device)
    return torch.einsum('ik,ytckl,jl->ytijc', M, w[..., 1:5, 1:5], M).reshape(-1, 36, w.shape[2])


def _bt_mag(w):
    M = BT.abs().to(w.device)
    return torch.einsum('ik,ytckl,jl->ytijc', M, w, M).reshape(-1, 36, w.shape[2])


def _g4_mag(w):
    M = G4.abs().to(w.device)
    return torch.einsum('ik,ytckl,jl->ytijc', M, w[..., 1:5, 1:5], M).reshape(-1, 36, w.shape[2])


def _all_chunks(fn, x, *more):
    """a reference over every chunk of the launch, results concatenated along the first axis (the small cases)"""
    B, H, W, N = x.shape
    parts = [fn(c) for c in tile_row_chunks(B, H, W, N)]
    return tuple(torch.cat([p[k] for p in parts]) for k in range(len(parts[0])))


# ------------------------------------------------------------------------------------------------ the references
def input_ref(A, chunk=None):
    """efgh_wino2d_input: A [B][H][W][C] -> (V [tiles][36][C], S) of the chunk's tiles (None: of all T)"""
    if chunk is None:
        return _all_chunks(lambda c: input_ref(A, c), A)
    B, H, W, C = A.shape
    a, e = _window_rows(chunk, H)
    w = _windows(A[chunk[0], a:e].double(), a, chunk, H, W)
    return _bt(w), _bt_mag(w.abs())


def input_act_ref(A, scale, shift, act, slope, chunk=None):
    """efgh_wino2d_input_act: the same transform of act(A*scale + shift); outside the image the ACTIVATION is zero (not act(shift))"""
    if chunk is None:
        return _all_chunks(lambda c: input_act_ref(A, scale, shift, act, slope, c), A)
    B, H, W, C = A.shape
    a, e = _window_rows(chunk, H)
    y, S, _ = BC.scale_shift_act(A[chunk[0], a:e], scale, shift, None, act, slope)
    return _bt(_windows(y, a, chunk, H, W)), _bt_mag(_windows(S, a, chunk, H, W))


def dy_ref(G, chunk=None):
    """efgh_wino2d_dy: G [B][H][W][N] -> (Gy [tiles][36][N], S)"""
    if chunk is None:
        return _all_chunks(lambda c: dy_ref(G, c), G)
    B, H, W, N = G.shape
    a, e = _window_rows(chunk, H)
    w = _windows(G[chunk[0], a:e].double(), a, chunk, H, W)
    return _g4(w), _g4_mag(w.abs())


def _both(draw, S, a, chunk, H, W):
    wd, ws = _windows(draw, a, chunk, H, W), _windows(S, a, chunk, H, W)
    return dict(Vd=_bt(wd), S_Vd=_bt_mag(ws), Gy=_g4(wd), S_Gy=_g4_mag(ws))


def bwd_transforms_ref(dy, raw, pos, pscale, pshift, mean, invstd, coef, m1, m2, act, slope, chunk):
    """efgh_wino2d_bwd_transforms for one chunk.  dy, raw [B][H][W][N]; the mask: pos [B][H][W][N] bool (the unpacked sign bits) or,
    pos None, raw*pscale + pshift > 0 -> dict(Vd, S_Vd, Gy, S_Gy [tiles][36][N]; dres, S_dres [rows_of(chunk)][W][N])"""
    B, H, W, N = dy.shape
    b = chunk[0]
    a, e = _window_rows(chunk, H)
    p = BC.mask_of(bits=None if pos is None else pos[b, a:e], raw=raw[b, a:e], pscale=pscale, pshift=pshift)
    draw, S, dres, S_dres = BC.act_bn_bwd_apply(dy[b, a:e], p, raw[b, a:e], mean, invstd, coef, m1, m2, act, slope)
    out = _both(draw, S, a, chunk, H, W)
    y0, y1 = rows_of(chunk, H)
    out['dres'], out['S_dres'] = dres[y0 - a:y1 - a], S_dres[y0 - a:y1 - a]
    return out


def bwd_transforms_pooled_ref(dy_pool, raw, pscale, pshift, mean, invstd, coef, m1, m2, act, slope, chunk):
    """efgh_wino2d_bwd_transforms_pooled for one chunk.  dy_pool [B][H/2][W/2][N], raw [B][H][W][N]: draw of
    bn_contract.pool_bn_bwd_apply (the floor-pool rim included: coef*(-m1 - xhat*m2)) -> dict(Vd, S_Vd, Gy, S_Gy)"""
    B, H, W, N = raw.shape
    b = chunk[0]
    a, e = _window_rows(chunk, H)
    a2 = a & ~1                                          # whole pooling windows: from an even row ...
    e2 = e if e == H else e + (e & 1)                    # ... to an even row, or to the image's last row (the rim of an odd H)
    h2 = (e2 - a2) // 2
    draw, S = BC.pool_bn_bwd_apply(dy_pool[b:b + 1, a2 // 2:a2 // 2 + h2], raw[b:b + 1, a2:e2], mean, invstd, coef, m1, m2, pscale, pshift,
                                   act, slope)
    return _both(draw[0], S[0], a2, chunk, H, W)


# ------------------------------------------------------------------------------------------------ comparison of a launch
def check_tiles(cls, label, got, ref, S, chunk, H, W, factor=1.0, table=None):
    """got [T][36][N] of the whole launch against the reference of one chunk -> elements over the bound"""
    t0, t1 = tiles_of(chunk, H, W)
    return cmp(cls, label, got[t0:t1], ref, S, factor, table)


def check_dres(label, dres4, ref, chunk, H):
    """dres4 [B][H][W][N] view of the launch's dres against ref = bwd_transforms_ref(chunk): a copy where the derivative is 1 or 0"""
    y0, y1 = rows_of(chunk, H)
    got = dres4[chunk[0], y0:y1]
    copy = ref['S_dres'] == 0
    return BC.cmp('exact', label, got[copy], ref['dres'][copy], None) + BC.cmp('elem', label + ' dres', got, ref['dres'], ref['S_dres'])


# ------------------------------------------------------------------------------------------------ the cases of the GPU module
ACTS = BC.ACTS
# (B, H, W): single partial tiles; exact multiples of 4; a last tile one pixel wide (W = 5, 9, 13); B > 1 (rowt / TH splits batches);
# at N = 64 a workgroup holds four tiles, so TW = 1, 2, 3 cut inside a workgroup (TW * N no multiple of 256)
GEOMS = [(1, 1, 1), (1, 2, 2), (3, 3, 5), (1, 4, 4), (2, 5, 9), (1, 6, 7), (2, 8, 12), (1, 4, 13)]
POOL_GEOMS = [g for g in GEOMS if g[1] >= 2 and g[2] >= 2]      # (2,2): Ho = Wo = 1; odd H; odd W; both odd
POOL_TIES = (2, 8, 12)                                          # H >= 2, W >= 8: carries bn_contract.plant_ties
FUSED_N = [64, 128, 512]      # 64: four tiles per workgroup; 512: two workgroups per tile, mask word index (c & ~63) >> 5 up to 14
PLAIN_C = [4, 64, 512]        # channel pairs: 2 (128 tiles per workgroup), 32, 256 (one tile per workgroup)
NONFINITE_GEOM = (2, 5, 9)
# either side of the non-temporal switch at N = 64: T = 43 690 is 6 KiB below 384 MiB, T = 43 692 above
NT_BELOW, NT_ABOVE, NT_N = (1, 680, 1028), (1, 528, 1324), 64
assert geo(*NT_BELOW)[2] == 43690 and BC.NT_BYTES - nt_bytes(*NT_BELOW, NT_N) == 6144
assert geo(*NT_ABOVE)[2] == 43692 and nt_bytes(*NT_ABOVE, NT_N) >= BC.NT_BYTES
NT_ACT = (BC.ACT_LEAKY, 0.2)


def case_seed(geom, N, a, slope):
    return BC.case_seed((*geom, N), a, slope)


def gen_plain(geom, N, a, slope, device):
    """inputs of efgh_wino2d_bwd_transforms: bn_contract.gen_rows over the B*H*W pixels (raw settled against scale / shift) + mask
    bits drawn independently of raw + the means m1 / m2 (any: the apply stage takes them as inputs)"""
    B, H, W = geom
    seed = case_seed(geom, N, a, slope)
    c = BC.gen_rows(B * H * W, N, seed, device, a, slope)
    g = torch.Generator(device=device).manual_seed(seed + 5)
    c['pos'] = torch.rand((B * H * W, N), generator=g, device=device) < 0.5
    c['m1'] = (0.05 * torch.randn(N, generator=g, device=device)).double()
    c['m2'] = (0.05 * torch.randn(N, generator=g, device=device)).double()
    return c


def gen_pooled(geom, N, a, slope, device, ties=False):
    """inputs of efgh_wino2d_bwd_transforms_pooled: bn_contract.gen_pool (+ plant_ties) + the means"""
    B, H, W = geom
    seed = case_seed(geom, N, a, slope)
    c = BC.gen_pool(B, H, W, N, seed, device, a, slope, ties=ties)
    g = torch.Generator(device=device).manual_seed(seed + 5)
    c['m1'] = (0.05 * torch.randn(N, generator=g, device=device)).double()
    c['m2'] = (0.05 * torch.randn(N, generator=g, device=device)).double()
    return c
