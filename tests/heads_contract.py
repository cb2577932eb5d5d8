"""float64 reference of G's head chain and of the layout converters (test helper): the fold of the one-GEMM transposed convolution and
its adjoint unfold, the two 2-way softmax kernels with their backward passes, and the planar <-> channels-last converters - the eight
entry points of include/efgh_hip.h listed in ENTRY_POINTS, written from the header and from gnet.py:56-68 / :121-124 of the reference
(`ConvTranspose2d(k 3, s 2)`, `nn.Softmax(dim=1)`), independent of the kernel bodies.

Every function takes the flat fp32 buffer a kernel gets (any device) with the offset of the first element and the pitch, computes in
float64 and returns the result with the scale S of its error bound.  Error model, element by element, U = 2^-24:

    |got - ref| <= CEIL[cls] * S + FLOOR[cls]          a NaN matches a NaN, an inf the same inf, any other non-finite mismatch fails

  copy          im2col, the two layout converters, the depth channel of the heads and every element that must be +0.0: CEIL 0, compared
                as int32 bit patterns (-0.0, NaN payloads and denormals survive).
  col2im        out = act(scale * sum + shift), S = (sum |Y term|) |scale| + |shift|.  oh = 2 ih - pad + kh has one solution ih per kh
                of the right parity, so at most 2 x 2 of the 9 taps land on one output pixel: 3 additions (3 roundings, each relative to
                a partial sum <= sum |Y|), scale and shift 2 more (1 if contracted to an FMA), the activation is 1-Lipschitz and the
                leaky slope one last product: 6 roundings in a chain, gamma_6 = 6 U / (1 - 6 U).  slope is the fp32 number the kernel is
                handed.
  softmax_bwd   dx_k = y_k (g_k - (g_0 y_0 + g_1 y_1)), S_k = |y_k| (|g_k| + |g_0 y_0| + |g_1 y_1|).  Five operations; the two products
                of the dot are side by side, so a term passes four roundings (product, add, subtract, product) and g_k two:
                gamma_4 = 4 U / (1 - 4 U).  Held as a formula in y: y need not be a softmax.
  softmax       y = softmax(a, c), S = y (1 + |a - c|): the rounding of a - m enters the exponent, so the relative error of the small
                component grows with |a - c|.  The device expf has no stated bound, so the constant is not derived: the yardstick is
                the fp32 CPU evaluation of the reference (torch.softmax in fp32 and exp(a-m) / (exp(a-m) + exp(c-m)) in fp32 torch, the
                larger error) pooled over every softmax case of this module, in units of S U; the constant is at most 4 x that figure
                (the margin of gemm_contract.TAU and pose_contract.CEIL).  FLOOR 2^-126: results in the subnormal range are not pinned.

OBSERVED records the largest (|got - ref| - FLOOR) / (S U) per class, to be read against CEIL / U."""
import functools

import numpy as np
import torch

from bn_contract import outside_unchanged, view2      # noqa: F401  (re-exported for the test modules)
from gemm_contract import DELTA, flat                 # noqa: F401

ENTRY_POINTS = ['efgh_convt_col2im', 'efgh_convt_im2col', 'efgh_heads_to_nchw', 'efgh_softmax2_to_nchw', 'efgh_heads_bwd',
                'efgh_softmax2_bwd', 'efgh_nchw_to_nhwc', 'efgh_nhwc_to_nchw']
U = 2.0 ** -24
SOFTMAX_YARDSTICK = 1.863    # fp32 CPU evaluation of the reference, largest error / (S U) over softmax_cases() (torch.softmax; three-line formula 1.553)
CEIL = {
    'copy': 0.0,
    'col2im': 6 * U / (1 - 6 * U),            # derived above; kernel (MI355X) 2.36 U (2x2x129, O 3, pad 1, opad 1, ldy 28, affine, act 0)
    'softmax_bwd': 4 * U / (1 - 4 * U),       # derived above; kernel (MI355X) 3.70 U (efgh_heads_bwd, 2 x 2097281 pixels, gradients 1e-20 .. 1e20)
    'softmax': 5.6 * U,                       # 3 x the yardstick 1.863 U, the margin of pose_contract.CEIL (<= 4 x); kernel (MI355X) 2.01 U (efgh_heads_to_nchw, 2 x 2097281 pixels)
}
FLOOR = {'copy': 0.0, 'col2im': DELTA, 'softmax_bwd': DELTA, 'softmax': 2.0 ** -126}
OBSERVED = {}                # class -> (largest (|got - ref| - FLOOR) / (S U), the case that produced it): filled by cmp()
SLOPE = float(np.float32(0.2))
POISON = 1e30                # padding of the inputs: shows in any result that reads it

MUTATIONS = ['tap_parity', 'pad_sign', 'last_col_dropped', 'opad_ignored', 'channels_swapped', 'no_max_subtract', 'bwd_without_dot',
             'depth_into_ch1', 'pad_channel_copied', 'plane_stride_Cd']


def ceil4(n):
    return (n + 3) // 4 * 4


def bits(t):
    return t.contiguous().view(torch.int32)


def cmp(cls, label, got, ref, S=None):
    """-> number of elements of the fp32 `got` outside CEIL[cls] * S + FLOOR[cls] of `ref`; class 'copy': differing bit patterns
    (ref fp32).  Records the largest (|got - ref| - FLOOR) / (S U) of the class in OBSERVED."""
    assert got.dtype == torch.float32 and got.shape == ref.shape, (label, got.dtype, tuple(got.shape), tuple(ref.shape))
    if CEIL[cls] == 0.0:
        assert ref.dtype == torch.float32
        bad = int((bits(got) != bits(ref)).sum())
        if bad > OBSERVED.get(cls, (-1, ''))[0]:
            OBSERVED[cls] = (bad, label)           # (differing elements, not a ratio)
        return bad
    g, r = got.double(), ref.double()
    same = (torch.isnan(g) & torch.isnan(r)) | (torch.isinf(g) & (g == r))
    fin = torch.isfinite(g) & torch.isfinite(r)
    inf = torch.full_like(g, float('inf'))
    err = torch.where(fin, (g - r).abs(), inf)
    err = torch.where(same, torch.zeros_like(g), err)
    Sx = torch.where(torch.isfinite(S), S.double().abs(), torch.zeros_like(g))
    over = (err - FLOOR[cls]).clamp_min(0)
    ratio = float((over / (Sx * U + 1e-300)).max()) if err.numel() else 0.0
    ratio = min(ratio, 1e300)
    if ratio > OBSERVED.get(cls, (-1.0, ''))[0]:
        OBSERVED[cls] = (ratio, label)
    return int((err > CEIL[cls] * Sx + FLOOR[cls]).sum())


def _act(v, act, slope):
    if act == 1:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == 2:
        return torch.where(v > 0, v, v * slope)
    return v


# ------------------------------------------------------------------------------------------------ transposed-conv fold / unfold
def _tap_pairs(n_in, n_out, pad, k, mut, last_dropped=False):
    """input index i and output index o = 2 i - pad + k of tap k along one axis, where o is inside the output"""
    i = torch.arange(n_in - 1 if (last_dropped and n_in > 1) else n_in)
    o = 2 * i + (pad if mut == 'pad_sign' else -pad) + k + (1 if mut == 'tap_parity' else 0)
    opad = n_out - ((n_in - 1) * 2 - 2 * pad + 3)
    ok = (o >= 0) & (o < (n_out - 1 if (mut == 'opad_ignored' and opad > 0) else n_out))
    return i[ok], o[ok]


def col2im(Y, ldy, B, Hin, Win, Ho, Wo, O, pad, scale, shift, act, slope, off=0, mut=None, dt=torch.float64):
    """efgh_convt_col2im: Y flat, rows [B*Hin*Win] of pitch ldy from `off`, column (kh*3+kw)*O+o; scale / shift [>= O] or None
    -> (ref float64 [B][Ho][Wo][4], channels >= O zero; S).  A scatter over the input pixels, oh = 2 ih - pad + kh.
    dt torch.float32: the same formula evaluated in fp32 (the host test holds the derived ceiling to it)"""
    y = view2(Y, off, ldy, B * Hin * Win, 9 * O).to(dt).reshape(B, Hin, Win, 9, O)
    dev = y.device
    ref = torch.zeros((B, Ho, Wo, 4), dtype=dt, device=dev)
    S = torch.zeros_like(ref)
    for kh in range(3):
        ih, oh = (t.to(dev) for t in _tap_pairs(Hin, Ho, pad, kh, mut))
        for kw in range(3):
            iw, ow = (t.to(dev) for t in _tap_pairs(Win, Wo, pad, kw, mut, mut == 'last_col_dropped'))
            if ih.numel() == 0 or iw.numel() == 0:
                continue
            t = y[:, ih[:, None], iw[None, :], kh * 3 + kw, :]
            ref[:, oh[:, None], ow[None, :], :O] += t
            S[:, oh[:, None], ow[None, :], :O] += t.abs()
    sc = torch.ones(O, dtype=dt, device=dev) if scale is None else scale[:O].to(dt).to(dev)
    sh = torch.zeros(O, dtype=dt, device=dev) if shift is None else shift[:O].to(dt).to(dev)
    ref[..., :O] = _act(ref[..., :O] * sc + sh, act, slope)
    S[..., :O] = S[..., :O] * sc.abs() + sh.abs()
    return ref, S


def im2col(G, ldg, B, Hin, Win, Ho, Wo, O, pad, ldy, off=0, mut=None):
    """efgh_convt_im2col: G flat, pixels [B*Ho*Wo] of pitch ldg from `off` -> fp32 [B*Hin*Win][ldy]: column (kh*3+kw)*O+o of input
    pixel (ih, iw) = G[b][2 ih - pad + kh][2 iw - pad + kw][o] (zero outside the output), columns 9*O .. ldy-1 zero.  Exact"""
    g = view2(G, off, ldg, B * Ho * Wo, O).reshape(B, Ho, Wo, O)
    out = torch.zeros((B, Hin, Win, ldy), dtype=torch.float32, device=g.device)
    for kh in range(3):
        ih, oh = (t.to(g.device) for t in _tap_pairs(Hin, Ho, pad, kh, mut))
        for kw in range(3):
            iw, ow = (t.to(g.device) for t in _tap_pairs(Win, Wo, pad, kw, mut, mut == 'last_col_dropped'))
            if ih.numel() == 0 or iw.numel() == 0:
                continue
            t = kh * 3 + kw
            out[:, ih[:, None], iw[None, :], t * O:(t + 1) * O] = g[:, oh[:, None], ow[None, :], :]
    return out.reshape(B * Hin * Win, ldy)


# ------------------------------------------------------------------------------------------------ softmax over two channels
def softmax2(a, c, mut=None):
    """-> (y0, y1, S0, S1) float64: nn.Softmax over the pair (a, c), S = y (1 + |a - c|)"""
    a, c = a.double(), c.double()
    m = torch.zeros_like(a) if mut == 'no_max_subtract' else torch.maximum(a, c)
    ea, ec = torch.exp(a - m), torch.exp(c - m)
    y0, y1 = ea / (ea + ec), ec / (ea + ec)
    w = 1 + (a - c).abs()
    return y0, y1, y0 * w, y1 * w


def softmax2_bwd(y0, y1, g0, g1, mut=None, dt=torch.float64):
    """-> (dx0, dx1, S0, S1) float64: dx_k = y_k (g_k - (g_0 y_0 + g_1 y_1)); a formula in y, which need not be a softmax"""
    y0, y1, g0, g1 = y0.to(dt), y1.to(dt), g0.to(dt), g1.to(dt)
    dot = torch.zeros_like(y0) if mut == 'bwd_without_dot' else g0 * y0 + g1 * y1
    A = (g0 * y0).abs() + (g1 * y1).abs()
    return y0 * (g0 - dot), y1 * (g1 - dot), y0.abs() * (g0.abs() + A), y1.abs() * (g1.abs() + A)


def softmax2_to_nchw(x, ld, B, HW, off=0, mut=None):
    """efgh_softmax2_to_nchw: x flat, rows [B*HW] of pitch ld from `off`, the first two channels -> (ref [B][2][HW], S)"""
    v = view2(x, off, ld, B * HW, 2).reshape(B, HW, 2)
    k0, k1 = (1, 0) if mut == 'channels_swapped' else (0, 1)
    y0, y1, S0, S1 = softmax2(v[..., k0], v[..., k1], mut)
    return torch.stack([y0, y1], 1), torch.stack([S0, S1], 1)


def softmax2_to_nchw_bwd(y, dy, B, HW, ld, mut=None):
    """efgh_softmax2_bwd: y, dy planar [B][2][HW] -> (ref [B*HW][ld] with channels >= 2 zero, S)"""
    y, dy = y.reshape(B, 2, HW), dy.reshape(B, 2, HW)
    d0, d1, S0, S1 = softmax2_bwd(y[:, 0], y[:, 1], dy[:, 0], dy[:, 1], mut)
    ref = torch.zeros((B, HW, ld), dtype=torch.float64, device=y.device)
    S = torch.zeros_like(ref)
    ref[..., 0], ref[..., 1], S[..., 0], S[..., 1] = d0, d1, S0, S1
    return ref.reshape(B * HW, ld), S.reshape(B * HW, ld)


def heads_fwd(x, B, HW, off=0, mut=None):
    """efgh_heads_to_nchw: x flat [B*HW][4] from `off`: channel 0 depth, channels 1-2 mask logits
    -> (depth fp32 [B*HW], a copy; mask ref [B][2][HW], S)"""
    v = view2(x, off, 4, B * HW, 4)
    depth = v[:, 1 if mut == 'depth_into_ch1' else 0].clone()
    k0, k1 = (2, 1) if mut == 'channels_swapped' else (1, 2)
    y0, y1, S0, S1 = softmax2(v[:, k0].reshape(B, HW), v[:, k1].reshape(B, HW), mut)
    return depth, torch.stack([y0, y1], 1), torch.stack([S0, S1], 1)


def heads_bwd(y, dmask, ddepth, B, HW, mut=None):
    """efgh_heads_bwd: y planar [B][2][HW]; dmask [B][2][HW] or None; ddepth [B*HW] or None
    -> (ref float64 [B*HW][4], S): channel 0 a copy of ddepth (S 0), channels 1-2 the softmax backward, channel 3 +0.0; an absent
    gradient gives zeros"""
    ref = torch.zeros((B * HW, 4), dtype=torch.float64, device=y.device)
    S = torch.zeros_like(ref)
    if dmask is not None:
        r, s = softmax2_to_nchw_bwd(y, dmask, B, HW, 2, mut)
        k0, k1 = (2, 1) if mut == 'channels_swapped' else (1, 2)
        ref[:, k0], ref[:, k1], S[:, k0], S[:, k1] = r[:, 0], r[:, 1], s[:, 0], s[:, 1]
    if ddepth is not None:
        if mut == 'depth_into_ch1':
            ref[:, 1] += ddepth.reshape(-1).double()
        else:
            ref[:, 0] = ddepth.reshape(-1).double()
    return ref, S


# ------------------------------------------------------------------------------------------------ layout
def nchw_to_nhwc(x, B, Cs, HW, Cd, off=0, mut=None):
    """efgh_nchw_to_nhwc: x flat planar [B][Cs][HW] from `off` -> fp32 [B*HW][Cd], channels >= Cs +0.0.  Exact"""
    f = flat(x)[off:]
    stride = Cd if mut == 'plane_stride_Cd' else Cs
    b = torch.arange(B, device=f.device)[:, None, None]
    p = torch.arange(HW, device=f.device)[None, :, None]
    c = torch.arange(Cd, device=f.device)[None, None, :]
    src = (b * stride + c.clamp_max(Cs - 1)) * HW + p
    assert mut == 'plane_stride_Cd' or int(src.max()) < B * Cs * HW
    v = f[src % f.numel()]
    if mut != 'pad_channel_copied':
        v = torch.where(c < Cs, v, torch.zeros_like(v))
    return v.reshape(B * HW, Cd)


def nhwc_to_nchw(x, ld, B, Cs, HW, off=0, mut=None):
    """efgh_nhwc_to_nchw: x flat, rows [B*HW] of pitch ld from `off`, the first Cs channels -> fp32 [B][Cs][HW].  Exact"""
    return view2(x, off, ld, B * HW, Cs).reshape(B, HW, Cs).permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------------------------------------ the cases both test modules run
GEOMS = [(1, 1, 1), (1, 1, 5), (1, 5, 1), (3, 3, 4), (2, 2, 128), (2, 2, 129)]       # (B, Hin, Win): Wo 255 .. 259 around one block
PAD_OPAD = [(0, 0), (1, 0), (1, 1)]
NAN_GEOM = (3, 3, 4)          # the col2im cases of this geometry with act 0 / 2 carry a NaN and a -0.0 in Y


def out_size(n, pad, opad):
    return (n - 1) * 2 - 2 * pad + 3 + opad


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


@functools.lru_cache(maxsize=None)
def col2im_cases():
    """-> tuple of (B, Hin, Win, O, pad, opad, ldy, ldo, affine, act): every geometry x O x (pad, opad) x every ldy, with ldo, the
    affine and the activation dealt round-robin so that each value meets each ldy, O and geometry"""
    out, n = [], 0
    for gi, (B, Hin, Win) in enumerate(GEOMS):
        for O in (1, 2, 3, 4):
            for pi, (pad, opad) in enumerate(PAD_OPAD):
                for ldy in sorted({9 * O, ceil4(9 * O), ceil4(9 * O) + 4}):
                    out.append((B, Hin, Win, O, pad, opad, ldy, (4, 8)[n % 2], (n // 3) % 2, (n + gi) % 3))
                    n += 1
    return tuple(out)


COL2IM_OFF = 3                # first element of Y in its buffer (Y need not be aligned)


@functools.lru_cache(maxsize=None)
def gen_col2im(case):
    """-> (Y buffer: rows at COL2IM_OFF, pitch ldy, pad columns and the rows around them POISON; scale, shift fp32 [4] or None)"""
    B, Hin, Win, O, pad, opad, ldy, ldo, affine, act = case
    g = _gen(hash(case) % (1 << 31))
    M = B * Hin * Win
    buf = torch.full((COL2IM_OFF + (M + 2) * ldy,), POISON, dtype=torch.float32)
    y = torch.randn((M, 9 * O), generator=g)
    if (B, Hin, Win) == NAN_GEOM and act != 1:
        y[M // 2, (4 * O) % (9 * O)] = float('nan')
        y[M // 3, 0] = -0.0
    view2(buf, COL2IM_OFF, ldy, M, 9 * O).copy_(y)
    if not affine:
        return buf, None, None
    scale = torch.tensor([1.5, -0.75, 0.3, 2.0]) + 0.1 * torch.randn(4, generator=g)
    shift = torch.tensor([0.2, -0.4, 0.0, 1.0]) + 0.1 * torch.randn(4, generator=g)
    scale[O:], shift[O:] = POISON, POISON
    return buf, scale, shift


@functools.lru_cache(maxsize=None)
def ref_col2im(case):
    B, Hin, Win, O, pad, opad, ldy, ldo, affine, act = case
    buf, scale, shift = gen_col2im(case)
    return col2im(buf, ldy, B, Hin, Win, out_size(Hin, pad, opad), out_size(Win, pad, opad), O, pad, scale, shift, act, SLOPE,
                  COL2IM_OFF)


@functools.lru_cache(maxsize=None)
def im2col_cases():
    """-> tuple of (B, Hin, Win, O, pad, opad, ldg): the shapes of the unfold; the pitches ldy and the routes are the GPU module's"""
    return tuple((B, Hin, Win, O, pad, opad, (4, 8)[(gi + O + pi) % 2]) for gi, (B, Hin, Win) in enumerate(GEOMS) for O in (1, 2, 3, 4)
                 for pi, (pad, opad) in enumerate(PAD_OPAD))


def vec_ldys(O):
    return [v for v in (12, 20, 28, 36, 40) if v >= 9 * O]


@functools.lru_cache(maxsize=None)
def gen_im2col(case, ldg=None):
    """-> (G buffer: [B*Ho*Wo] pixels of pitch ldg from element `off` = two poison rows in, every other element POISON - the channels
    >= O of every pixel too; off)"""
    B, Hin, Win, O, pad, opad, ldg0 = case
    ldg = ldg or ldg0
    Ho, Wo = out_size(Hin, pad, opad), out_size(Win, pad, opad)
    off = 2 * Wo * ldg // 4 * 4 + 4
    buf = torch.full((off + (B * Ho * Wo + 2 * Wo + 2) * ldg,), POISON, dtype=torch.float32)
    view2(buf, off, ldg, B * Ho * Wo, min(O, ldg)).copy_(torch.randn((B * Ho * Wo, min(O, ldg)), generator=_gen(hash(case) % (1 << 31))))
    return buf, off


def _softmax_pairs():
    f = np.float32
    inf, nan = f(np.inf), f(np.nan)
    big = f(1e30)
    rows = [(0.5, 0.5), (-3.25, -3.25), (3e38, -3e38), (big, np.nextafter(big, inf)), (-0.0, 0.0), (-inf, 0.0), (inf, 0.0), (-inf, -inf),
            (nan, 0.0), (nan, nan), (-inf, 2.5), (88.5, 1.25)]
    for d in (1e-3, 10.0, 87.0, 104.0):
        rows += [(d, 0.0), (-d, 0.0), (1.75 + d, 1.75), (-0.3 - d, -0.3)]
    rows += [(c, a) for a, c in rows]
    return torch.tensor(np.array(rows, dtype=np.float32))


SOFTMAX_PAIRS = _softmax_pairs()
SOFTMAX_SIZES = [(1, 1), (2, 255), (1, 256), (3, 257)]
SOFTMAX_BIG = (2, 2097152 + 129)          # past the 16384-block grid cap: the second trip of the grid-stride loop


def logits(n, rot, device='cpu', seed=0):
    """[n][2] logit pairs: the special pairs of SOFTMAX_PAIRS (from `rot` on) at the even pixels, 3 randn beside them at the odd ones"""
    i = torch.arange(n, device=device)
    sp = SOFTMAX_PAIRS.to(device)[((i // 2) + rot) % SOFTMAX_PAIRS.shape[0]]
    g = torch.Generator(device=device)
    g.manual_seed(1000 + seed)
    rn = 3 * torch.randn((n, 2), generator=g, device=device)
    return torch.where((i % 2 == 0)[:, None], sp, rn)


@functools.lru_cache(maxsize=None)
def softmax_cases():
    """-> tuple of (B, HW, rot): every special pair alone in a 1 x 1 image, and the larger images at three rotations"""
    return tuple([(1, 1, r) for r in range(SOFTMAX_PAIRS.shape[0])] + [(B, HW, r) for B, HW in SOFTMAX_SIZES[1:] for r in (0, 7, 23)])


@functools.lru_cache(maxsize=None)
def gen_logits(case):
    B, HW, rot = case
    return logits(B * HW, rot, seed=rot)


def mixed_grads(shape, seed, device='cpu'):
    """gradients of mixed magnitude, 1e-20 .. 1e20, beside plain randn"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    r = torch.randn(shape, generator=g, device=device)
    e = torch.randint(-20, 21, shape, generator=g, device=device).float()
    plain = torch.rand(shape, generator=g, device=device) < 0.5
    return torch.where(plain, r, r * 10.0 ** e)


@functools.lru_cache(maxsize=None)
def bwd_cases():
    """-> tuple of (B, HW, y_kind): y_kind 'fwd' (the fp32 softmax of the logits of rotation 0, NaN rows included) or 'any' (in [0, 1])"""
    return tuple((B, HW, k) for B, HW in SOFTMAX_SIZES for k in ('fwd', 'any'))


@functools.lru_cache(maxsize=None)
def gen_bwd(case):
    """-> (y [B][2][HW], dmask [B][2][HW], ddepth [B*HW]) fp32"""
    B, HW, kind = case
    if kind == 'fwd':
        lg = gen_logits((B, HW, 0)) if HW > 1 else torch.tensor([[0.3, -1.2]])
        y = torch.softmax(lg.reshape(B, HW, 2).double(), 2).float().permute(0, 2, 1).contiguous()
    else:
        y = torch.rand((B, 2, HW), generator=_gen(B * 131 + HW))
    dd = mixed_grads((B * HW,), B * 17 + HW + 1)
    if HW > 4:
        dd[0], dd[1], dd[2] = -0.0, float('nan'), 1e-42
    return y, mixed_grads((B, 2, HW), B * 17 + HW), dd


LAYOUT_CASES = [(1, 1, 1, 1), (2, 3, 5, 4), (1, 3, 257, 4), (3, 1, 7, 4), (2, 5, 33, 8), (2, 16, 9, 16)]       # (B, Cs, HW, Cd)
LAYOUT_BIG = (1, 4, 4194304 + 3, 4)       # past the grid cap of both converters
LAYOUT_OFF = 5


def special_floats(n, seed, device='cpu'):
    """fp32 [n] as int32 bit patterns drawn over the whole range: NaN payloads, infinities, -0.0 and denormals among them"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    b = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, device=device, dtype=torch.int64).to(torch.int32)
    fixed = torch.tensor([-2 ** 31, 0x7fc00001, -4194303, 1, 0x007fffff, 0x7f800000, -8388608, 0x7f800001], dtype=torch.int32, device=device)
    k = min(n, fixed.numel())
    b[:k] = fixed[:k]
    return b.view(torch.float32)


@functools.lru_cache(maxsize=None)
def gen_planar(case):
    """-> planar buffer: [B][Cs][HW] at LAYOUT_OFF inside POISON"""
    B, Cs, HW, Cd = case
    buf = torch.full((LAYOUT_OFF + B * Cs * HW + 7,), POISON, dtype=torch.float32)
    buf[LAYOUT_OFF:LAYOUT_OFF + B * Cs * HW] = special_floats(B * Cs * HW, B * 1000 + Cs * 10 + HW)
    return buf


def nhwc_lds(Cs):
    return sorted({ld for ld in (Cs, Cs + 1, 8) if ld >= Cs})


@functools.lru_cache(maxsize=None)
def gen_rows(B, Cs, HW, ld):
    """-> channels-last buffer: rows [B*HW] of pitch ld at LAYOUT_OFF, channels >= Cs and everything around POISON"""
    buf = torch.full((LAYOUT_OFF + (B * HW + 1) * ld,), POISON, dtype=torch.float32)
    view2(buf, LAYOUT_OFF, ld, B * HW, Cs).copy_(special_floats(B * HW * Cs, B * 77 + Cs + HW + ld).reshape(B * HW, Cs))
    return buf


NHWC_EXTRA = [(2, 1, 33, 4), (2, 2, 33, 4)]       # (B, Cs, HW, ld): the product's use, one and two channels of a 4-channel map


# ------------------------------------------------------------------------------------------------ the float32 yardsticks
def softmax_yardstick():
    """-> (units of S U of torch.softmax in fp32, of the three-line formula in fp32 torch) over softmax_cases(), against softmax2"""
    worst = [0.0, 0.0]
    for case in softmax_cases():
        lg = gen_logits(case)
        a, c = lg[:, 0], lg[:, 1]
        y0, y1, S0, S1 = softmax2(a, c)
        m = torch.maximum(a, c)
        ea, ec = torch.exp(a - m), torch.exp(c - m)
        three = torch.stack([ea / (ea + ec), ec / (ea + ec)], 1)
        for k, got in enumerate((torch.softmax(lg, 1), three)):
            for j, (r, S) in enumerate(((y0, S0), (y1, S1))):
                fin = torch.isfinite(r) & torch.isfinite(S) & (S > 0)
                over = ((got[:, j].double() - r).abs() - FLOOR['softmax']).clamp_min(0)
                if bool(fin.any()):
                    worst[k] = max(worst[k], float((over[fin] / (S[fin] * U)).max()))
    return tuple(worst)


# ------------------------------------------------------------------------------------------------ the chain, end to end
# One transposed head layer (ConvTranspose2d 128 -> O, k 3, s 2, pad 1, output_padding 1, + BatchNorm2d + LeakyReLU(0.2): the small form
# of layers.conv_transpose2d) and G's two head stacks with their softmax (gnet.py:56-68, :121-124), as plain nn modules.  The reference
# is the float64 CPU run of a deep copy of the modules; the error is pose_contract.rel_err per tensor; a family's ceiling is 3 x the
# largest error of the fp32 CPU run of the same modules against that float64 run (at most 4 x: tests/test_heads_contract_host.py
# recomputes the figure and holds the constant inside 1 x .. 4 x of it).
CHAIN_B, CHAIN_C = 2, 128
CHAIN_SHAPES = [(1, 1), (3, 129), (5, 7)]
CHAIN_MODES = ['eval', 'train', 'tape']            # eval-mode BatchNorm; batch statistics without autograd; batch statistics on the tape
# fp32 CPU yardstick: value 9.57e-07 (heads 5x7 eval depth), input gradient 2.50e-07 (layer O 3 3x129 tape dx), parameter gradient
# 4.4e-06 .. 7.6e-06 with the thread count of the CPU run (heads 3x129 train, d.1.bias / d.4.weight: BatchNorm sums that cancel)
CHAIN_YARDSTICK = {'value': 9.57e-7, 'input_grad': 2.50e-7, 'param_grad': 5.0e-6}
# kernels (MI355X): value 1.11e-06 (fused heads 1x1 train, depth), input gradient 3.11e-07 (layer O 3 3x129 on the tape), parameter
# gradient 3.80e-06 (fused heads 1x1 train, d.4.weight)
CHAIN_CEIL = {k: 3 * v for k, v in CHAIN_YARDSTICK.items()}


def _randomize_bn(mods, g):
    import torch.nn as nn
    for m in mods:
        if isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=g))


@functools.lru_cache(maxsize=None)
def chain_layer_case(O, H, W):
    """-> (ConvTranspose2d, BatchNorm2d, x (B,128,H,W), gy (B,O,2H,2W)) fp32 on the CPU; deep-copy the modules before use"""
    import torch.nn as nn
    g = _gen(O * 10000 + H * 100 + W)
    ct, bn = nn.ConvTranspose2d(CHAIN_C, O, 3, 2, 1, 1, bias=False), nn.BatchNorm2d(O)
    with torch.no_grad():
        ct.weight.copy_(0.1 * torch.randn(ct.weight.shape, generator=g))
    _randomize_bn([bn], g)
    return ct, bn, torch.randn((CHAIN_B, CHAIN_C, H, W), generator=g), torch.randn((CHAIN_B, O, 2 * H, 2 * W), generator=g)


def chain_layer_run(O, H, W, mode, dtype):
    """the layer as nn modules on the CPU in `dtype` -> dict family -> {name: tensor}"""
    import copy
    import torch.nn.functional as F
    ct, bn, x, gy = chain_layer_case(O, H, W)
    ct, bn = copy.deepcopy(ct).to(dtype), copy.deepcopy(bn).to(dtype)
    bn.train(mode != 'eval')
    x = x.clone().to(dtype).requires_grad_(mode == 'tape')
    with torch.set_grad_enabled(mode == 'tape'):
        y = F.leaky_relu(bn(ct(x)), 0.2)
    out = {'value': {'y': y.detach(), 'running_mean': bn.running_mean.clone(), 'running_var': bn.running_var.clone()}}
    if mode == 'tape':
        y.backward(gy.to(dtype))
        out['input_grad'] = {'dx': x.grad}
        out['param_grad'] = {'ct.weight': ct.weight.grad, 'bn.weight': bn.weight.grad, 'bn.bias': bn.bias.grad}
    return out


@functools.lru_cache(maxsize=None)
def chain_heads_case(H, W):
    """-> (depth stack, mask stack (builders.convt_bn_relu), x (B,128,H,W), gd (B,1,2H,2W), gm (B,2,2H,2W)) fp32 on the CPU"""
    from efgh_amd.nets.builders import convt_bn_relu
    g = _gen(77 + H * 100 + W)
    torch.manual_seed(77 + H * 100 + W)
    sd, sm = convt_bn_relu(CHAIN_C, 1, 3, 2, 1, 1), convt_bn_relu(CHAIN_C, 2, 3, 2, 1, 1)
    _randomize_bn(list(sd.modules()) + list(sm.modules()), g)
    shape = (CHAIN_B, CHAIN_C, H, W)
    return (sd, sm, torch.randn(shape, generator=g), torch.randn((CHAIN_B, 1, 2 * H, 2 * W), generator=g),
            torch.randn((CHAIN_B, 2, 2 * H, 2 * W), generator=g))


def chain_heads_run(H, W, train, dtype):
    """g_depth = convt_dimg(x), g_mask = softmax(convt_mask(x)) as nn modules on the CPU in `dtype` -> dict family -> {name: tensor}"""
    import copy
    sd, sm, x, gd, gm = chain_heads_case(H, W)
    sd, sm = copy.deepcopy(sd).to(dtype).train(train), copy.deepcopy(sm).to(dtype).train(train)
    x = x.clone().to(dtype).requires_grad_(train)
    with torch.set_grad_enabled(train):
        d, m = sd(x), torch.softmax(sm(x), 1)
    out = {'value': {'depth': d.detach(), 'mask': m.detach()}}
    for tag, seq in (('d.', sd), ('m.', sm)):
        for n, b in seq.named_buffers():
            if b.dtype == dtype:
                out['value'][tag + n] = b.clone()
    if train:
        ((d * gd.to(dtype)).sum() + (m * gm.to(dtype)).sum()).backward()
        out['input_grad'] = {'dx': x.grad}
        out['param_grad'] = {tag + n: p.grad for tag, seq in (('d.', sd), ('m.', sm)) for n, p in seq.named_parameters()}
    return out


def chain_yardstick():
    """-> dict family -> (largest rel_err of the fp32 CPU run against the float64 CPU run, the tensor that set it)"""
    from pose_contract import rel_err
    worst = {}

    def fold(label, a, b):
        for fam in b:
            for n in b[fam]:
                e = rel_err(a[fam][n], b[fam][n])
                if e > worst.get(fam, (-1.0, ''))[0]:
                    worst[fam] = (e, '%s %s' % (label, n))
    for H, W in CHAIN_SHAPES:
        for O in (1, 2, 3):
            for mode in CHAIN_MODES:
                fold('layer O %d %dx%d %s' % (O, H, W, mode), chain_layer_run(O, H, W, mode, torch.float32),
                     chain_layer_run(O, H, W, mode, torch.float64))
        for train in (False, True):
            fold('heads %dx%d %s' % (H, W, 'train' if train else 'eval'), chain_heads_run(H, W, train, torch.float32),
                 chain_heads_run(H, W, train, torch.float64))
    return worst
