"""Float64 restatement of the slice step of the BCL and of the whole BilateralConvFlex layer (test helper, in the style of
bn_contract.py): what include/efgh_hip.h promises for efgh_slice / efgh_slice_bwd / efgh_offsets_invert, and nets/bilateralNN.py
for the layer, written from those texts - not from the kernel bodies.

    slice        out[p][c]   = sum_{r<4} bary[p][r] * feat[off[p][r]][c] (+ bias[c])
    inversion    list        = the flat positions f = 4p + r ordered by (off[f], f): numpy's STABLE argsort of off.ravel();
                 vseg[h]     = (start, length) of vertex h in it; entries outside [0, H) are left out and counted
    slice bwd    gfeat[h][c] = sum over the list of h of bary[f] * gout[f >> 2][c];    gbias[c] = sum_p gout[p][c]
    layer        splat (index_add of bary * feature, / (sum bary + 1e-5) with use_norm) -> [zero row appended, rows gathered through
                 the neighbour table, Conv2d (F,1)] -> ReLU -> (1,1) convolutions ... -> last activation -> slice + bias

Error bounds, element by element, U = 2^-24 (float32 unit roundoff), every one with the additive DELTA of gemm_contract.py:
    slice           8 U (sum_r |b_r||f_r| + |bias|)       four products, three additions, the bias addition: at most eight roundings
    slice backward  (L + 2) U sum |b||gout|                L = the vertex's list length: one product and at most L additions per
                                                           term, in any order
    bias gradient   (n_out + 1) U sum_p |gout|             any summation order of n_out terms; a tree sits far below it
The layer rows are float32 ROWS [n][C] (channels last); the reference's tensors are (B, C, N)."""
import numpy as np
import torch

from gemm_contract import DELTA

U = 2.0 ** -24


# ---- the three kernels ------------------------------------------------------------------------------------------------------
def invert_lists(off, H):
    """off [n_out][4] integers -> (vseg [H][2] int32, list int32 [number of valid entries], number of entries outside [0, H))"""
    flat = np.asarray(off).reshape(-1).astype(np.int64)
    valid = (flat >= 0) & (flat < H)
    order = np.argsort(flat, kind='stable')
    order = order[valid[order]]
    counts = np.bincount(flat[valid], minlength=H).astype(np.int64)
    start = np.cumsum(counts) - counts
    return np.stack([start, counts], 1).astype(np.int32), order.astype(np.int32), int((~valid).sum())


def slice_ref(feat, bary, off, bias=None):
    """feat [H][C], bary / off [n_out][4] -> (out [n_out][C] float64, S = sum_r |b||f| + |bias|)"""
    f, b, o = np.asarray(feat, np.float64), np.asarray(bary, np.float64), np.asarray(off).astype(np.int64)
    out, S = np.zeros((o.shape[0], f.shape[1])), np.zeros((o.shape[0], f.shape[1]))
    for r in range(4):
        out += b[:, r, None] * f[o[:, r]]
        S += np.abs(b[:, r, None]) * np.abs(f[o[:, r]])
    if bias is not None:
        out += np.asarray(bias, np.float64)[None]
        S += np.abs(np.asarray(bias, np.float64))[None]
    return out, S


def slice_bwd_ref(gout, bary, vseg, lst, H):
    """gout [n_out][C], bary [n_out][4], the inverse lists -> (gfeat [H][C], S = sum |b||gout|, L [H] list lengths)"""
    g, b = np.asarray(gout, np.float64), np.asarray(bary, np.float64).reshape(-1)
    vseg, lst = np.asarray(vseg).astype(np.int64), np.asarray(lst).astype(np.int64)
    L = vseg[:, 1]
    gfeat, S = np.zeros((H, g.shape[1])), np.zeros((H, g.shape[1]))
    # entry k of vertex h sits at list[vseg[h][0] + k]
    hs = np.repeat(np.arange(H), L)
    pos = np.repeat(vseg[:, 0], L) + (np.arange(L.sum()) - np.repeat(np.cumsum(L) - L, L))
    f = lst[pos]
    np.add.at(gfeat, hs, b[f, None] * g[f >> 2])
    np.add.at(S, hs, np.abs(b[f, None]) * np.abs(g[f >> 2]))
    return gfeat, S, L


def bias_grad_ref(gout):
    g = np.asarray(gout, np.float64)
    return g.sum(0), np.abs(g).sum(0)


def slice_bound(S):
    return 8 * U * S + DELTA


def slice_bwd_bound(S, L):
    return (np.asarray(L, np.float64)[:, None] + 2) * U * S + DELTA


def bias_grad_bound(S, n_out):
    return (n_out + 1) * U * S + DELTA


def ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (inf for a non-finite value)"""
    got = np.asarray(got, np.float64)
    err = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
    return float((err / bound).max()) if err.size else 0.0


# ---- the whole layer, float64 torch (autograd gives the gradients) ------------------------------------------------------------
def layer_ref(cfg, params, feat, lat, out_bary=None, out_off=None):
    """cfg: use_norm, do_splat, do_slice, last_relu, use_leaky, use_bias; params: name -> float64 tensor ('blur_conv.{i}.weight' /
    '.bias', 'bias'); feat [n_in][C] (do_splat) or [H][C] rows; lat: bary [n_in][4] float64, off [n_in][4] long, nbr [H][F] long
    (-1 = no neighbour), H.  out_bary / out_off: the out points (None: the level's own) -> [n_out][C_last] or [H][C_last]"""
    H, nbr = lat['H'], lat['nbr']
    C = feat.shape[1]
    if cfg['do_splat']:
        b, o = lat['bary'], lat['off'].reshape(-1)
        v = (b[:, :, None] * feat[:, None, :]).reshape(-1, C)
        x = torch.zeros(H, C, dtype=torch.float64).index_add(0, o, v)
        if cfg['use_norm']:
            w = torch.zeros(H, dtype=torch.float64).index_add(0, o, b.reshape(-1))
            x = x * (1.0 / (w + 1e-5))[:, None]
    else:
        x = feat
    convs = sorted({int(k.split('.')[1]) for k in params if k.startswith('blur_conv.')})
    for j, i in enumerate(convs):
        w, bi = params['blur_conv.%d.weight' % i], params['blur_conv.%d.bias' % i]
        if j == 0:
            s = torch.cat([x, torch.zeros(1, C, dtype=torch.float64)], 0)
            g = s[torch.where(nbr >= 0, nbr, torch.full_like(nbr, H))]              # [H][F][C]
            x = torch.einsum('hfc,ocf->ho', g, w[..., 0]) + bi
        else:
            x = x @ w[:, :, 0, 0].t() + bi
        if j < len(convs) - 1:
            x = torch.relu(x)
        elif cfg['last_relu']:
            x = torch.nn.functional.leaky_relu(x, 0.1) if cfg['use_leaky'] else torch.relu(x)
    if not cfg['do_slice']:
        return x
    ob = lat['bary'] if out_bary is None else out_bary
    oo = lat['off'] if out_off is None else out_off
    x = (ob[:, :, None] * x[oo]).sum(1)
    if cfg['use_bias']:
        x = x + params['bias']
    return x


def loss_weights(C, n):
    """the weights of the scalar loss (out * linspace(-1, 1)).sum() of the golden, as rows [n][C]: the linspace runs over the
    reference's (1, C, n) output, in float32 as the golden's generator makes it"""
    return torch.linspace(-1, 1, C * n, dtype=torch.float32).double().view(C, n).t()


# ---- the five variants of tests/golden/bcl_layer.npz (make_golden_bcl_layer.py) ----------------------------------------------
SCALES = (1.0, 0.75, 0.5, 0.25, 0.125)
N_POINTS, SCENE_SEED, N_SELECT = 2048, 3, 777
_BASE = dict(num_input=8, radius=1, use_bias=True, use_leaky=False, use_norm=True, do_splat=True, do_slice=True, last_relu=False,
             select=False)
VARIANTS = {
    'a': dict(_BASE, level=0, num_output=[16, 12]),
    'b': dict(_BASE, level=3, num_output=[12], last_relu=True, use_leaky=True, use_bias=False, use_norm=False),
    'c': dict(_BASE, level=0, num_output=[8, 8, 4], last_relu=True, do_splat=False, select=True),
    'd': dict(_BASE, level=0, num_output=[16, 16], radius=2),
    'e': dict(_BASE, level=3, num_output=[16, 8], do_splat=False, do_slice=False),
}
MAX_ROWS = 256


def row_stride(n):
    """the golden keeps every row_stride(n)-th row of a per-point / per-vertex array (at most MAX_ROWS rows: the file stays small)"""
    return max(1, -(-n // MAX_ROWS))


def variant_input(tag, rows, C):
    """the input rows of a variant, float32 [rows][C], from its seed"""
    return np.random.default_rng(1000 + ord(tag)).standard_normal((rows, C)).astype(np.float32)


def select_idx(n):
    """variant c: N_SELECT of the level's n points, drawn with repetition"""
    return np.random.default_rng(777).integers(0, n, N_SELECT).astype(np.int64)


def variant_weights(tag, names, shapes):
    """float32 parameters of a variant over its own state-dict name / shape list (efgh_amd.synthetic.synthetic_state_dict: the
    slice bias is non-zero); the index buffers are not included"""
    from efgh_amd import synthetic as syn
    man = [[n, list(s), 'float32'] for n, s in zip(names, shapes) if not n.endswith('_indices')]
    return syn.synthetic_state_dict(man, seed=ord(tag))
