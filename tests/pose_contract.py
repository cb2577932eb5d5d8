"""float64 contract of the kernels that turn features into a pose, a loss and the first gradient of a training step (test helper,
not collected): csrc/pose.hip (heads, yaw head, calibration chain, compose, pose loss), csrc/loss.hip (image terms), the gradient
kernels of csrc/raster.hip and csrc/eval.hip's pose errors.  Written from the reference's semantics (common/torch_utils.py:105-146
sign decode, :170-200 rotation between two vectors, :256-269 calibration chain, nets/fnet.py:87-91 yaw, losses/loss_utils.py and
losses/efghloss.py, common/helper.py:163-207), not from the kernel bodies.  Plain torch on the CPU at the dtype of its inputs.

    float64 run            the truth
    float32 run (CPU)      what float32 arithmetic costs on the same inputs: the yardstick of the ceilings below
    gradients              torch autograd of the same run

Discrete decisions (sign class, yaw column, first positive column xmin, same / opposite branch, valid mask, pixel index, selected
set) are taken ONCE from the float32 inputs by the reference's rule (`*_decide`), returned with a margin (how far the deciding
quantity is from flipping) and handed to every evaluation as given: a float64 run cannot take another branch.  The case builders
assert the margin against a stated gap unless the case is exact on purpose (an exact tie, a one-hot softmax from logits of +-200).

Error of an output: max |got - ref| / max |ref| over the output of one case (absolute where the reference is zero throughout, i.e. below 1e-30: the
gradients of a one-hot softmax are 1e-174 in float64); a NaN
matches a NaN, any other non-finite mismatch is infinite.  The ceiling of a family is a multiple of the largest error of the
float32 run over all the cases of the family: at most 4 x (the margin TAU gets in gemm_contract.py: the kernels evaluate in float32
in another order than torch), and tests/test_pose_contract_host.py recomputes the pooled values and holds every constant between
1 x and 4 x its measurement.  The measurement is a largest rounding error, so it moves with the CPU that takes it: with the same
input bits, two x86-64 machines agreed on 19 of the 22 families and differed by up to 1.8 x on the other three (head_grad,
raster_grad, pose_err_rot_quat: exp and the order of a 16684-term sum), always upwards of the figures below.  The constants stand
at 3 x: a measurement a quarter smaller or three times larger still finds them inside the band, and no kernel needs more (the
largest observed is 1.7 x its family's measurement: l_mask of a single pixel, see CEIL).

`mut` names one deliberate misreading of the reference (MUTATIONS); the host test shows that each of them leaves a ceiling."""
import math

import torch
import torch.nn.functional as F

ULP1 = 2.0 ** -23
GAP_BRANCH = 32 * ULP1       # |1 -+ c| of a near-degenerate rotation: the reference's exact branch drops K (about 3e-4 in R)
GAP_ARGMAX = 1e-3            # between the two largest logits / scores of an argmax that is no deliberate tie
GAP_SIGN = 1e-3              # |component| of a ground-truth normal that is no deliberate zero
GAP_FRAC = 0.01              # fractional part of f_idx in [GAP_FRAC, 1 - GAP_FRAC]
GAP_SELECT = 1e-4            # BCE gap across the boundary of the mined negatives that is no deliberate tie
GAP_SL1 = 0.05               # | |residual| - 1 | of the smooth-L1 translation term
GAP_PIXEL = 1e-4             # distance of a projected point from the next pixel / field-of-view boundary, in pixels / radians

LOSS_NAME = ['total', 'e_gn', 'e_gn_sgn', 'e_gn_abs', 'h_hrzn', 'h_hrzn_abs', 'h_hrzn_sgn', 'fov', 'g_trs', 'g_depth', 'g_mask']
GT_COLS = {'e_gn': (0, 3), 'e_l': (3, 19), 'h_hrzn': (19, 22), 'h_c': (22, 31), 'f_l': (31, 47), 'g_trs': (47, 50), 'g_l': (50, 66),
           'e_gn_abs': (66, 69), 'h_hrzn_abs': (69, 72)}                # h_hrzn_abs: two values and a zero
LOSS_GRADS = ('e_gn_abs', 'e_gn_sgn', 'h_hrzn_abs', 'h_hrzn_sgn', 'f_score', 'g_trs', 'e_l', 'l_depth', 'l_mask')

MUTATIONS = ['k_attached', 'r33_kept', 'fix_swapped', 'lsb_first', 'last_max', 'yaw_div_n', 'no_cos_clamp', 'total_once',
             'mask_once', 'gtrs_detached', 'no_wrap', 'window_off_one', 'neg_unclamped', 'ties_high_first', 'no_bce_clamp',
             'depth_ignores_mask', 'mask_over_valid', 'winner_only', 'range_without_w', 'rank_in_chunk']

# family -> ceiling = 3 x the pooled float32-vs-float64 error of this module on the CPU (first number of the comment, with the case
# and output that set it), then the largest kernel error observed on an MI355X over every case of tests/test_gpu_pose_contract.py
CEIL = {
    'head_val': 1.0e-06,                # 3.438e-07 (head nd=3 near_opposite R); kernel 3.256e-07 (head nd=3 near_opposite R)
    'head_grad': 1.3e-05,               # 4.436e-06 (head nd=3 near_same grad); kernel 4.476e-06 (head nd=3 near_same grad)
    'yaw_R': 5.3e-07,                   # 1.788e-07 (yaw n=509 R); kernel 1.788e-07 (yaw n=509 R)
    'calib_val': 5.5e-07,               # 1.853e-07 (calib general out); kernel 1.853e-07 (calib general out)
    'calib_grad': 6.5e-07,              # 2.195e-07 (calib pixel g_lT); kernel 1.269e-07 (calib general g_lT)
    'loss_entry': 6.0e-07,              # 2.019e-07 (loss B=5 W=64 L); kernel 1.700e-07 (loss B=1 W=600 L)
    'loss_gt': 5.6e-07,                 # 1.873e-07 (loss B=5 W=31 gt72); kernel 1.925e-07 (loss B=5 W=31 gt72)
    'loss_grad_e_gn_abs': 5.6e-07,      # 1.870e-07 (loss B=5 W=31 grad_e_gn_abs); kernel 2.177e-07 (loss B=1 W=600 grad_e_gn_abs)
    'loss_grad_e_gn_sgn': 3.0e-07,      # 1.013e-07 (loss B=1 W=31 grad_e_gn_sgn); kernel 1.107e-07 (loss B=5 W=600 grad_e_gn_sgn)
    'loss_grad_h_hrzn_abs': 2.3e-06,    # 7.694e-07 (loss B=1 W=64 grad_h_hrzn_abs); kernel 3.936e-07 (loss B=1 W=64 grad_h_hrzn_abs)
    'loss_grad_h_hrzn_sgn': 4.3e-07,    # 1.454e-07 (loss B=5 W=64 grad_h_hrzn_sgn); kernel 1.196e-07 (loss B=5 W=64 grad_h_hrzn_sgn)
    'loss_grad_f_score': 5.3e-07,       # 1.773e-07 (loss B=5 W=600 grad_f_score); kernel 1.773e-07 (loss B=5 W=600 grad_f_score)
    'loss_grad_g_trs': 3.5e-07,         # 1.194e-07 (loss B=5 W=256 grad_g_trs); kernel 1.087e-07 (loss B=5 W=600 grad_g_trs)
    'loss_grad_e_l': 4.6e-07,           # 1.554e-07 (loss B=5 W=257 grad_e_l); kernel 1.705e-07 (loss B=1 W=31 grad_e_l)
    'loss_grad_l_depth': 2.9e-07,       # 9.831e-08 (loss B=5 W=600 grad_l_depth); kernel 9.831e-08 (loss B=5 W=600 grad_l_depth)
    'loss_grad_l_mask': 3.6e-07,        # 1.229e-07 (loss B=1 W=256 grad_l_mask); kernel 1.137e-07 (loss B=1 W=64 grad_l_mask)
    'img_scalar': 1.4e-07,              # 4.961e-08 (img 3x5x7 none valid l_mask); kernel 8.318e-08 (img 1x1x1 l_mask)
    'img_grad': 2.3e-07,                # 7.976e-08 (img 2x37x53 d_depth); kernel 7.976e-08 (img 2x37x53 d_depth)
    'raster_grad': 4.2e-07,             # 1.401e-07 (raster mode=0 N=16684 g_pose); kernel 3.852e-08 (raster mode=0 N=16684 g_pose)
    'pose_err_rot_trace': 2.5e-04,      # 8.377e-05 (pose errors mode=0 rot); kernel 8.377e-05 (pose errors mode=0 rot)
    'pose_err_rot_quat': 2.4e-08,       # 8.289e-09 (pose errors mode=1 rot); kernel 1.319e-09 (pose errors mode=1 rot)
    'pose_err_trs': 1.9e-07,            # 6.656e-08 (pose errors mode=1 trs); kernel 6.656e-08 (pose errors mode=1 trs)
}
OBSERVED = {}                # family -> (largest error, case): filled by check(), printed by the last GPU test


def rel_err(got, ref):
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    if g.shape != r.shape:
        return float('inf')
    if g.numel() == 0:
        return 0.0
    d = (g - r).abs()
    d = torch.where(torch.isnan(g) & torch.isnan(r), torch.zeros_like(d), d)
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
    fin = r[torch.isfinite(r)]
    scale = float(fin.abs().max()) if fin.numel() else 0.0
    return float(d.max()) / (scale if scale > 1e-30 else 1.0)


def check(family, label, got, ref):
    """-> error of `got` against the float64 `ref`; records the family's largest in OBSERVED"""
    e = rel_err(got, ref)
    if e > OBSERVED.get(family, (-1.0, ''))[0]:
        OBSERVED[family] = (e, label)
    return e


# ---------------------------------------------------------------------------------------------------------------- decisions
def argmax_rule(x, last=False):
    """-> (FIRST maximum of every row (the last under the mutation), gap between the two largest values; inf for one column)"""
    n = x.shape[1]
    mx = x.max(1, keepdim=True).values
    idx = torch.arange(n)[None].expand_as(x)
    if last:
        i = torch.where(x == mx, idx, torch.full_like(idx, -1)).max(1).values
    else:
        i = torch.where(x == mx, idx, torch.full_like(idx, n)).min(1).values
    if n < 2:
        return i, torch.full((x.shape[0],), float('inf'))
    top = torch.topk(x.double(), 2, dim=1).values
    gap = top[:, 0] - top[:, 1]
    return i, torch.where(torch.isnan(gap), torch.zeros_like(gap), gap)


def rot_decide(v1, dest):
    """branch of rotation_between for float32 unit vectors v1 (B,3) onto the constant `dest` (torch_utils.py:179-193)"""
    d = torch.tensor(dest, dtype=torch.float32)
    c = (v1.float() * d[None]).sum(1)
    same, opp = (1 - c) == 0, (1 + c) == 0
    return dict(same=same, opp=opp, fix0=(v1[:, 0] == 0) & (d[0] == 0), fix2=(v1[:, 2] == 0) & (d[2] == 0),
                margin=torch.minimum((1 - c).abs(), (1 + c).abs()).double())


def _unit(lg):
    a = torch.softmax(lg, 1)
    return a / torch.sqrt((a * a).sum(1, keepdim=True))


def _signs(cls, nd, dtype, mut):
    shifts = torch.arange(nd) if 'lsb_first' in mut else torch.arange(nd - 1, -1, -1)
    return (((cls[:, None] >> shifts[None]) & 1) * 2 - 1).to(dtype)


def _pad3(v):
    return v if v.shape[1] == 3 else torch.cat([v, torch.zeros_like(v[:, :1])], 1)


def head_decide(abs32, sgn32, nd, dest, mut=()):
    cls, gap = argmax_rule(sgn32[:, :1 << nd], last='last_max' in mut)
    nv = _unit(abs32.float()) * _signs(cls, nd, torch.float32, ())
    return dict(cls=cls, cls_margin=gap, rot=rot_decide(_pad3(nv), dest))


# ---------------------------------------------------------------------------------------------------------------- heads
def rotation_between(v1, dest, br, mut=()):
    """torch_utils.py:170-200.  v1 (B,3), `dest` a constant, `br` from rot_decide -> (B,4,4).  K from DETACHED values (:184,194):
    only (1 - c) / s^2 carries gradient.  same: the identity.  opposite: -I with [0][0] flipped back when both x components vanish,
    else [2][2] when both z components do, and [3][3] = -1 (the reference negates a 4x4 identity)"""
    B, dt = v1.shape[0], v1.dtype
    d = torch.tensor(dest, dtype=dt)
    exact = br['same'] | br['opp']
    # a sample on an exact branch never evaluates the general formula (0 / 0 there): hand it a vector at a right angle instead
    v1 = torch.where(exact[:, None], torch.roll(d, 1)[None].expand(B, 3), v1)
    v2 = d[None].expand(B, 3)
    v = torch.linalg.cross(v1, v2, dim=1)
    c = (v1 * v2).sum(1)
    s = torch.sqrt((v * v).sum(1))
    k = v if 'k_attached' in mut else v.detach()
    z = torch.zeros_like(c)
    K = torch.stack([torch.stack([z, -k[:, 2], k[:, 1]], 1), torch.stack([k[:, 2], z, -k[:, 0]], 1),
                     torch.stack([-k[:, 1], k[:, 0], z], 1)], 1)
    eye = torch.eye(3, dtype=dt)[None].expand(B, 3, 3)
    r3 = eye + K + torch.bmm(K, K) * ((1 - c) / (s * s))[:, None, None]
    if 'fix_swapped' in mut:
        f2 = br['fix2']
        f0 = br['fix0'] & ~f2
    else:
        f0 = br['fix0']
        f2 = br['fix2'] & ~f0
    one = torch.ones_like(c)
    neg = torch.diag_embed(torch.stack([torch.where(f0, one, -one), -one, torch.where(f2, one, -one)], 1))
    r3 = torch.where(br['opp'][:, None, None], neg, r3)
    r3 = torch.where(br['same'][:, None, None], eye, r3)
    r33 = one if 'r33_kept' in mut else torch.where(br['opp'] & ~br['same'], -one, one)
    top = torch.cat([r3, torch.zeros((B, 3, 1), dtype=dt)], 2)
    bot = torch.cat([torch.zeros((B, 1, 3), dtype=dt), r33[:, None, None]], 2)
    return torch.cat([top, bot], 1)


def head(abs_logits, dec, nd, dest, mut=()):
    """enet.py:161-164 / hnet.py:59-63 + torch_utils.py:105-146: -> (abs (B,nd), normal (B,nd), R (B,4,4))"""
    a = _unit(abs_logits)
    nv = a * _signs(dec['cls'], nd, a.dtype, mut)
    return a, nv, rotation_between(_pad3(nv), dest, dec['rot'], mut)


def yaw_decide(score32, mut=()):
    """fnet.py:87-89: first maximum -> yaw in float32 -> cos / sin in double, rounded to float: the vector both evaluations rotate"""
    n = score32.shape[1]
    idx, gap = argmax_rule(score32, last='last_max' in mut)
    f_idx = idx[:, None].float()
    f_rad = -(f_idx / (n if 'yaw_div_n' in mut else n - 1)) * 2 * math.pi + math.pi
    assert f_rad.dtype == torch.float32
    rad = f_rad[:, 0].double()
    v1 = torch.stack([torch.cos(rad), torch.sin(rad), torch.zeros_like(rad)], 1).float()
    return dict(idx=idx, idx_margin=gap, v1=v1, rot=rot_decide(v1, (1., 0., 0.)))


def yaw_rotation(dec, dtype, mut=()):
    return rotation_between(dec['v1'].to(dtype), (1., 0., 0.), dec['rot'], mut)


def cam_T_velo(c_T, l_T, calib, A):
    """torch_utils.py:256-269: A^-1 (c_T (A (calib l_T)))"""
    return torch.bmm(torch.linalg.inv(A), torch.bmm(c_T, torch.bmm(A, torch.bmm(calib, l_T))))


# ---------------------------------------------------------------------------------------------------------------- pose loss
def _bce_clamped(p, t, mut=()):
    if 'no_bce_clamp' in mut:
        return -(t * torch.log(p) + (1 - t) * torch.log(1 - p))
    return F.binary_cross_entropy(p, t, reduction='none')      # log terms clamped at -100, gradient denominator at 1e-12


def _gt_normal(R, col):
    g = R[:, :3, col]
    return g / torch.sqrt((g * g).sum(1, keepdim=True))


def _sign_class(g, nd):
    """loss_utils.py:33-41: sign -> {0, 1} (0 and -1 give 0), bits MSB-first"""
    w = torch.tensor([2 ** (nd - 1 - i) for i in range(nd)])
    return ((g[:, :nd] > 0).long() * w[None]).sum(1)


def _f_axis(e_l, T4):
    Tinv = torch.linalg.inv(T4[:, :3, :3])
    return torch.bmm(torch.bmm(e_l[:, :3, :3], Tinv), torch.tensor([1., 0., 0.], dtype=e_l.dtype)[None, :, None].expand(e_l.shape[0], 3, 1))


def rank_rule(lc, mut=()):
    """position of every column in the descending sort of its row, the lower column first among equals"""
    W = lc.shape[1]
    q, j = torch.arange(W)[None, :, None], torch.arange(W)[None, None, :]          # rank[b][j] = #{q before j}
    before = (q > j) if 'ties_high_first' in mut else (q < j)
    m = (lc[:, :, None] > lc[:, None, :]) | ((lc[:, :, None] == lc[:, None, :]) & before)
    if 'rank_in_chunk' in mut:
        m = m & ((q // 256) == (j // 256))
    return m.sum(1)


def loss_decide(inp, cfg, mut=()):
    """every discrete decision of the pose loss from the float32 inputs, with its margin"""
    lam, pos_num, neg_ratio = cfg
    x = {k: v.float() for k, v in inp.items()}
    B, W = x['f_score'].shape
    g_e, g_h = _gt_normal(x['rand_init_l'], 2), _gt_normal(x['rand_init_c'], 1)
    dec = dict(cls_e=_sign_class(g_e, 3), cls_h=_sign_class(g_h, 2), rot_e=rot_decide(g_e, (0., 0., 1.)),
               rot_h=rot_decide(g_h, (0., 1., 0.)))
    comp = torch.cat([g_e, g_h[:, :2]], 1).abs().double()
    dec['sign_margin'] = torch.where(comp == 0, torch.full_like(comp, float('inf')), comp).min(1).values     # an exact zero is a case
    axis = _f_axis(x['e_l'], x['sensor2_T_sensor1'])
    yaw = torch.atan2(axis[:, 1, 0], axis[:, 0, 0])
    f_idx = ((-yaw + math.pi) / (2 * math.pi)) * W                                   # loss_utils.py:125-127
    xmin = f_idx.long() - int(pos_num / 2) + (1 if 'window_off_one' in mut else 0)
    frac = (f_idx - torch.floor(f_idx)).double()
    dec['xmin'], dec['xmin_margin'] = xmin, torch.minimum(frac, 1 - frac)
    j = torch.arange(W)[None, :]
    if 'no_wrap' in mut:
        pos = (j >= xmin[:, None]) & (j < xmin[:, None] + pos_num)
    else:
        pos = torch.remainder(j - xmin[:, None], W) < pos_num
    lc = torch.where(pos, torch.zeros_like(x['f_score']), _bce_clamped(x['f_score'], torch.zeros_like(x['f_score'])))
    num_neg = neg_ratio * pos.sum(1, keepdim=True).float()
    if 'neg_unclamped' not in mut:
        num_neg = torch.clamp(num_neg, max=W - 1)
    sel = pos | (rank_rule(lc, mut).float() < num_neg)
    dec['pos'], dec['sel'], dec['n_selected'] = pos, sel, sel.sum().float()
    # gap across the selection boundary: between the last mined column and the first one left out
    srt = lc.double().sort(1, descending=True).values
    k = torch.ceil(num_neg[:, 0]).long()
    gap = torch.full((B,), float('inf'), dtype=torch.float64)
    for b in range(B):
        if 0 < int(k[b]) < W and float(srt[b, int(k[b]) - 1]) > 0:
            gap[b] = srt[b, int(k[b]) - 1] - srt[b, int(k[b])]
    dec['select_margin'] = gap
    return dec


def _cosine(x, y, mut=()):
    """F.cosine_similarity(dim=1): each norm clamped at 1e-8"""
    nx, ny = torch.linalg.vector_norm(x, dim=1, keepdim=True), torch.linalg.vector_norm(y, dim=1, keepdim=True)
    if 'no_cos_clamp' not in mut:
        nx, ny = nx.clamp_min(1e-8), ny.clamp_min(1e-8)
    return ((x / nx) * (y / ny)).sum(1)


def _embed44(m3):
    B, dt = m3.shape[0], m3.dtype
    top = torch.cat([m3, torch.zeros((B, 3, 1), dtype=dt)], 2)
    return torch.cat([top, torch.tensor([0., 0., 0., 1.], dtype=dt)[None, None].expand(B, 1, 4)], 1)


def pose_loss(inp, dec, cfg, mut=()):
    """losses/efghloss.py:19-38 over loss_utils.py:25-58 (E), :227-262 (H), :77-144 (F), :165-207 (G)
    -> (L (11,) in LOSS_NAME order, gt72 (B,72))"""
    lam, pos_num, neg_ratio = cfg
    dt = inp['f_score'].dtype
    B, W = inp['f_score'].shape
    T4 = inp['sensor2_T_sensor1']
    # E / H: ground-truth normal = a column of the random initial rotation, normalised; rotation onto e3 / e2
    g_e, g_h = _gt_normal(inp['rand_init_l'], 2), _gt_normal(inp['rand_init_c'], 1)
    e_l = rotation_between(g_e, (0., 0., 1.), dec['rot_e'], mut)
    h_c = rotation_between(g_h, (0., 1., 0.), dec['rot_h'], mut)
    la_e = (1 - _cosine(inp['e_gn_abs'], g_e.abs(), mut)).mean() * 10.0
    ls_e = F.cross_entropy(inp['e_gn_sgn'], dec['cls_e'])
    la_h = (1 - _cosine(inp['h_hrzn_abs'], g_h[:, :2].abs(), mut)).mean() * 10.0
    ls_h = F.cross_entropy(inp['h_hrzn_sgn'], dec['cls_h'])
    L = {'e_gn': (la_e + ls_e) * lam['e_gn'], 'e_gn_abs': la_e * lam['e_gn'], 'e_gn_sgn': ls_e * lam['e_gn'],
         'h_hrzn': (la_h + ls_h) * lam['h_hrzn'], 'h_hrzn_abs': la_h * lam['h_hrzn'], 'h_hrzn_sgn': ls_h * lam['h_hrzn']}
    # F: positives as given, the mined negatives as given; mean over the selected scores
    Tinv = torch.linalg.inv(T4[:, :3, :3])
    f_l = _embed44(torch.linalg.inv(torch.bmm(e_l[:, :3, :3], Tinv)))
    t = dec['pos'].to(dt)
    lf = _bce_clamped(inp['f_score'], t, mut)
    L['fov'] = torch.where(dec['sel'], lf, torch.zeros_like(lf)).sum() / dec['n_selected'].to(dt) * lam['fov']
    # G: the ground-truth translation is built from UN-detached predictions (:170-175)
    origin = torch.tensor([0., 0., 0., 1.], dtype=dt)[None, :, None].expand(B, 4, 1)
    pef = torch.bmm(inp['f_l'], inp['e_l'])
    g_trs = torch.bmm(torch.bmm(T4, torch.linalg.inv(pef)), origin)[:, :3, 0]
    if 'gtrs_detached' in mut:
        g_trs = g_trs.detach()
    gcp = torch.bmm(torch.bmm(T4, torch.linalg.inv(torch.bmm(f_l, e_l))), origin)[:, :3, 0]
    g_l = torch.eye(4, dtype=dt)[None].repeat(B, 1, 1)
    g_l[:, :3, 3] = gcp.detach()
    L['g_trs'] = F.smooth_l1_loss(g_trs, inp['g_trs']) * lam['g_trs']
    L['g_depth'] = inp['l_depth'] * lam['g_depth']
    L['g_mask'] = inp['l_mask'] * lam['g_mask'] * (1.0 if 'mask_once' in mut else lam['g_depth'])        # :199 and :204
    names = [k for k in L if not ('total_once' in mut and k in ('e_gn', 'h_hrzn'))]
    L['total'] = sum(L[k] for k in names)                                                                # efghloss.py:33-36
    gt = torch.cat([g_e, e_l.reshape(B, 16), g_h, h_c[:, :3, :3].reshape(B, 9), f_l.reshape(B, 16), g_trs, g_l.reshape(B, 16),
                    g_e.abs(), g_h[:, :2].abs(), torch.zeros((B, 1), dtype=dt)], 1)
    return torch.stack([L[k] for k in LOSS_NAME]), gt.detach()


def pose_loss_run(case, dtype, mut=()):
    """one evaluation with its gradients: -> {'L', 'gt72', 'grad_<input>'}"""
    dec = loss_decide(case['inp'], case['cfg'], mut) if mut else case['dec']
    x = {k: v.to(dtype).clone() for k, v in case['inp'].items()}
    for k in LOSS_GRADS:
        x[k].requires_grad_(True)
    L, gt = pose_loss(x, dec, case['cfg'], mut)
    (L * case['weights'].to(dtype)).sum().backward()
    out = {'L': L.detach(), 'gt72': gt}
    for k in LOSS_GRADS:
        out['grad_' + k] = torch.zeros_like(x[k]) if x[k].grad is None else x[k].grad
    return out


# ---------------------------------------------------------------------------------------------------------------- image terms
def gimg_decide(gdep4, img_mask, mut=()):
    gd = gdep4[..., 3].float()
    return dict(valid=(gd > 0) if 'depth_ignores_mask' in mut else (gd > 0) & (img_mask > 0), gt_mask=gd > 0)


def gimg_loss(pred_depth, pred_mask, gdep4, dec, mut=()):
    """loss_utils.py:186-199: pred_depth (B,1,H,W), pred_mask (B,C,H,W) whose channel 0 is the mask -> (l_depth, l_mask)"""
    B = pred_depth.shape[0]
    gd = gdep4[..., 3].to(pred_depth.dtype)
    valid = dec['valid']
    l_depth = ((gd - pred_depth[:, 0])[valid] ** 2).mean()                     # NaN over an empty selection, as the reference's
    p, y = pred_mask[:, 0].reshape(B, -1), dec['gt_mask'].to(pred_depth.dtype).reshape(B, -1)
    lm = _bce_clamped(p, y, mut)
    l_mask = lm[valid.reshape(B, -1)].mean() if 'mask_over_valid' in mut else lm.mean()
    return l_depth, l_mask


def gimg_run(case, dtype, mut=()):
    dec = gimg_decide(case['gdep4'], case['img_mask'], mut) if mut else case['dec']
    pd, pm = case['pred_depth'].to(dtype).clone().requires_grad_(True), case['pred_mask'].to(dtype).clone().requires_grad_(True)
    ld, lm = gimg_loss(pd, pm, case['gdep4'], dec, mut)
    # the two terms are differentiated apart: a NaN l_depth must not reach the mask gradient
    gd, = torch.autograd.grad(ld * case['g'][0].to(dtype), pd, allow_unused=True)
    gm, = torch.autograd.grad(lm * case['g'][1].to(dtype), pm)
    return {'l_depth': ld.detach(), 'l_mask': lm.detach(), 'd_depth': torch.zeros_like(pd) if gd is None else gd, 'd_mask': gm,
            'n_valid': dec['valid'].sum().float(), 'gt_depth': case['gdep4'][..., 3][:, None].clone(),
            'gt_mask': dec['gt_mask'][:, None].float()}


# ---------------------------------------------------------------------------------------------------------------- raster gradients
def raster_decide(pc, pose, H, W, mode, fov=None):
    """pixel of every point by the reference's float32 rule (torch_utils.py:11-59 range, :61-103 depth): -> (pix (B,N) int32 with
    -1 for a point that is not rasterised, margin (B,N): distance from the next pixel or view boundary)"""
    pc, pose = pc.float(), pose.float()
    B, _, N = pc.shape
    p1 = torch.cat([pc, torch.ones((B, 1, N))], 1)
    q = torch.bmm(pose, p1)
    if mode == 0:
        fov_up, fov_down = fov
        r = torch.sqrt((q * q).sum(1))                                          # :29, the w row included
        pitch, yaw = torch.asin(q[:, 2] / r), torch.atan2(q[:, 1], q[:, 0])
        u = ((fov_up - pitch) / (fov_up - fov_down)) * (H - 1)
        v = ((-yaw + math.pi) / (2 * math.pi)) * (W - 1)
        inside = (pitch < fov_up) & (pitch > fov_down)
        edge = torch.minimum((pitch - fov_up).abs(), (pitch - fov_down).abs())
        ui, vi = u.long(), v.long()
        inside = inside & (ui >= 0) & (ui < H) & (vi >= 0) & (vi < W)
    else:
        w = q[:, 2]
        v, u = q[:, 0] / w, q[:, 1] / w                                         # v: column, u: row
        inside = (v < W) & (v > 0) & (u < H) & (u > 0) & (w > 0)
        edge = w.abs()
        ui, vi = u.long(), v.long()
    fr = lambda t: torch.minimum(t - torch.floor(t), torch.ceil(t) - t)
    margin = torch.minimum(torch.minimum(fr(u), fr(v)), edge)
    margin = torch.where(torch.isfinite(margin), margin, torch.zeros_like(margin))
    pix = torch.where(inside, ui * W + vi, torch.full_like(ui, -1)).to(torch.int32)
    return pix, margin.double()


def raster_values_grad(pix, gimg):
    """index_put's autograd formula: EVERY rasterised point receives grad_img[pix], overwritten points included; exact"""
    B, N = pix.shape
    g = gimg.reshape(B, -1, 4)
    out = torch.gather(g, 1, pix.clamp_min(0).long()[:, :, None].expand(B, N, 4))
    return torch.where((pix >= 0)[:, :, None], out, torch.zeros_like(out))


def raster_pose_grad(pix, gimg, pc, pose, mode, dtype, mut=()):
    """gradient of sum_points <grad_img[pix], values(pose)> w.r.t. the pose: range values (x, y, z, |q|) with q = E [p;1] (4 rows),
    depth values (px, py, pz, w) with w the third row of the projection"""
    B, N = pix.shape
    pose = pose.to(dtype).clone().requires_grad_(True)
    p1 = torch.cat([pc.to(dtype), torch.ones((B, 1, N), dtype=dtype)], 1)
    q = torch.bmm(pose, p1)
    if mode == 0:
        r = torch.sqrt((q[:, :3] ** 2).sum(1)) if 'range_without_w' in mut else torch.sqrt((q * q).sum(1))
        vals = torch.cat([q[:, :3], r[:, None]], 1).transpose(1, 2)
    else:
        vals = torch.cat([p1[:, :3], q[:, 2:3]], 1).transpose(1, 2)
    keep = pix >= 0
    if 'winner_only' in mut:                                                    # the point with the largest index of its pixel
        n = torch.arange(N)[None].expand(B, N)
        win = torch.full((B, int(gimg.shape[1] * gimg.shape[2])), -1, dtype=torch.long)
        win.scatter_reduce_(1, pix.clamp_min(0).long(), torch.where(keep, n, torch.full_like(n, -1)), 'amax')
        keep = keep & (torch.gather(win, 1, pix.clamp_min(0).long()) == n)
    g = raster_values_grad(pix, gimg).to(dtype)
    (torch.where(keep[:, :, None], g * vals, torch.zeros_like(vals))).sum().backward()
    return pose.grad.reshape(B, -1)


# ---------------------------------------------------------------------------------------------------------------- pose errors
def pose_errors(gt, pred, mode):
    """common/helper.py:198-207 (mode 0: trace form, Euclidean translation error) and :165-196 (mode 1: angle of
    gt_R pred_R^T as atan2(|vee| / 2, (trace - 1) / 2), which is the reference's 2 atan2(|v|, |w|) of the quaternion; mean
    absolute translation error), in degrees"""
    dt = gt[:, :3, 3] - pred[:, :3, 3]
    if mode == 0:
        tr = (pred[:, :3, :3] * gt[:, :3, :3]).sum((1, 2))
        rot = 180.0 * torch.acos(((tr - 1) / 2).clamp(-1, 1)) / math.pi
        return rot, torch.sqrt((dt * dt).sum(1))
    R = torch.bmm(gt[:, :3, :3], pred[:, :3, :3].transpose(1, 2))
    v = torch.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1)
    s, c = 0.5 * torch.sqrt((v * v).sum(1)), 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1)
    return torch.atan2(s, c) * (180.0 / math.pi), dt.abs().mean(1)


# ================================================================================================================ cases
# Seeded, nothing read from disk, the smallest shapes that reach every path.  Every builder asserts the margins of its decisions.
_CACHE = {}


def _cached(fn):
    def wrap(*a):
        key = (fn.__name__,) + a
        if key not in _CACHE:
            _CACHE[key] = fn(*a)
        return _CACHE[key]
    return wrap


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# Inputs must be the same bits on every machine (the ceilings are multiples of a float32 error measured on them): uniform numbers
# are drawn in float64, the normal ones made from them in float64, every transcendental of a builder is taken in float64, and only
# then is anything rounded to float32.  What a builder does in float32 is +, -, * and /.
def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64).float()


def _randn(g, *shape):
    u1, u2 = torch.rand(*shape, generator=g, dtype=torch.float64), torch.rand(*shape, generator=g, dtype=torch.float64)
    return (torch.sqrt(-2 * torch.log(1 - u1)) * torch.cos(2 * math.pi * u2)).float()


def _unit64(lg):
    return _unit(lg.double()).float()


def _sigmoid64(x):
    return torch.sigmoid(x.double()).float()


def _rot_xyz(ang):
    """(B,3) angles -> Rz Ry Rx, float64"""
    ang = ang.double()
    c, s = torch.cos(ang), torch.sin(ang)
    o, z = torch.ones_like(c[:, 0]), torch.zeros_like(c[:, 0])
    Rx = torch.stack([o, z, z, z, c[:, 0], -s[:, 0], z, s[:, 0], c[:, 0]], 1).reshape(-1, 3, 3)
    Ry = torch.stack([c[:, 1], z, s[:, 1], z, o, z, -s[:, 1], z, c[:, 1]], 1).reshape(-1, 3, 3)
    Rz = torch.stack([c[:, 2], -s[:, 2], z, s[:, 2], c[:, 2], z, z, z, o], 1).reshape(-1, 3, 3)
    return Rz @ Ry @ Rx


HEAD_REGIMES = ('random', 'near_same', 'near_opposite', 'exact_same', 'exact_opposite', 'sign_tie')
HEAD_DEST = {3: (0., 0., 1.), 2: (0., 1., 0.)}


@_cached
def head_case(nd, regime):
    """B = 67 (one thread per sample, 64 per workgroup); logits are row views of (B,32) buffers"""
    B, ncls, dest = 67, 1 << nd, HEAD_DEST[nd]
    g = _gen(100 * nd + HEAD_REGIMES.index(regime))
    abuf, sbuf = _randn(g, B, 32) * 3, _randn(g, B, 32)
    want = sbuf[:, :ncls].argmax(1)
    if regime in ('near_same', 'near_opposite'):
        # softmax (eps, eps, 1): 1 - |c| is about sum eps^2 / 2, kept in [4e-6, 1e-3], i.e. above 32 ulp(1)
        abuf[:, :nd] = 0.0
        abuf[:, :nd - 1] = -(3.6 + 2.2 * _rand(g, B, nd - 1))
    if regime in ('exact_same', 'exact_opposite'):
        abuf[:, :nd] = -200.0                                   # exp(-400) is zero in float32: one-hot in any evaluation order
        abuf[:, nd - 1] = 200.0
    if regime in ('near_same', 'exact_same'):
        want = want | 1                                         # the bit of the destination axis is the last one
    if regime in ('near_opposite', 'exact_opposite'):
        want = want & ~1
    top = sbuf[:, :ncls].max(1).values
    sbuf[torch.arange(B), want] = top + 0.01
    if regime == 'sign_tie':
        other = (want + 1 + torch.randint(0, ncls - 1, (B,), generator=g)) % ncls
        sbuf[torch.arange(B), other] = top + 0.01
    dec = head_decide(abuf[:, :nd], sbuf, nd, dest)
    if regime in ('random', 'sign_tie'):                        # scale 3 now and then saturates the softmax: soften those rows
        abuf[dec['rot']['margin'] < 1e-5, :nd] *= 0.3
        dec = head_decide(abuf[:, :nd], sbuf, nd, dest)
    if regime == 'sign_tie':
        assert bool((dec['cls_margin'] == 0).all()) and bool((dec['cls'] == torch.minimum(want, other)).all())
    else:
        assert float(dec['cls_margin'].min()) >= GAP_ARGMAX and bool((dec['cls'] == want).all())
    if regime.startswith('exact'):
        assert bool(dec['rot']['same' if regime == 'exact_same' else 'opp'].all())
    else:
        assert float(dec['rot']['margin'].min()) >= GAP_BRANCH, float(dec['rot']['margin'].min())
        if regime.startswith('near'):
            assert float(dec['rot']['margin'].max()) <= 2e-3
    return dict(name='head nd=%d %s' % (nd, regime), nd=nd, dest=dest, abuf=abuf, sbuf=sbuf, dec=dec, exact=regime.startswith('exact'),
                ga=_randn(g, B, nd), gn=_randn(g, B, nd), gR=_randn(g, B, 4, 4))


def head_cases():
    return [head_case(nd, r) for nd in (3, 2) for r in HEAD_REGIMES]


HEAD_FAMILY = {'abs': 'head_val', 'normal': 'head_val', 'R': 'head_val', 'grad': 'head_grad'}
HEAD_GRADS = ('abs', 'normal', 'R', 'all')     # the incoming gradients present: each alone, then all together


def head_run(case, dtype, mut=()):
    """'grad' (4,B,nd): the logit gradient with only g_abs, only g_normal, only g_R, and all three.  The four are one output of one
    kernel: their error is taken relative to the largest of them all (near the degenerate directions the gradient through R alone
    is a difference of two terms 1 / angle^2 apart and carries no digit of its own)"""
    nd = case['nd']
    dec = head_decide(case['abuf'][:, :nd], case['sbuf'], nd, case['dest'], mut) if mut else case['dec']
    x = case['abuf'][:, :nd].to(dtype).clone().requires_grad_(True)
    a, nv, R = head(x, dec, nd, case['dest'], mut)
    terms = {'abs': (a * case['ga'].to(dtype)).sum(), 'normal': (nv * case['gn'].to(dtype)).sum(), 'R': (R * case['gR'].to(dtype)).sum()}
    terms['all'] = sum(terms.values())
    grads = []
    for k in HEAD_GRADS:
        g, = torch.autograd.grad(terms[k], x, retain_graph=True, allow_unused=True)
        grads.append(torch.zeros_like(x) if g is None else g)
    return {'abs': a.detach(), 'normal': nv.detach(), 'R': R.detach(), 'grad': torch.stack(grads)}


YAW_N = (2, 63, 64, 65, 509)


@_cached
def yaw_case(n):
    """rows of a buffer with a pitch above n: a peak in column 0, n-1 and (n-1)/2 (n odd); equal maxima in one lane (columns j and
    j + 64) and in neighbouring lanes (j and j + 1); a row of -inf; plain rows"""
    g = _gen(200 + n)
    rows = [('col0', [0]), ('last', [n - 1]), ('lanes', [n // 3, n // 3 + 1])]
    if n % 2:
        rows.append(('middle', [(n - 1) // 2]))
    if n > 64:
        rows.append(('lane', [(n - 65) // 2, (n - 65) // 2 + 64]))
    rows += [('minus_inf', []), ('plain', None), ('plain', None), ('plain', None)]
    buf = _rand(g, len(rows), n + 7) * 0.9
    exempt = torch.zeros(len(rows), dtype=torch.bool)
    first = torch.zeros(len(rows), dtype=torch.long)
    for r, (kind, cols) in enumerate(rows):
        if kind == 'minus_inf':
            buf[r, :n] = float('-inf')
        if cols is None:
            cols = [int(torch.randint(0, n, (1,), generator=g))]
        for c in cols:
            buf[r, c] = 0.95
        exempt[r] = kind == 'minus_inf' or len(cols) > 1
        first[r] = min(cols) if cols else 0
    score = buf[:, :n]
    dec = yaw_decide(score)
    assert bool((dec['idx'] == first).all())
    assert float(dec['idx_margin'][~exempt].min()) >= GAP_ARGMAX
    exact = dec['rot']['same'] | dec['rot']['opp']
    assert not bool((~exact).any()) or float(dec['rot']['margin'][~exact].min()) >= GAP_BRANCH
    assert bool(dec['rot']['opp'][0]) and bool(dec['rot']['opp'][1]) and (n % 2 == 0 or bool(dec['rot']['same'][3]))
    return dict(name='yaw n=%d' % n, n=n, score=score, dec=dec, exact=exact)


def yaw_run(case, dtype, mut=()):
    dec = yaw_decide(case['score'], mut) if mut else case['dec']
    return {'R': yaw_rotation(dec, dtype, mut)}


@_cached
def calib_case(kind):
    """B = 67; the loaders' pixel-centre A or a general invertible one; calibration at scale 700"""
    B = 67
    g = _gen(300 + ('pixel', 'general').index(kind))
    A = torch.eye(3)[None].repeat(B, 1, 1)
    if kind == 'pixel':
        A[:, 0, 2], A[:, 1, 2] = -640.0, -192.0
    else:
        A = A + 0.2 * _randn(g, B, 3, 3)
        assert float(torch.linalg.cond(A.double()).max()) < 50
    calib = _randn(g, B, 3, 4) * torch.tensor([700., 700., 1.])[None, :, None]
    return dict(name='calib ' + kind, A=A, calib=calib, c_T=torch.eye(3)[None] + 0.1 * _randn(g, B, 3, 3),
                l_T=_randn(g, B, 4, 4), g=_randn(g, B, 3, 4))


def calib_run(case, dtype, mut=()):
    c, l = case['c_T'].to(dtype).clone().requires_grad_(True), case['l_T'].to(dtype).clone().requires_grad_(True)
    out = cam_T_velo(c, l, case['calib'].to(dtype), case['A'].to(dtype))
    (out * case['g'].to(dtype)).sum().backward()
    return {'out': out.detach(), 'g_cT': c.grad, 'g_lT': l.grad}


@_cached
def compose_case():
    g = _gen(310)
    return dict(name='compose', a=_randn(g, 67, 4, 4), b=_randn(g, 67, 4, 4),
                g=_randn(g, 67, 4, 4))


def compose_run(case, dtype, mut=()):
    a, b = case['a'].to(dtype).clone().requires_grad_(True), case['b'].to(dtype).clone().requires_grad_(True)
    out = torch.bmm(a, b)
    (out * case['g'].to(dtype)).sum().backward()
    return {'out': out.detach(), 'g_a': a.grad, 'g_b': b.grad}                 # g b^T and a^T g: the two transposed forms


CALIB_FAMILY = {'out': 'calib_val', 'g_cT': 'calib_grad', 'g_lT': 'calib_grad', 'g_a': 'calib_grad', 'g_b': 'calib_grad'}

LOSS_B, LOSS_W = (1, 5), (31, 64, 256, 257, 600)
LOSS_CFG = ({'e_gn': 1.3, 'h_hrzn': 0.7, 'fov': 1.1, 'g_trs': 2.0, 'g_depth': 0.9, 'g_mask': 0.6}, 30, 3)
LOSS_HARSH_W = (64, 257)     # the widths whose cases carry saturated scores, a zero e_gn_abs row and an exactly aligned ground-truth
#                              normal: their gradients reach 1e12 / 1e8, which would hide every other element of the same output
_WINDOWS = ('wrap_low', 'wrap_high', 'ends_at_W', 'middle', 'middle')


@_cached
def loss_case(B, W):
    """layouts alternate with the case: rand_init_* as 3x3 or 4x4; e_gn_abs / h_hrzn_abs / g_trs as (B,n,1) or as 2-D row views of
    a wider buffer.  Sign logits and f_score are always row views with a pitch."""
    lam, pos_num, neg_ratio = LOSS_CFG
    ci = LOSS_B.index(B) * len(LOSS_W) + LOSS_W.index(W)
    g = _gen(400 + ci)
    harsh = W in LOSS_HARSH_W
    rnd = lambda *s: _randn(g, *s)
    uni = lambda *s: _rand(g, *s)
    # ground truth
    Rl, Rc = _rot_xyz((uni(B, 3) - 0.5) * 1.0), _rot_xyz((uni(B, 3) - 0.5) * 0.6)
    for _ in range(8):                                             # draw again where a component of a normal is nearly zero
        bad = torch.cat([Rl[:, :, 2], Rc[:, :2, 1]], 1).abs().min(1).values < 10 * GAP_SIGN
        Rl[bad], Rc[bad] = _rot_xyz((uni(B, 3) - 0.5) * 1.0)[bad], _rot_xyz((uni(B, 3) - 0.5) * 0.6)[bad]
    ang = (uni(B, 3) - 0.5)
    ang[:, 1:] = 0
    Rl[0] = _rot_xyz(ang)[0]                                       # Rx: the third column has an exactly zero x component
    if harsh and B > 1:
        ang = (uni(B, 3) - 0.5)
        ang[:, :2] = 0
        Rl[1] = _rot_xyz(ang)[1]                                   # Rz: the third column is e3 exactly ("same")
    T4 = torch.eye(4, dtype=torch.float64)[None].repeat(B, 1, 1)
    T4[:, :3, :3] = _rot_xyz((uni(B, 3) - 0.5) * 0.4)
    T4[:, :3, 3] = (uni(B, 3) * 2 - 1).double()
    dim = 3 if ci % 2 == 0 else 4
    emb = lambda R: R.float().contiguous() if dim == 3 else _embed44(R).float().contiguous()
    # predictions: e_l places the positive window: axis = e_l T^-1 e1 = Rz(yaw) e1
    kinds = [_WINDOWS[(ci + b) % 5] if B == 1 else _WINDOWS[b] for b in range(B)]
    centre = {'wrap_low': 5.5, 'wrap_high': W - 5.5, 'ends_at_W': W - pos_num // 2 + 0.5, 'middle': W // 2 + 0.37}
    f_idx = torch.tensor([centre[k] for k in kinds], dtype=torch.float64)
    yaw = math.pi - 2 * math.pi * f_idx / W
    az = torch.zeros(B, 3, dtype=torch.float64)
    az[:, 2] = yaw
    e_l = _embed44(_rot_xyz(az) @ T4[:, :3, :3])
    if ci % 2:
        e_l[:, :3, 3] = 0.1 * rnd(B, 3).double()
    az[:, 2] = (uni(B) * 6 - 3).double()
    f_l = _embed44(_rot_xyz(az))
    if harsh:
        f_l[B - 1] = torch.diag(torch.tensor([-1., -1., 1., -1.], dtype=torch.float64))       # the yaw head's "opposite" output
    e_l, f_l, T4 = e_l.float(), f_l.float(), T4.float()
    gtrs = torch.bmm(torch.bmm(T4.double(), torch.linalg.inv(torch.bmm(f_l.double(), e_l.double()))),
                     torch.tensor([0., 0., 0., 1.], dtype=torch.float64)[None, :, None].expand(B, 4, 1))[:, :3, 0]
    res = torch.tensor([0.3, -1.7, 0.8, -0.4, 1.3, -0.9, 2.1, 0.1, -1.2])[torch.arange(B * 3) % 9].reshape(B, 3)
    res = res * (1 + 0.05 * uni(B, 3))
    g_trs = (gtrs + res.double()).float()
    assert float(((g_trs.double() - gtrs).abs() - 1).abs().min()) >= GAP_SL1
    e_abs, h_abs = _unit64(rnd(B, 3)), _unit64(rnd(B, 2))
    if harsh:
        e_abs[B - 1] = 0.0                                         # the cosine's 1e-8 clamp
    sbuf_e, sbuf_h = rnd(B, 32), rnd(B, 32)
    fbuf = _sigmoid64(2 * rnd(B, W + 5))
    inp = dict(e_gn_sgn=sbuf_e[:, :8], h_hrzn_sgn=sbuf_h[:, :4], f_score=fbuf[:, :W], e_l=e_l, f_l=f_l, rand_init_l=emb(Rl),
               rand_init_c=emb(Rc), sensor2_T_sensor1=T4, l_depth=torch.tensor(0.37), l_mask=torch.tensor(0.61),
               e_gn_abs=e_abs, h_hrzn_abs=h_abs, g_trs=g_trs)
    dec = loss_decide(inp, LOSS_CFG)
    want_xmin = torch.floor(f_idx).long() - pos_num // 2
    assert bool((dec['xmin'] == want_xmin).all()) and float(dec['xmin_margin'].min()) >= GAP_FRAC
    tie = torch.zeros(B, dtype=torch.bool)
    fs = inp['f_score']
    for b in range(B):
        inside, outside = torch.nonzero(dec['pos'][b])[:, 0], torch.nonzero(~dec['pos'][b])[:, 0]
        if harsh:                                                  # exactly 0 and exactly 1, inside and outside the window
            fs[b, inside[3]], fs[b, inside[11]] = 0.0, 1.0
            fs[b, outside[len(outside) // 3]], fs[b, outside[-1]] = 1.0, 0.0
        if len(outside) == 1:                                      # W = 31: BCE 0 like the positives, so its column alone ranks it and
            fs[b, outside[0]] = 0.0                                # the W - 1 clamp decides whether the last column is mined
        if b == B - 1 and len(outside) > neg_ratio * pos_num + 1:  # two equal scores straddling the selection boundary
            order = torch.argsort(fs[b, outside], descending=True, stable=True)
            k = neg_ratio * pos_num
            fs[b, outside[order[k]]] = fs[b, outside[order[k - 1]]]
            tie[b] = True
    dec = loss_decide(inp, LOSS_CFG)
    free = dec['select_margin'][~tie]
    assert bool((dec['select_margin'][tie] == 0).all()) and (free.numel() == 0 or float(free.min()) >= GAP_SELECT), dec['select_margin']
    for b in range(B):                                             # a tie is settled for the lower column
        if tie[b]:
            p = fs[b]
            eq = torch.nonzero((p == p[outside[order[k]]]) & ~dec['pos'][b])[:, 0]
            assert len(eq) == 2 and bool(dec['sel'][b, eq[0]]) and not bool(dec['sel'][b, eq[1]])
    assert float(dec['sign_margin'].min()) >= GAP_SIGN
    for r in (dec['rot_e'], dec['rot_h']):
        ex = r['same'] | r['opp']
        assert float(r['margin'][~ex].min()) >= GAP_BRANCH
    kinds_seen = dict(low=bool((dec['xmin'] < 0).any()), high=bool((dec['xmin'] + pos_num > W).any()))
    return dict(name='loss B=%d W=%d' % (B, W), B=B, W=W, inp=inp, dec=dec, cfg=LOSS_CFG, views2d=bool(ci % 2 == 0), harsh=harsh,
                weights=_rand(g, 11) + 0.5, tie=tie, windows=kinds, seen=kinds_seen)


def loss_cases():
    return [loss_case(B, W) for B in LOSS_B for W in LOSS_W]


def loss_family(key):
    return {'L': 'loss_entry', 'gt72': 'loss_gt'}.get(key) or 'loss_' + key


IMG_CASES = ('1x1x1', '3x5x7', '3x5x7 none valid', '2x37x53')


@_cached
def img_case(name):
    B, H, W = [int(v) for v in name.split()[0].split('x')]
    g = _gen(500 + IMG_CASES.index(name))
    depth = torch.where(_rand(g, B, H, W) < 0.45, 1 + 49 * _rand(g, B, H, W), torch.zeros(B, H, W))
    img_mask = (_rand(g, B, H, W) < 0.7).to(torch.uint8)
    if name == '1x1x1':
        depth[:], img_mask[:] = 7.5, 1
    if name == '3x5x7':
        img_mask[1] = (depth[1] <= 0).to(torch.uint8)              # one sample without a valid pixel
        depth[0, 0, :4], depth[0, 1, :4] = torch.tensor([3., 0., 4., 0.]), torch.tensor([0., 5., 0., 6.])
    if name == '3x5x7 none valid':
        img_mask[:] = 0
    gdep4 = torch.cat([_randn(g, B, H, W, 3), depth[..., None]], 3).contiguous()
    pred_mask = _sigmoid64(2 * _randn(g, B, 2, H, W))
    if name == '3x5x7':                                            # probabilities exactly 0 and 1 against both targets
        pred_mask[0, 0, 0, :4], pred_mask[0, 0, 1, :4] = torch.tensor([0., 0., 1., 1.]), torch.tensor([0., 0., 1., 1.])
    dec = gimg_decide(gdep4, img_mask)
    if name == '3x5x7':
        assert int(dec['valid'][1].sum()) == 0 and int(dec['valid'][0].sum()) > 0 and int(dec['gt_mask'][1].sum()) > 0
    if name.endswith('none valid'):
        assert int(dec['valid'].sum()) == 0
    return dict(name='img ' + name, gdep4=gdep4, img_mask=img_mask, pred_depth=depth[:, None] + _randn(g, B, 1, H, W),
                pred_mask=pred_mask, dec=dec, g=_rand(g, 2) + 0.5)


def img_cases():
    return [img_case(n) for n in IMG_CASES]


IMG_FAMILY = {'l_depth': 'img_scalar', 'l_mask': 'img_scalar', 'd_depth': 'img_grad', 'd_mask': 'img_grad'}
IMG_EXACT = ('n_valid', 'gt_depth', 'gt_mask')
RASTER_N = (1000, 16384 + 300)
RASTER_FOV = (0.3, -0.3)


@_cached
def raster_case(mode, N):
    """B = 2 with a pose per sample; N = 1000 onto 8 x 16 pixels (many points per pixel); N = 16684 takes more than 64 workgroups of
    256 points and its second sample lies entirely out of view"""
    B = 2
    H, W = (8, 16) if N == 1000 else (16, 64)
    g = _gen(600 + 10 * mode + RASTER_N.index(N))
    M = 2 * N
    hidden = N != 1000
    if mode == 0:
        pose = torch.eye(4)[None].repeat(B, 1, 1)
        pose[:, :3, :3] += 0.05 * _randn(g, B, 3, 3)
        pose[:, :3, 3] = 0.1 * _randn(g, B, 3)
        pose[:, 3, :3] = 0.01 * _randn(g, B, 3)
        yaw, pitch = (_rand(g, B, M) * 2 - 1) * 3.1, (_rand(g, B, M) * 2 - 1) * 0.4
        if hidden:
            pitch[1] = 0.7 + 0.3 * _rand(g, M)
        r = 2 + 28 * _rand(g, B, M)
        r, pitch, yaw = r.double(), pitch.double(), yaw.double()
        pc = torch.stack([r * torch.cos(pitch) * torch.cos(yaw), r * torch.cos(pitch) * torch.sin(yaw), r * torch.sin(pitch)], 1).float()
    else:
        K = torch.tensor([[W / 2., 0., W / 2., 0.], [0., W / 2., H / 2., 0.], [0., 0., 1., 0.]])
        T = torch.tensor([[0., -1., 0., 0.], [0., 0., -1., 0.], [1., 0., 0., 0.], [0., 0., 0., 1.]])
        T = T[None].repeat(B, 1, 1)
        T[:, :3, 3] = 0.2 * _randn(g, B, 3)
        T[:, :3, :3] += 0.03 * _randn(g, B, 3, 3)
        pose = torch.matmul(K[None], T).contiguous()
        x = 2 + 28 * _rand(g, B, M)
        if hidden:
            x[1] = -x[1]
        pc = torch.stack([x, x.abs() * (_rand(g, B, M) * 2.6 - 1.3), x.abs() * (_rand(g, B, M) * 0.8 - 0.4)], 1)
    pix, margin = raster_decide(pc, pose, H, W, mode, RASTER_FOV)
    keep = torch.stack([torch.nonzero(margin[b] >= GAP_PIXEL)[:N, 0] for b in range(B)])       # fails when fewer than N are left
    pc = torch.gather(pc, 2, keep[:, None, :].expand(B, 3, N)).contiguous()
    pix, margin = raster_decide(pc, pose, H, W, mode, RASTER_FOV)
    assert float(margin.min()) >= GAP_PIXEL
    seen = (pix[0] >= 0).sum()
    assert int(seen) > N // 4 and int(pix.max()) < H * W
    if hidden:
        assert int((pix[1] >= 0).sum()) == 0
    else:
        assert int((pix[1] >= 0).sum()) > N // 4 and int(seen) > 4 * len(torch.unique(pix[0]))
    return dict(name='raster mode=%d N=%d' % (mode, N), mode=mode, N=N, H=H, W=W, pc=pc, pose=pose, pix=pix,
                gimg=_randn(g, B, H, W, 4))


def raster_cases():
    return [raster_case(m, N) for m in (0, 1) for N in RASTER_N]


def raster_run(case, dtype, mut=()):
    return {'g_pose': raster_pose_grad(case['pix'], case['gimg'], case['pc'], case['pose'], case['mode'], dtype, mut),
            'gvals': raster_values_grad(case['pix'], case['gimg'])}


@_cached
def err_case(mode):
    """B = 67: identical poses (row 0), identical poses whose float32 trace rounds above 3 (row 1), a half turn (row 2)"""
    B = 67
    g = _gen(700)
    gt = _embed44(_rot_xyz((_rand(g, B, 3) - 0.5) * 3)).float()
    gt[:, :3, 3] = _randn(g, B, 3) * 5
    found = None
    for R in _rot_xyz((_rand(g, 4096, 3) - 0.5) * 3).float():
        if float((R * R).sum()) > 3.0:
            found = R
            break
    assert found is not None
    gt[1, :3, :3] = found
    pred = gt.clone()
    pred[:, :3, :3] = torch.bmm(gt[:, :3, :3].double(), _rot_xyz((_rand(g, B, 3) - 0.5) * 0.2)).float()
    pred[:, :3, 3] += _randn(g, B, 3) * 0.3
    pred[:2] = gt[:2]
    pred[2, :3, :3] = gt[2, :3, :3] * torch.tensor([1., -1., -1.])[None, :]      # gt Rx(pi): exact in float32
    return dict(name='pose errors mode=%d' % mode, mode=mode, gt=gt, pred=pred)


# the issue's one family "pose errors", split by what is computed: the trace form's acos near 1 costs 1e-4 of 180 degrees, which
# would be no bound at all for the translation errors and for the atan2 form
ERR_FAMILY = [{'rot': 'pose_err_rot_trace', 'trs': 'pose_err_trs'}, {'rot': 'pose_err_rot_quat', 'trs': 'pose_err_trs'}]


def err_run(case, dtype, mut=()):
    rot, trs = pose_errors(case['gt'].to(dtype), case['pred'].to(dtype), case['mode'])
    return {'rot': rot, 'trs': trs}


def all_cases():
    """-> [(case, run, family of an output key or None for an exact one)]"""
    out = [(c, head_run, HEAD_FAMILY.get) for c in head_cases()]
    out += [(yaw_case(n), yaw_run, {'R': 'yaw_R'}.get) for n in YAW_N]
    out += [(calib_case(k), calib_run, CALIB_FAMILY.get) for k in ('pixel', 'general')] + [(compose_case(), compose_run, CALIB_FAMILY.get)]
    out += [(c, pose_loss_run, loss_family) for c in loss_cases()]
    out += [(c, gimg_run, IMG_FAMILY.get) for c in img_cases()]
    out += [(c, raster_run, {'g_pose': 'raster_grad'}.get) for c in raster_cases()]
    out += [(err_case(m), err_run, ERR_FAMILY[m].get) for m in (0, 1)]
    return out


def reference(case, run):
    """the float64 evaluation of a case, computed once and shared"""
    key = ('ref', case['name'])
    if key not in _CACHE:
        _CACHE[key] = run(case, torch.float64)
    return _CACHE[key]


def pooled_float32_errors():
    """family -> (largest error of the float32 evaluation against the float64 one, the case)"""
    pooled = {}
    for case, run, fam in all_cases():
        ref, f32 = reference(case, run), run(case, torch.float32)
        for k, v in ref.items():
            if fam(k) is None:
                assert torch.equal(f32[k].double(), v.double()), (case['name'], k)
                continue
            e = rel_err(f32[k], v)
            if e > pooled.get(fam(k), (-1.0, ''))[0]:
                pooled[fam(k)] = (e, case['name'] + ' ' + k)
    return pooled
