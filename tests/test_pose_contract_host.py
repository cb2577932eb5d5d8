"""tests/pose_contract.py proved on the CPU: (1) its float64 evaluation equals independent float64 torch autograd of the reference
expressions in the per-sample loop forms of oracle/efgh_oracle.py, lifted to double where those force float, at every case;
(2) every ceiling lies between 1 x and 4 x the float32-vs-float64 error it was measured from; (3) every deliberate misreading of
the reference (pose_contract.MUTATIONS) leaves a ceiling at some element of some case, which is what makes the comparison of
tests/test_gpu_pose_contract.py mean something.

The loop forms branch where the reference branches (`if (1 - c) == 0`, `int(f_idx)`, `argmax`, `sort`) on their own float64
values rounded to float32, the precision the reference decides at: the cases keep every such value a stated gap away from
flipping, or make it exact, so both readings decide alike."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pose_contract as PC

F64 = torch.float64
TOL = 1e-9                   # two float64 evaluations of one expression in different orders


def _close(case, got, ref, tol=TOL):
    assert set(got) == set(ref)
    for k in got:
        e = PC.rel_err(got[k], ref[k])
        assert e <= tol, (case['name'], k, e)


# ---------------------------------------------------------------------------------------------------------------- loop forms
def _f32(x):
    return x.detach().float()


def ref_rotation_between(v1, v2):
    """one sample; K from detached scalars, (1 - c) / s^2 attached; the exact branches as the reference's -eye(4) / eye(4)"""
    v = torch.linalg.cross(v1, v2)
    c = torch.dot(v1, v2)
    s = torch.sqrt(torch.sum(v ** 2))
    vd = v.detach()
    K = torch.tensor([[0, -vd[2], vd[1]], [vd[2], 0, -vd[0]], [-vd[1], vd[0], 0]], dtype=F64)
    if (1 - _f32(c)) == 0:
        return torch.eye(4, dtype=F64)
    if (1 + _f32(c)) == 0:
        R = -torch.eye(4, dtype=F64)
        if _f32(v1[0]).item() == 0.0 and v2[0].item() == 0.0:
            R[0, 0] = 1
        elif _f32(v1[2]).item() == 0.0 and v2[2].item() == 0.0:
            R[2, 2] = 1
        return R
    R = torch.zeros(4, 4, dtype=F64)
    R[3, 3] = 1
    R[:3, :3] = torch.eye(3, dtype=F64) + K + torch.mm(K, K) * ((1 - c) / (s ** 2))
    return R


def ref_head(case):
    nd, B = case['nd'], case['abuf'].shape[0]
    x = case['abuf'][:, :nd].double().clone().requires_grad_(True)
    dest = torch.tensor(case['dest'], dtype=F64)
    a_, n_, R_ = [], [], []
    for b in range(B):
        a = torch.softmax(x[b], 0)
        a = a / torch.sqrt(torch.sum(a ** 2))
        cls = int(torch.argmax(torch.softmax(case['sbuf'][b, :1 << nd], 0)).item())
        sgn = torch.tensor([1.0 if (cls >> (nd - 1 - i)) & 1 else -1.0 for i in range(nd)], dtype=F64)
        n = a * sgn
        n3 = n if nd == 3 else torch.cat([n, torch.zeros(1, dtype=F64)])
        a_.append(a)
        n_.append(n)
        R_.append(ref_rotation_between(n3, dest))
    a, n, R = torch.stack(a_), torch.stack(n_), torch.stack(R_)
    terms = {'abs': (a * case['ga'].double()).sum(), 'normal': (n * case['gn'].double()).sum(), 'R': (R * case['gR'].double()).sum()}
    terms['all'] = sum(terms.values())
    grads = []
    for k in PC.HEAD_GRADS:
        g = torch.autograd.grad(terms[k], x, retain_graph=True, allow_unused=True)[0] if terms[k].requires_grad else None
        grads.append(torch.zeros_like(x) if g is None else g)
    return {'abs': a.detach(), 'normal': n.detach(), 'R': R.detach(), 'grad': torch.stack(grads)}


def ref_yaw(case):
    out = []
    n = case['n']
    for b in range(case['score'].shape[0]):
        sc = case['score'][b:b + 1]
        f_idx = torch.argmax(sc, dim=1, keepdim=True).float()
        f_rad = -(f_idx / (n - 1)) * 2 * math.pi + math.pi
        rad = f_rad[0]
        f_fwd = torch.tensor([math.cos(rad), math.sin(rad), 0.])                  # float32, as the reference builds it
        out.append(ref_rotation_between(f_fwd.double(), torch.tensor([1., 0., 0.], dtype=F64)))
    return {'R': torch.stack(out)}


def ref_calib(case):
    c, l = case['c_T'].double().requires_grad_(True), case['l_T'].double().requires_grad_(True)
    A = case['A'].double()
    m = torch.bmm(case['calib'].double(), l)
    m = torch.bmm(A, m)
    m = torch.bmm(c, m)
    out = torch.bmm(torch.inverse(A), m)
    (out * case['g'].double()).sum().backward()
    return {'out': out.detach(), 'g_cT': c.grad, 'g_lT': l.grad}


def ref_compose(case):
    a, b, g = case['a'].double(), case['b'].double(), case['g'].double()
    return {'out': torch.einsum('nij,njk->nik', a, b), 'g_a': torch.einsum('nik,njk->nij', g, b), 'g_b': torch.einsum('nki,nkj->nij', a, g)}


def _ref_abs_sign(pred_abs, pred_sgn, gt_vec, nd):
    gt_abs = torch.abs(gt_vec)[:, :nd, :]
    s = torch.sign(gt_vec)
    s = torch.where(s == -1, torch.zeros_like(s), s)
    cls = []
    for b in range(s.size(0)):
        c = 0
        for i in range(nd):
            c = c + s[b, i, 0] * (2 ** (nd - 1 - i))
        cls.append(c.long()[None])
    cls = torch.cat(cls, 0)
    cos = F.cosine_similarity(pred_abs, gt_abs, dim=1)
    return torch.mean(1 - cos) * 10.0, F.cross_entropy(pred_sgn, cls) * 1.0, gt_abs, cls


def _ref_gt_fov(axis, width, positive_num):
    zz = torch.zeros((axis.size(0), width), dtype=F64)
    for b in range(axis.size(0)):
        yaw = torch.atan2(axis[b, 1, 0], axis[b, 0, 0]).detach()
        f_idx = ((-yaw + math.pi) / (2 * math.pi)) * width
        xmin = int(f_idx) - int(positive_num / 2)
        xmax = xmin + positive_num
        if xmin >= 0 and xmax < width:
            zz[b, xmin:xmax] = 1
        elif xmin < 0:
            zz[b, 0:xmax] = 1
            zz[b, xmin:] = 1
        else:
            zz[b, xmin:] = 1
            zz[b, 0:xmax - width] = 1
    return zz


def ref_pose_loss(case):
    lam, pos_num, neg_ratio = case['cfg']
    x = {k: v.double().clone() for k, v in case['inp'].items()}
    for k in PC.LOSS_GRADS:
        x[k].requires_grad_(True)
    B, W = x['f_score'].shape
    col = lambda v: torch.tensor(v, dtype=F64)[None, :, None]
    e1, e2, e3 = col([1., 0., 0.]), col([0., 1., 0.]), col([0., 0., 1.])
    rot = lambda g, e: torch.stack([ref_rotation_between(g[b, :, 0], e[0, :, 0]) for b in range(B)])
    L, gt = {}, {}
    g = torch.bmm(x['rand_init_l'][:, :3, :3], e3.expand(B, -1, -1))
    g = g / torch.sqrt(torch.sum(g ** 2, 1, keepdim=True))
    gt['e_gn'], gt['e_l'] = g, rot(g, e3)
    la, ls, gt['e_gn_abs'], cls_e = _ref_abs_sign(x['e_gn_abs'][:, :, None], x['e_gn_sgn'], g, 3)
    L['e_gn'], L['e_gn_abs'], L['e_gn_sgn'] = (la + ls) * lam['e_gn'], la * lam['e_gn'], ls * lam['e_gn']
    g = torch.bmm(x['rand_init_c'][:, :3, :3], e2.expand(B, -1, -1))
    g = g / torch.sqrt(torch.sum(g ** 2, 1, keepdim=True))
    gt['h_hrzn'], gt['h_c'] = g, rot(g, e2)[:, :3, :3]
    la, ls, gt['h_hrzn_abs'], cls_h = _ref_abs_sign(x['h_hrzn_abs'][:, :, None], x['h_hrzn_sgn'], g, 2)
    L['h_hrzn'], L['h_hrzn_abs'], L['h_hrzn_sgn'] = (la + ls) * lam['h_hrzn'], la * lam['h_hrzn'], ls * lam['h_hrzn']
    T4 = x['sensor2_T_sensor1']
    Tinv = torch.inverse(T4[:, :3, :3])
    pe = x['e_l'][:, :3, :3].clone().detach()
    axis = torch.bmm(torch.bmm(pe, Tinv), e1.expand(B, -1, -1))
    gt_fs = _ref_gt_fov(axis, W, pos_num)
    ge = gt['e_l'][:, :3, :3].clone().detach()
    fl = torch.zeros((B, 4, 4), dtype=F64)
    fl[:, :3, :3] = torch.inverse(torch.bmm(ge, Tinv))
    fl[:, 3, 3] = 1
    gt['f_l'] = fl
    pos = gt_fs > 0
    lc = F.binary_cross_entropy(x['f_score'], gt_fs, reduction='none').detach().clone()
    lc[pos] = 0
    _, idx = lc.sort(dim=1, descending=True, stable=True)     # among equals the lower column first
    _, rank = idx.sort(1)
    num_pos = pos.long().sum(1, keepdim=True)
    num_neg = torch.clamp(neg_ratio * num_pos, max=pos.size(1) - 1)
    wsel = pos | (rank < num_neg.expand_as(rank))
    L['fov'] = torch.mean(F.binary_cross_entropy(x['f_score'][wsel], gt_fs[wsel], reduction='none')) * lam['fov']
    origin = col([0., 0., 0., 1.]).expand(B, -1, -1)
    gt['g_trs'] = torch.bmm(torch.bmm(T4, torch.inverse(torch.bmm(x['f_l'], x['e_l']))), origin)[:, :3, :]
    gcp = torch.bmm(torch.bmm(T4, torch.inverse(torch.bmm(gt['f_l'], gt['e_l']))), origin)
    g_l = torch.eye(4, dtype=F64)[None].repeat(B, 1, 1)
    g_l[:, :3, 3] = gcp[:, :3, 0].detach()
    gt['g_l'] = g_l
    L['g_trs'] = F.smooth_l1_loss(gt['g_trs'], x['g_trs'][:, :, None]) * lam['g_trs']
    L['g_depth'] = x['l_depth'] * lam['g_depth']
    L['g_mask'] = (x['l_mask'] * lam['g_mask']) * lam['g_depth']
    total = 0
    for k in L:
        total = total + L[k]
    L['total'] = total
    Lv = torch.stack([L[k] for k in PC.LOSS_NAME])
    (Lv * case['weights'].double()).sum().backward()
    gt72 = torch.zeros((B, 72), dtype=F64)
    for k, (a, b) in PC.GT_COLS.items():
        v = gt[k].detach().reshape(B, -1)
        gt72[:, a:a + v.shape[1]] = v
    out = {'L': Lv.detach(), 'gt72': gt72}
    for k in PC.LOSS_GRADS:
        out['grad_' + k] = torch.zeros_like(x[k]) if x[k].grad is None else x[k].grad
    return out, dict(cls_e=cls_e, cls_h=cls_h, pos=pos, sel=wsel)


def ref_gimg(case):
    B = case['pred_depth'].shape[0]
    pd, pm = case['pred_depth'].double().requires_grad_(True), case['pred_mask'].double().requires_grad_(True)
    g_depth = case['gdep4'][..., 3][:, None].double()
    g_mask = (g_depth > 0).double()
    valid = (g_depth > 0) & (case['img_mask'][:, None] > 0)
    l_dep = ((g_depth - pd)[valid] ** 2).mean()
    l_msk = F.binary_cross_entropy(pm[:, 0].reshape(B, -1), g_mask.view(B, -1))
    gd = torch.autograd.grad(l_dep * case['g'][0].double(), pd, allow_unused=True)[0]
    gm, = torch.autograd.grad(l_msk * case['g'][1].double(), pm)
    return {'l_depth': l_dep.detach(), 'l_mask': l_msk.detach(), 'd_depth': torch.zeros_like(pd) if gd is None else gd, 'd_mask': gm,
            'n_valid': valid.sum().float(), 'gt_depth': g_depth.float(), 'gt_mask': g_mask.float()}


def ref_raster(case):
    """the gradient of the reference's `index_put` image, whichever point wins a pixel, by torch's own index_put autograd"""
    B, N = case['pix'].shape
    HW = case['H'] * case['W']
    pose = case['pose'].double().requires_grad_(True)
    p1 = torch.cat([case['pc'].double(), torch.ones((B, 1, N), dtype=F64)], 1)
    q = torch.bmm(pose, p1)
    if case['mode'] == 0:
        vals = torch.cat([q[:, :3], torch.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2 + q[:, 2] ** 2 + q[:, 3] ** 2)[:, None]], 1)
    else:
        vals = torch.cat([p1[:, :3], q[:, 2:3]], 1)
    vals = vals.transpose(1, 2)
    vals.retain_grad()
    b, n = torch.nonzero(case['pix'] >= 0, as_tuple=True)
    img = torch.zeros((B, HW, 4), dtype=F64).index_put((b, case['pix'][b, n].long()), vals[b, n])
    (img * case['gimg'].double().reshape(B, HW, 4)).sum().backward()
    return {'g_pose': pose.grad.reshape(B, -1), 'gvals': vals.grad.float()}


def ref_errors(case):
    from scipy.spatial.transform import Rotation
    gt, pred = case['gt'].double().numpy(), case['pred'].double().numpy()
    rot, trs = [], []
    for g, p in zip(gt, pred):
        if case['mode'] == 0:
            t = np.clip((np.trace(p[:3, :3].T.dot(g[:3, :3])) - 1) / 2, -1.0, 1.0)
            rot.append(180 * np.arccos(t) / np.pi)
            trs.append(np.linalg.norm(p[:3, 3] - g[:3, 3]))
        else:
            q = (Rotation.from_matrix(g[:3, :3]) * Rotation.from_matrix(p[:3, :3]).inv()).as_quat()       # x, y, z, w
            rot.append(2 * np.arctan2(np.linalg.norm(q[:3]), abs(q[3])) * (180 / np.pi))
            trs.append(np.mean(np.fabs(g[:3, 3] - p[:3, 3])))
    return {'rot': torch.tensor(rot), 'trs': torch.tensor(trs)}


# ---------------------------------------------------------------------------------------------------------------- (1) the contract
@pytest.mark.parametrize('nd', [3, 2])
@pytest.mark.parametrize('regime', PC.HEAD_REGIMES)
def test_heads_equal_the_loop_form(nd, regime):
    case = PC.head_case(nd, regime)
    _close(case, PC.reference(case, PC.head_run), ref_head(case))


@pytest.mark.parametrize('n', PC.YAW_N)
def test_yaw_equals_the_loop_form(n):
    case = PC.yaw_case(n)
    _close(case, PC.reference(case, PC.yaw_run), ref_yaw(case))
    idx = case['dec']['idx']
    assert int(idx[0]) == 0 and int(idx[1]) == n - 1                            # both ends are reached, and give "opposite"


def test_calibration_and_compose_equal_the_reference_expressions():
    for kind in ('pixel', 'general'):
        case = PC.calib_case(kind)
        _close(case, PC.reference(case, PC.calib_run), ref_calib(case))
    case = PC.compose_case()
    _close(case, PC.reference(case, PC.compose_run), ref_compose(case))


@pytest.mark.parametrize('W', PC.LOSS_W)
@pytest.mark.parametrize('B', PC.LOSS_B)
def test_pose_loss_equals_the_loop_form(B, W):
    case = PC.loss_case(B, W)
    ref, d = ref_pose_loss(case)
    _close(case, PC.reference(case, PC.pose_loss_run), ref, tol=1e-8)
    dec = case['dec']
    assert torch.equal(d['cls_e'], dec['cls_e']) and torch.equal(d['cls_h'], dec['cls_h'])
    assert torch.equal(d['pos'], dec['pos']) and torch.equal(d['sel'], dec['sel'])
    assert float(dec['n_selected']) == float(d['sel'].sum())


def test_pose_loss_cases_reach_what_they_are_for():
    cases = PC.loss_cases()
    kinds = set(k for c in cases for k in c['windows'])
    assert kinds == {'wrap_low', 'wrap_high', 'ends_at_W', 'middle'}
    for c in cases:
        dec, W, pos_num = c['dec'], c['W'], c['cfg'][1]
        for b, k in enumerate(c['windows']):
            x = int(dec['xmin'][b])
            assert {'wrap_low': x < 0, 'wrap_high': x + pos_num > W, 'ends_at_W': x + pos_num == W, 'middle': x >= 0 and x + pos_num < W}[k]
        assert int(dec['pos'].sum()) == c['B'] * pos_num
    assert any(c['tie'].any() for c in cases if c['W'] > 256) and any(c['views2d'] and c['B'] > 1 for c in cases)
    c = PC.loss_case(5, 31)                                 # the W - 1 clamp leaves the last column out where the window ends before it
    assert sorted(c['dec']['sel'].sum(1).tolist()) == [30, 30, 31, 31, 31]
    c = PC.loss_case(5, 257)
    p, pos = c['inp']['f_score'], c['dec']['pos']
    for v in (0.0, 1.0):
        assert bool(((p == v) & pos).any()) and bool(((p == v) & ~pos).any())
    assert float(c['inp']['e_gn_abs'][-1].abs().max()) == 0.0 and bool(c['dec']['rot_e']['same'][1])
    assert float(c['inp']['rand_init_l'][0, 0, 2]) == 0.0


@pytest.mark.parametrize('name', PC.IMG_CASES)
def test_image_terms_equal_the_reference_expressions(name):
    case = PC.img_case(name)
    got = PC.reference(case, PC.gimg_run)
    _close(case, got, ref_gimg(case))
    if name.endswith('none valid'):
        assert bool(torch.isnan(got['l_depth'])) and float(got['d_depth'].abs().max()) == 0.0 and bool(torch.isfinite(got['d_mask']).all())


@pytest.mark.parametrize('N', PC.RASTER_N)
@pytest.mark.parametrize('mode', [0, 1])
def test_raster_gradients_equal_index_put_autograd(mode, N):
    case = PC.raster_case(mode, N)
    _close(case, PC.reference(case, PC.raster_run), ref_raster(case))


@pytest.mark.parametrize('mode', [0, 1])
def test_pose_errors_equal_the_numpy_form(mode):
    case = PC.err_case(mode)
    # scipy re-orthonormalises the float32 rotation matrices it is handed: 1e-7 rad of 180 degrees
    _close(case, PC.reference(case, PC.err_run), ref_errors(case), tol=1e-12 if mode == 0 else 1e-8)


# ---------------------------------------------------------------------------------------------------------------- (2) the ceilings
def test_every_ceiling_is_between_one_and_four_times_its_measurement():
    pooled = PC.pooled_float32_errors()
    assert set(pooled) == set(PC.CEIL)
    for fam, c in PC.CEIL.items():
        e, label = pooled[fam]
        print('%-22s ceiling %.3e  float32 %.3e  x%.2f  (%s)' % (fam, c, e, c / e, label))
        assert e > 0 and e <= c <= 4 * e, (fam, c, e, label)


# ---------------------------------------------------------------------------------------------------------------- (3) the mutations
def _leaves_a_ceiling(mut, triples):
    for case, run, fam in triples:
        ref, got = PC.reference(case, run), run(case, F64, (mut,))
        for k in ref:
            if fam(k) is None:
                if not torch.equal(got[k].double(), ref[k].double()):
                    return case['name'], k, 'not equal'
            elif not PC.rel_err(got[k], ref[k]) <= PC.CEIL[fam(k)]:
                return case['name'], k, PC.rel_err(got[k], ref[k])
    return None


GROUPS = {
    'head': lambda: [(c, PC.head_run, PC.HEAD_FAMILY.get) for c in PC.head_cases()],
    'yaw': lambda: [(PC.yaw_case(n), PC.yaw_run, {'R': 'yaw_R'}.get) for n in PC.YAW_N],
    'loss': lambda: [(c, PC.pose_loss_run, PC.loss_family) for c in PC.loss_cases()],
    'img': lambda: [(c, PC.gimg_run, PC.IMG_FAMILY.get) for c in PC.img_cases()],
    'raster': lambda: [(c, PC.raster_run, {'g_pose': 'raster_grad'}.get) for c in PC.raster_cases()],
}
WHERE = {'k_attached': ['head'], 'r33_kept': ['head', 'yaw'], 'fix_swapped': ['head'], 'lsb_first': ['head'], 'last_max': ['head', 'yaw'],
         'yaw_div_n': ['yaw'], 'no_cos_clamp': ['loss'], 'total_once': ['loss'], 'mask_once': ['loss'], 'gtrs_detached': ['loss'],
         'no_wrap': ['loss'], 'window_off_one': ['loss'], 'neg_unclamped': ['loss'], 'ties_high_first': ['loss'],
         'no_bce_clamp': ['loss', 'img'], 'depth_ignores_mask': ['img'], 'mask_over_valid': ['img'], 'winner_only': ['raster'],
         'range_without_w': ['raster'], 'rank_in_chunk': ['loss']}


@pytest.mark.parametrize('mut', PC.MUTATIONS)
def test_every_misreading_leaves_a_ceiling(mut):
    assert set(WHERE) == set(PC.MUTATIONS)
    for group in WHERE[mut]:                                 # in every group it is listed for: e.g. last_max in the sign class AND the yaw
        found = _leaves_a_ceiling(mut, GROUPS[group]())
        print(mut, group, found)
        assert found is not None, (mut, group)


def test_the_unmutated_contract_stays_under_every_ceiling():
    """the mutation test's own control: with no mutation nothing is found"""
    for group in GROUPS.values():
        for case, run, fam in group():
            got, ref = run(case, F64), PC.reference(case, run)
            for k in ref:
                assert PC.rel_err(got[k], ref[k]) == 0.0, (case['name'], k)
