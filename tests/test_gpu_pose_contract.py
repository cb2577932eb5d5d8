"""The pose heads, the yaw head, the calibration chain, the compose, the pose loss, the image terms, the raster gradients and the
pose errors (csrc/pose.hip, loss.hip, raster.hip, eval.hip) against the float64 contract of tests/pose_contract.py, at every case
of that module and under its ceilings.  Every kernel is reached through the product's own wrappers; ctypes only where a wrapper
cannot reach a path (a NULL incoming gradient of the head backward, efgh_pose_rotation_between, efgh_pose_errors with B > 1).
The contract runs on the CPU; the kernels' outputs are brought there.

Two groups of cases hold wrapper fixes in place: test_pose_loss[5-64] and [5-257] hand e_gn_abs, h_hrzn_abs and g_trs over as row
views of a wider buffer (PoseLossFn used to read them with pitch 3 / 2: every sample after the first from the wrong place), and the
test_image_terms cases above 1x1x1 hand the depth image and the image mask over as views (ops.gimg_loss_fwd / _bwd used to read
them densely).  Before those fixes exactly these five cases failed."""
import ctypes

import pytest
import torch

import pose_contract as PC

pytestmark = pytest.mark.gpu


def _hold(case, run, fam, got, exact_keys=()):
    """every output of `got` against the float64 evaluation of the case: under the ceiling of its family, or bit-equal"""
    ref = PC.reference(case, run)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    bad = []
    for k, v in got.items():
        v = v.detach().cpu()
        if fam(k) is None or k in exact_keys:
            ok = torch.equal(v.float(), ref[k].float())
            print('%-28s %-14s exact %s' % (case['name'], k, ok))
            if not ok:
                bad.append((k, 'not bit-equal'))
        if fam(k) is not None:
            e = PC.check(fam(k), case['name'] + ' ' + k, v, ref[k])
            print('%-28s %-14s %.3e (ceiling %.3e)' % (case['name'], k, e, PC.CEIL[fam(k)]))
            if not e <= PC.CEIL[fam(k)]:
                bad.append((k, e, PC.CEIL[fam(k)]))
    assert not bad, (case['name'], bad)


def _pitched(view, pad):
    """a row view with the pitch of the case's buffer; what lies behind the row is `pad`"""
    rows, n = view.shape
    buf = torch.full((rows, view.stride(0)), pad, device='cuda')
    buf[:, :n] = view.cuda()
    return buf


@pytest.mark.parametrize('regime', PC.HEAD_REGIMES)
@pytest.mark.parametrize('nd', [3, 2])
def test_head_normal(nd, regime):
    from efgh_amd import _C
    from efgh_amd.common import pose
    case = PC.head_case(nd, regime)
    B, dest, ncls = case['abuf'].shape[0], case['dest'], 1 << nd
    ab, sb = case['abuf'].cuda().requires_grad_(True), case['sbuf'].cuda()
    ga, gn, gR = case['ga'].cuda(), case['gn'].cuda(), case['gR'].cuda()
    a, n, R = pose.head_normal(ab[:, :nd], sb[:, :ncls], dest)
    assert a.shape == (B, nd, 1) and n.shape == (B, nd, 1) and R.shape == (B, 4, 4)
    ((a[:, :, 0] * ga).sum() + (n[:, :, 0] * gn).sum() + (R * gR).sum()).backward()
    assert float(ab.grad[:, nd:].abs().max()) == 0.0
    grads = []
    for present in ((ga, None, None), (None, gn, None), (None, None, gR)):
        g = torch.full((B, nd), float('nan'), device='cuda')
        x = ab.detach()
        _C.check(_C.lib().efgh_pose_head_normal_bwd(
            _C.ptr(x), ctypes.c_int64(x.stride(0)), _C.ptr(sb), ctypes.c_int64(sb.stride(0)), ctypes.c_int32(B), ctypes.c_int32(nd),
            ctypes.c_float(dest[0]), ctypes.c_float(dest[1]), ctypes.c_float(dest[2]), _C.ptr(present[0]), _C.ptr(present[1]),
            _C.ptr(present[2]), _C.ptr(g), _C.stream_ptr()))
        grads.append(g)
    grads.append(ab.grad[:, :nd])
    got = {'abs': a[:, :, 0], 'normal': n[:, :, 0], 'R': R, 'grad': torch.stack(grads)}
    _hold(case, PC.head_run, PC.HEAD_FAMILY.get, got, exact_keys=('R',) if case['exact'] else ())
    # the inference path is the same launch
    with torch.no_grad():
        a2, n2, R2 = pose.head_normal(ab[:, :nd], sb[:, :ncls], dest)
    assert torch.equal(a2, a) and torch.equal(n2, n) and torch.equal(R2, R)
    if nd == 3:             # the stand-alone rotation of unit vectors onto a constant (the loss's ground-truth poses): same contract
        v1 = n.detach()[:, :, 0].contiguous()
        Rk = torch.empty((B, 4, 4), device='cuda')
        _C.check(_C.lib().efgh_pose_rotation_between(_C.ptr(v1), ctypes.c_int32(B), ctypes.c_float(dest[0]), ctypes.c_float(dest[1]),
                                                     ctypes.c_float(dest[2]), _C.ptr(Rk), _C.stream_ptr()))
        br = PC.rot_decide(v1.cpu(), dest)
        ex = br['same'] | br['opp']
        assert bool(ex.all()) if case['exact'] else float(br['margin'][~ex].min()) >= PC.GAP_BRANCH
        want = PC.rotation_between(v1.cpu().double(), dest, br)
        e = PC.check('head_val', case['name'] + ' rotation_between', Rk, want)
        assert e <= PC.CEIL['head_val'], e
        assert not case['exact'] or torch.equal(Rk.cpu(), want.float())


@pytest.mark.parametrize('n', PC.YAW_N)
def test_yaw_head(n):
    from efgh_amd.common import pose
    case = PC.yaw_case(n)
    buf = _pitched(case['score'], 2.0)              # above every score: a read past column n - 1 would find it
    R = pose.yaw_rotation_from_scores(buf[:, :n])
    ref = PC.reference(case, PC.yaw_run)['R']
    _hold(case, PC.yaw_run, {'R': 'yaw_R'}.get, {'R': R})
    ex = case['exact']
    assert torch.equal(R.cpu()[ex], ref.float()[ex])                                        # the exact branches are bit-equal
    opp = torch.diag(torch.tensor([-1., -1., 1., -1.]))
    assert torch.equal(R[0].cpu(), opp) and torch.equal(R[1].cpu(), opp)                    # columns 0 and n - 1: "opposite"
    if n % 2:
        assert torch.equal(R[3].cpu(), torch.eye(4))                                         # column (n - 1) / 2: "same"


@pytest.mark.parametrize('kind', ['pixel', 'general'])
def test_cam_T_velo(kind):
    """backward with both gradients, only c_T and only l_T (the kernel's two NULL paths)"""
    from efgh_amd.common import pose
    case = PC.calib_case(kind)
    calib, A, g = case['calib'].cuda(), case['A'].cuda(), case['g'].cuda()
    for want_c, want_l in ((True, True), (True, False), (False, True)):
        c, l = case['c_T'].cuda().requires_grad_(want_c), case['l_T'].cuda().requires_grad_(want_l)
        out = pose.compute_cam_T_velo(c, l, calib, A)
        (out * g).sum().backward()
        ref = PC.reference(case, PC.calib_run)
        got = {'out': out, 'g_cT': c.grad if want_c else ref['g_cT'], 'g_lT': l.grad if want_l else ref['g_lT']}
        assert (c.grad is not None) == want_c and (l.grad is not None) == want_l
        _hold(case, PC.calib_run, PC.CALIB_FAMILY.get, got)
    with torch.no_grad():
        assert torch.equal(pose.compute_cam_T_velo(case['c_T'].cuda(), case['l_T'].cuda(), calib, A), out)


def test_compose():
    from efgh_amd.common import pose
    case = PC.compose_case()
    a, b = case['a'].cuda().requires_grad_(True), case['b'].cuda().requires_grad_(True)
    out = pose.compose(a, b)
    (out * case['g'].cuda()).sum().backward()
    _hold(case, PC.compose_run, PC.CALIB_FAMILY.get, {'out': out, 'g_a': a.grad, 'g_b': b.grad})


@pytest.mark.parametrize('W', PC.LOSS_W)
@pytest.mark.parametrize('B', PC.LOSS_B)
def test_pose_loss(B, W):
    """all 11 entries, all 72 ground-truth columns, both classes, the positive window, the selected set and the gradient of an
    arbitrary weighting of the entries w.r.t. every prediction.  Cases with `views2d` hand e_gn_abs, h_hrzn_abs and g_trs over as 2-D
    row views of a wider buffer (the layout the heads use for their logits)"""
    from efgh_amd.losses.efghloss import PoseLossFn
    case = PC.loss_case(B, W)
    inp, dec = case['inp'], case['dec']
    leaves, args = {}, {}
    for k in ('e_gn_abs', 'h_hrzn_abs', 'g_trs'):
        n = inp[k].shape[1]
        if case['views2d']:
            leaves[k] = torch.full((B, 32), 7.0, device='cuda')
            leaves[k][:, :n] = inp[k].cuda()
            leaves[k].requires_grad_(True)
            args[k] = leaves[k][:, :n]
            assert not args[k].is_contiguous() or B == 1
        else:
            leaves[k] = inp[k].cuda()[:, :, None].contiguous().requires_grad_(True)
            args[k] = leaves[k]
    for k in ('e_gn_sgn', 'h_hrzn_sgn', 'f_score'):
        leaves[k] = _pitched(inp[k], 0.5).requires_grad_(True)
        args[k] = leaves[k][:, :inp[k].shape[1]]
    leaves['e_l'] = args['e_l'] = inp['e_l'].cuda().requires_grad_(True)
    for k in ('l_depth', 'l_mask'):
        leaves[k] = args[k] = inp[k].cuda().requires_grad_(True)
    Lv, gtbuf, gtcls, gtfs = PoseLossFn.apply(args['e_gn_abs'], args['e_gn_sgn'], args['h_hrzn_abs'], args['h_hrzn_sgn'], args['f_score'],
                                              args['g_trs'], args['e_l'], inp['f_l'].cuda(), args['l_depth'], args['l_mask'],
                                              inp['rand_init_l'].cuda(), inp['rand_init_c'].cuda(), inp['sensor2_T_sensor1'].cuda(),
                                              case['cfg'])
    sel, nsel = Lv.grad_fn.saved_tensors[-2:]
    (Lv * case['weights'].cuda()).sum().backward()
    # exact outputs
    assert torch.equal(gtcls.cpu(), torch.stack([dec['cls_e'], dec['cls_h']], 1))
    assert torch.equal(gtfs.cpu(), dec['pos'].float())
    assert torch.equal(sel.cpu(), dec['sel'].float()), torch.nonzero(sel.cpu() != dec['sel'].float())
    assert torch.equal(nsel.cpu(), dec['n_selected'].reshape(1))
    got = {'L': Lv, 'gt72': gtbuf}
    for k in PC.LOSS_GRADS:
        g = leaves[k].grad
        n = inp[k].shape[1] if inp[k].dim() == 2 else None
        if k in ('e_gn_abs', 'h_hrzn_abs', 'g_trs'):
            g = g[:, :n] if case['views2d'] else g[:, :, 0]
            assert not case['views2d'] or float(leaves[k].grad[:, n:].abs().max()) == 0.0
        elif k in ('e_gn_sgn', 'h_hrzn_sgn', 'f_score'):
            assert float(g[:, n:].abs().max()) == 0.0
            g = g[:, :n]
        got['grad_' + k] = g
    _hold(case, PC.pose_loss_run, PC.loss_family, got)
    for m in ('e_l', 'h_c'):                            # an exactly aligned ground-truth normal: the exact-branch matrices
        a, b = PC.GT_COLS[m]
        ex = (dec['rot_e' if m == 'e_l' else 'rot_h']['same'] | dec['rot_e' if m == 'e_l' else 'rot_h']['opp'])
        assert torch.equal(gtbuf.cpu()[ex, a:b], PC.reference(case, PC.pose_loss_run)['gt72'].float()[ex, a:b])


@pytest.mark.parametrize('name', PC.IMG_CASES)
def test_image_terms(name):
    """the depth image and the image mask arrive as views (every other channel pair of a wider map, every other column of a wider
    mask): the wrappers hand the kernels dense memory"""
    from efgh_amd.nets import fn as FN
    case = PC.img_case(name)
    B, H, W, _ = case['gdep4'].shape
    wide = torch.full((B, H, W, 8), -3.0, device='cuda')
    wide[..., :4] = case['gdep4'].cuda()
    gdep4 = wide[..., :4]
    wmask = torch.ones((B, H, 2 * W), dtype=torch.uint8, device='cuda')
    wmask[:, :, ::2] = case['img_mask'].cuda()
    imask = wmask[:, :, ::2]
    pd, pm = case['pred_depth'].cuda().requires_grad_(True), case['pred_mask'].cuda().requires_grad_(True)
    ld, lm, gt_depth, gt_mask, n_valid = FN.GImageLossFn.apply(pd, pm, gdep4, imask)
    (ld * case['g'][0].cuda() + lm * case['g'][1].cuda()).backward()
    got = {'l_depth': ld, 'l_mask': lm, 'd_depth': pd.grad, 'd_mask': pm.grad, 'n_valid': n_valid, 'gt_depth': gt_depth,
           'gt_mask': gt_mask}
    _hold(case, PC.gimg_run, PC.IMG_FAMILY.get, got)
    assert float(pm.grad[:, 1].abs().max()) == 0.0 and bool(torch.isfinite(pm.grad).all())
    if name.endswith('none valid'):
        assert bool(torch.isnan(ld)) and float(pd.grad.abs().max()) == 0.0


@pytest.mark.parametrize('N', PC.RASTER_N)
@pytest.mark.parametrize('mode', [0, 1])
def test_raster_gradients(mode, N):
    from efgh_amd import ops
    case = PC.raster_case(mode, N)
    B, HW = 2, case['H'] * case['W']
    pix, gimg, pc, P = case['pix'].cuda(), case['gimg'].cuda(), case['pc'].cuda(), case['pose'].cuda()
    assert (N + 255) // 256 > 64 or N == 1000
    got = {'gvals': ops.raster_bwd(pix, gimg, B, N, HW), 'g_pose': ops.raster_pose_bwd(pix, gimg, pc, P if mode == 0 else None, B, N, HW, mode)}
    _hold(case, PC.raster_run, {'g_pose': 'raster_grad'}.get, got)
    # the product's rasteriser places the points where the reference's rule does (every point is GAP_PIXEL away from a boundary)
    if mode == 0:
        _, pix_k = ops.range_image(pc, P, case['H'], case['W'], *PC.RASTER_FOV)
    else:
        _, pix_k = ops.depth_image(pc, P, case['H'], case['W'])
    assert torch.equal(pix_k.cpu(), case['pix'])


@pytest.mark.parametrize('mode', [0, 1])
def test_pose_errors(mode):
    from efgh_amd import _C
    from efgh_amd.common.metrics import Err
    case = PC.err_case(mode)
    gt, pred = case['gt'].cuda(), case['pred'].cuda()
    B = gt.shape[0]
    rot, trs = torch.empty(B, device='cuda'), torch.empty(B, device='cuda')
    _C.check(_C.lib().efgh_pose_errors(_C.ptr(gt), _C.ptr(pred), ctypes.c_int32(B), ctypes.c_int32(mode), _C.ptr(rot), _C.ptr(trs),
                                       _C.stream_ptr()))
    _hold(case, PC.err_run, PC.ERR_FAMILY[mode].get, {'rot': rot, 'trs': trs})
    assert float(trs[0]) == 0.0 and float(trs[1]) == 0.0
    meter = Err('KITTI_RAW' if mode == 1 else 'KITTI_ODOM')
    assert meter.mode == mode
    for b in (5, 2):                                    # the meter takes sample 0 of what it is handed
        meter.update({'sensor2_T_sensor1': gt[b:]}, {'sensor2_T_sensor1': pred[b:]})
    d = meter.error_dict
    assert d['rot'] == [float(rot[5]), float(rot[2])] and d['trs'] == [float(trs[5]), float(trs[2])]


def test_zz_every_family_was_measured():
    """runs last in this module: the largest kernel error of every family (the figures next to the constants of pose_contract.py)"""
    for fam, (e, label) in sorted(PC.OBSERVED.items()):
        print('%-22s ceiling %.3e  observed %.3e  (%s)' % (fam, PC.CEIL[fam], e, label))
        assert e <= PC.CEIL[fam]
