"""Multi-sweep accumulation on the GPU (SweepSet / preproc_pcd over efgh_prep_sweeps_*, csrc/prep.hip) against what the
unmodified reference loaders returned (tests/golden/sweeps.npz): the kept rows and their order exactly, the float64 values
inside the bound derived in tests/sweeps_contract.py, float32 = float32(float64) bit for bit."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import sweeps_contract as SC

pytestmark = pytest.mark.gpu

CASES = ('odomA', 'odomA/stride3', 'odomB', 'odomC', 'rellisA', 'rawA', 'nuscA', 'nuscB', 'nuscA/stride4')


@pytest.fixture(scope='module')
def fx(golden_dir):
    from efgh_amd.data import preproc_gt
    G, cases = SC.load_cases(golden_dir)
    for c in cases.values():                                     # the float64 restatement and its bound, once
        c['T'] = preproc_gt(*c['rand_init'])['rand_init_l']
        c['contract'] = SC.chain_of(c, c['T'])
    return G, cases


def _sweeps(c, variant):
    if variant == 'stride3':
        return [np.ascontiguousarray(s[:, :3]) for s in c['sweeps']]
    if variant == 'stride4':
        return [np.concatenate([s, np.full((s.shape[0], 1), 0.5, np.float32)], axis=1) for s in c['sweeps']]
    return c['sweeps']


def _set(c, variant=None, tensors=False):
    from efgh_amd.data import SweepSet
    sweeps = _sweeps(c, variant)
    if tensors:
        sweeps = [torch.from_numpy(s).cuda() for s in sweeps]
    return SweepSet(sweeps, c['transforms'], own_order=c['own_order'], ego_box=c['ego_box'])


def _run(c, ss):
    from efgh_amd.data import preproc_pcd
    return preproc_pcd(ss, {'rand_init_l': c['T']}, c['num_points'], c['lidar_line'], sampled_indices=c['sampled'],
                       flip_xy=c['flip_xy'], want_float64=True)


@pytest.mark.parametrize('case', CASES)
def test_selection_order_and_values(fx, case):
    name, _, variant = case.partition('/')
    c = fx[1][name]
    ss = _set(c, variant or None)
    keep = ss.kept_indices(lidar_line=c['lidar_line'], flip_xy=c['flip_xy']).cpu().numpy()
    assert keep.dtype == np.int32 and np.array_equal(keep, c['keep'])                # the reference's rows, in its order
    out32, out64 = _run(c, ss)
    got = out64.cpu().numpy()
    assert got.shape == c['out_pc'].shape
    assert SC.within(got, c['out_pc'], c['contract']['bound'])
    assert np.array_equal(out32.cpu().numpy().view(np.int32), got.astype(np.float32).view(np.int32))
    if c['keep'].size < c['num_points']:                                             # the zero-pad tail: T . (0, 0, 0, 1)
        assert np.array_equal(got[:, c['keep'].size:], np.broadcast_to(c['T'][:3, 3:4], (3, c['num_points'] - c['keep'].size)))


@pytest.mark.parametrize('case', ('odomA', 'odomA/stride3', 'rellisA', 'nuscA', 'nuscB'))
def test_accumulated_cloud(fx, case):
    name, _, variant = case.partition('/')
    c = fx[1][name]
    acc = _set(c, variant or None).accumulated()
    assert acc.dtype == torch.float64 and acc.is_cuda
    got, ref = acc.cpu().numpy(), np.asarray(c['acc'], np.float64)
    assert got.shape == ref.shape
    assert SC.within(got, ref, c['contract']['acc_bound'])
    n_own = int(SC.positions(c['sweeps'][:1], [], None, c['ego_box'])[2].sum())
    assert np.array_equal(got[:n_own].view(np.int64), ref[:n_own].view(np.int64))    # the own sweep untouched: NaN and -0.0 survive
    if name == 'odomA':
        assert np.isnan(got[:n_own]).any() and (np.signbit(got[:n_own]) & (got[:n_own] == 0)).any()


def test_one_identity_sweep_equals_the_plain_array_path(fx):
    """K = 1 with identity against today's kernels on the same [n, 4] array, bit for bit: with and without sub-sampling,
    with the RELLIS flip, with the lidar-line reduction"""
    from efgh_amd.data import SweepSet, preproc_pcd
    c = fx[1]['odomA']
    own = c['sweeps'][0]                                                             # 257 rows, boundary points, NaN, -0.0
    gts = {'rand_init_l': c['T']}
    rng = np.random.default_rng(3)
    for npts, ll, flip in ((512, None, False), (100, None, True), (64, 16, False)):
        n_keep = int(SweepSet([own]).kept_indices(lidar_line=ll, flip_xy=flip).numel())
        sel = rng.permutation(n_keep)[:npts] if npts < n_keep else None
        a32, a64 = preproc_pcd(own, gts, npts, ll, sampled_indices=sel, flip_xy=flip, want_float64=True)
        b32, b64 = preproc_pcd(SweepSet([own]), gts, npts, ll, sampled_indices=sel, flip_xy=flip, want_float64=True)
        assert torch.equal(a64.view(torch.int64), b64.view(torch.int64)) and torch.equal(a32.view(torch.int32), b32.view(torch.int32))
        c32 = preproc_pcd(np.ascontiguousarray(own[:, :3]), gts, npts, ll, sampled_indices=sel, flip_xy=flip)    # [n, 3] rows
        assert torch.equal(a32.view(torch.int32), c32.view(torch.int32))


def test_two_runs_give_identical_bits(fx):
    c = fx[1]['odomA']
    runs = []
    for tensors in (False, True, False):                          # host arrays and device tensors stage the same bytes
        ss = _set(c, tensors=tensors)
        o32, o64 = _run(c, ss)
        runs.append((o32.cpu().numpy().view(np.int32), o64.cpu().numpy().view(np.int64),
                     ss.kept_indices().cpu().numpy(), ss.accumulated().cpu().numpy().view(np.int64)))
    for r in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], r))


def _check_tuple(G, c, got, tag):
    pc, img, calib, A, gts, fname = got
    name = c['name']
    assert fname == tag and pc.is_cuda and img.is_cuda and pc.dtype == torch.float32
    assert torch.equal(img.cpu(), torch.from_numpy(G[name + '.out.img'])), name
    for k in ('img_raw', 'img_rot', 'img_mask'):
        assert np.array_equal(gts[k].cpu().numpy(), G[name + '.gt.' + k]), (name, k)
    ref = c['out_pc']
    p = pc.cpu().numpy()
    assert p.shape == ref.shape
    # float32(v) with |v - ref| <= bound: off by the bound plus half a float32 spacing at the most
    half = 0.5 * np.maximum(np.spacing(np.abs(ref).astype(np.float32)), np.spacing(np.abs(p))).astype(np.float64)
    assert (np.abs(p.astype(np.float64) - ref) <= c['contract']['bound'] + half).all(), name
    assert np.allclose(calib, G[name + '.out.calib'], rtol=0, atol=1e-12) and np.shape(calib) == G[name + '.out.calib'].shape
    assert np.array_equal(A, G[name + '.out.A'])
    for k in ('rand_init_l', 'rand_init_c', 'sensor2_T_sensor1', 'intrinsic_sensor2', 'cam_T_velo'):
        assert np.allclose(gts[k], G[name + '.gt.' + k], rtol=0, atol=1e-12), (name, k)


def test_process_classes_equal_the_recorded_tuples(fx):
    from efgh_amd.data import ProcessKITTIODOM, ProcessKITTIRAW, ProcessNUSC, ProcessRELLIS, SweepSet
    G, cases = fx

    def args(c, raw, line=True):
        a = {'raw_cam_img_size': raw, 'num_points': c['num_points'], 'test': True}
        if line:
            a['lidar_line'] = c['lidar_line']
        return a

    c = cases['odomA']
    got = ProcessKITTIODOM(args(c, [12, 24]))(_set(c), G['odomA.img'], {'P2': G['P2'], 'Tr': G['Tr']}, G['pose_ji'], 'odomA',
                                              rand_init=c['rand_init'], sampled_indices=c['sampled'])
    _check_tuple(G, c, got, 'odomA')
    c = cases['rellisA']
    got = ProcessRELLIS(args(c, [14, 26]))(_set(c), G['rellisA.img'], {'P': G['P2'], 'Tr': G['Tr']}, G['pose_ji'], 'rellisA',
                                           rand_init=c['rand_init'], sampled_indices=c['sampled'])
    _check_tuple(G, c, got, 'rellisA')
    c = cases['rawA']
    cal = types.SimpleNamespace(T_cam2_velo=G['rawA.T_cam2_velo'], T_cam3_velo=G['rawA.T_cam3_velo'])
    for pcd in (G['rawA.pcd'], SweepSet([G['rawA.pcd']])):                           # the reader's [n, 3] rows, and a set of one
        got = ProcessKITTIRAW(args(c, [12, 24]))(pcd, G['rawA.img'], cal, 'image_03', 'rawA', rand_init=c['rand_init'],
                                                 sampled_indices=c['sampled'])
        _check_tuple(G, c, got, 'rawA')
        assert got[2].shape == (3, 4)
    with pytest.raises(ValueError):
        ProcessKITTIRAW(args(c, [12, 24]))(G['rawA.pcd'], G['rawA.img'], cal, 'image_00', 'rawA', rand_init=c['rand_init'])
    for name, pcd in (('nuscA', _set(cases['nuscA'])), ('nuscB', _set(cases['nuscB'])), ('nuscB', G['nuscB.acc'])):
        c = cases[name]                                                              # nuscB.acc: the own sweep the loader hands over
        cal = {'T_cam_velo': G[name + '.T_cam_velo'], 'posej_T_posei': G['pose_ji']}
        got = ProcessNUSC(args(c, [12, 24], line=False))(pcd, G[name + '.img'], cal, name, rand_init=c['rand_init'],
                                                         sampled_indices=c['sampled'])
        _check_tuple(G, c, got, name)


def test_refusals(fx):
    from efgh_amd import _C
    from efgh_amd._C import EfghError
    from efgh_amd.data import SweepSet, preproc_pcd
    c = fx[1]['rawA']
    gts = {'rand_init_l': c['T']}
    p3, I = c['sweeps'][0], np.eye(4)
    with pytest.raises(EfghError):
        SweepSet([p3] * 65, [I] * 64)
    with pytest.raises(EfghError):
        SweepSet([np.zeros((0, 3), np.float32), p3], [I])
    with pytest.raises(EfghError):                                                   # a CPU tensor: there is no CPU path
        preproc_pcd(SweepSet([torch.from_numpy(p3)]), gts, 64, device='cpu')
    with pytest.raises(EfghError):
        SweepSet([p3]).accumulated(device='cpu')
    # the library's own checks: K = 65 and n_total = 2^29 are EFGH_E_INVALID with a message, nothing is launched
    ss = SweepSet([p3])
    pts, a = ss._args('cuda')
    keep = torch.zeros(p3.shape[0], dtype=torch.int32, device='cuda')
    out = torch.zeros((p3.shape[0], 3), dtype=torch.float64, device='cuda')
    L = _C.lib()
    for K, n_total, word in ((65, ss.n_total, 'K = 65'), (0, ss.n_total, 'K = 0'), (1, 1 << 29, 'n_total'), (1, 0, 'n_total')):
        bad = a[:5] + (ctypes.c_int32(K), ctypes.c_int32(n_total))
        rc = L.efgh_prep_sweeps_materialize(*bad, _C.ptr(keep), ctypes.c_int32(p3.shape[0]), _C.ptr(out), _C.stream_ptr())
        assert rc == -1 and word in L.efgh_last_error().decode()
        with pytest.raises(EfghError):
            _C.check(L.efgh_prep_sweeps_filter(*bad, None, ctypes.c_int32(p3.shape[0]), ctypes.c_int32(0), ctypes.c_double(50.),
                                               ctypes.c_float(0), ctypes.c_float(0), _C.ptr(keep), _C.ptr(keep), _C.ptr(keep),
                                               _C.stream_ptr()))
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0


def test_more_blocks_than_one_scan_pass():
    """3 x 30k points: more than 256 blocks, so the single-block scan of the per-block counts carries from one pass to the
    next; kept rows against the float64 restatement (points within 1e-3 of +-radius after the transform are left out of the
    input, so no rounding decides), values inside its bound"""
    from efgh_amd.data import SweepSet, preproc_gt, preproc_pcd
    rng = np.random.default_rng(9)
    Ms = []
    for i in (1, 2):
        M = np.eye(4)
        M[:3, :3] = [[np.cos(0.02 * i), -np.sin(0.02 * i), 0], [np.sin(0.02 * i), np.cos(0.02 * i), 0], [0, 0, 1]]
        M[:3, 3] = (1.1 * i, -0.2 * i, 0.03 * i)
        Ms.append(M)
    sweeps = []
    for k in range(3):
        p = rng.uniform(-60, 60, (30000, 3)).astype(np.float32)
        q = SC.positions([p[:1], p], [Ms[k - 1]] if k else [np.eye(4)])[0][1:] if k else p.astype(np.float64)
        sweeps.append(np.ascontiguousarray(p[(np.abs(np.abs(q[:, :2]) - 50.0) > 1e-3).all(axis=1)]))
    assert sum(s.shape[0] for s in sweeps) > 256 * 256
    T = preproc_gt(0.1, -0.05, 0.3, 0.2, 0.1, -0.3, 0.0)['rand_init_l']
    n_keep = int(SC.chain(sweeps, Ms, T, 1 << 20)['keep'].size)
    sel = rng.permutation(n_keep)[:4096]
    ref = SC.chain(sweeps, Ms, T, 4096, sampled_indices=sel)
    ss = SweepSet(sweeps, Ms)
    assert np.array_equal(ss.kept_indices().cpu().numpy(), ref['keep'])
    out32, out64 = preproc_pcd(ss, {'rand_init_l': T}, 4096, sampled_indices=sel, want_float64=True)
    assert SC.within(out64.cpu().numpy(), ref['out64'], ref['bound'])
    assert np.array_equal(out32.cpu().numpy(), out64.cpu().numpy().astype(np.float32))
