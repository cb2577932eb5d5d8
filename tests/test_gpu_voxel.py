"""Voxel thinning on the GPU (efgh_prep_voxel_keep / efgh_prep_sweeps_voxel_keep, csrc/prep.hip) against the numpy contract of
tests/voxel_contract.py: the kept rows bit for bit, on the smallest shapes at which the table, the waves, the blocks and the
compaction can go wrong (tests/test_voxel_host.py shows that every fixture has the property it is named for)."""
import os

import numpy as np
import pytest
import torch

from tests import sweeps_contract as SC
from tests import voxel_contract as VC
from tests.train_harness import waits_for_nothing

pytestmark = pytest.mark.gpu

CASES = VC.cases()


def _is_plain(c):
    return (len(c['sweeps']) == 1 and c['radius'] is None and c['lidar_line'] is None and c['own_order'] is None
            and c['ego_box'] is None)


def _set(c):
    from efgh_amd.data import SweepSet
    return SweepSet(c['sweeps'], c['transforms'], own_order=c['own_order'], ego_box=c['ego_box'])


def _gpu_keep(c):
    """the kept rows through every public route the case admits"""
    from efgh_amd.data import voxel_keep
    outs = [_set(c).kept_indices(radius=c['radius'], lidar_line=c['lidar_line'], flip_xy=c['flip_xy'], voxel_size=c['v'])]
    if _is_plain(c):
        outs.append(voxel_keep(c['sweeps'][0], c['v']))                       # packed rows at stride 3 or 4
        outs.append(voxel_keep(torch.from_numpy(c['sweeps'][0]).cuda(), c['v'], keep=np.arange(c['sweeps'][0].shape[0])))
    return outs


def test_n1_keeps_its_row():
    """fails without the feature: there is no voxel_keep and no voxel_size argument"""
    from efgh_amd.data import SweepSet, voxel_keep
    p = CASES['n1']['sweeps'][0]
    got = voxel_keep(p, 0.25)
    assert got.dtype == torch.int32 and got.is_cuda and got.cpu().tolist() == [0]
    assert SweepSet([p]).kept_indices(voxel_size=0.25).cpu().tolist() == [0]


@pytest.mark.parametrize('name', sorted(CASES))
def test_kept_rows_equal_the_contract(name):
    c = CASES[name]
    want = VC.expected(c)
    cand, q = VC.candidates(c)
    pos = {int(r): j for j, r in enumerate(cand)}
    key, rep = VC.keys(q, c['v'])
    runs = [_gpu_keep(c), _gpu_keep(c)]
    for got in runs[0] + runs[1]:
        got = got.cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, want), name          # bit for bit, in order
        js = [pos[int(r)] for r in got]
        assert js == sorted(js) and len(set(js)) == len(js)                       # ascending in the candidate order
        ks = [key[r] for r in got if rep[r]]
        assert len(ks) == len(set(ks))                                            # no two representable outputs share a voxel
        assert {key[r] for r in cand if rep[r]} == set(ks)                        # every occupied voxel is represented
        assert {int(r) for r in cand if not rep[r]} <= {int(r) for r in got}      # and every row without a voxel is there
    assert all(torch.equal(a, b) for a, b in zip(*runs))                          # two runs are identical


def test_more_blocks_than_one_scan_pass():
    """258 blocks: the single-block scan of the per-block counts carries from one pass to the next, and about three rows contend
    for every voxel"""
    from efgh_amd.data import voxel_keep
    p = VC.random_cloud(256 * 257 + 77, 3, half=(2.0, 2.0, 1.0))
    q = p[:, :3].astype(np.float64)
    assert VC.margin(q, 0.1) > VC.MARGIN
    want = VC.keep(q, 0.1)
    assert 0.2 * p.shape[0] < want.size < 0.6 * p.shape[0]
    assert np.array_equal(voxel_keep(p, 0.1).cpu().numpy(), want)


def test_keep_list_restricts_and_orders_the_candidates():
    """`keep` in front: candidates in the given order (here reversed, so the LAST row of a voxel in memory wins), and a sweep set's
    own selection chained by hand equals the fused call"""
    from efgh_amd.data import voxel_keep
    c = CASES['n513']
    p, n = c['sweeps'][0], c['sweeps'][0].shape[0]
    order = np.arange(n)[::-1].copy()
    got = voxel_keep(p, c['v'], keep=order).cpu().numpy()
    assert np.array_equal(got, order[VC.keep(p[order, :3].astype(np.float64), c['v'])])
    assert voxel_keep(p, c['v'], keep=np.zeros(0, np.int64)).numel() == 0
    e = CASES['ego_radius_voxel']
    ss = _set(e)
    by_hand = voxel_keep(ss, e['v'], keep=ss.kept_indices(radius=e['radius']))
    assert np.array_equal(by_hand.cpu().numpy(), VC.expected(e))


def _eye_gts():
    return {'rand_init_l': np.eye(4)}


def _columns(q, rows, flip, num_points):
    """what preproc_pcd returns under rand_init_l = I: the (flipped) positions of `rows`, then zero columns"""
    x, y, z = np.zeros(num_points), np.zeros(num_points), np.zeros(num_points)
    s = -1.0 if flip else 1.0
    x[:rows.size], y[:rows.size], z[:rows.size] = q[rows, 0] * s, q[rows, 1] * s, q[rows, 2]
    with np.errstate(invalid='ignore'):
        return SC._affine(np.eye(4), x, y, z)[0].T          # exact for finite rows; 0 * NaN and 0 * inf spread as in the kernel


@pytest.mark.parametrize('name,flip', [('n513', False), ('n513', True), ('n257/stride3', False), ('faces', False)])
def test_preproc_pcd_thins_then_pads_or_samples(name, flip):
    """plain arrays (every value exact under rand_init_l = I): zero padding when fewer than num_points remain, `sampled_indices`
    honoured when more remain; with the RELLIS flip the voxels are taken on the unflipped position"""
    from efgh_amd.data import preproc_pcd
    c = VC.case(CASES[name]['sweeps'], CASES[name]['v'], radius=1.5, flip_xy=flip)
    want = VC.expected(c)
    q = VC.candidates(c)[1]
    assert 8 < want.size < c['sweeps'][0].shape[0]
    p = c['sweeps'][0]
    pad = want.size + 7
    o32, o64 = preproc_pcd(p, _eye_gts(), pad, radius=1.5, flip_xy=flip, want_float64=True, voxel_size=c['v'])
    ref = _columns(q, want, flip, pad)
    assert np.array_equal(o64.cpu().numpy(), ref, equal_nan=True) and np.array_equal(o64.cpu().numpy()[:, want.size:], np.zeros((3, 7)))
    assert np.array_equal(o32.cpu().numpy(), ref.astype(np.float32), equal_nan=True)
    few = want.size - 5
    sel = np.random.default_rng(1).permutation(want.size)[:few]
    o64 = preproc_pcd(p, _eye_gts(), few, radius=1.5, flip_xy=flip, sampled_indices=sel, want_float64=True, voxel_size=c['v'])[1]
    assert np.array_equal(o64.cpu().numpy(), _columns(q, want[sel], flip, few), equal_nan=True)
    every = VC.expected(VC.case(c['sweeps'], c['v'], flip_xy=flip))             # no radius filter in front: rows 0 .. n-1
    o64 = preproc_pcd(p, _eye_gts(), every.size, radius=None, flip_xy=flip, want_float64=True, voxel_size=c['v'])[1]
    assert np.array_equal(o64.cpu().numpy(), _columns(q, every, flip, every.size), equal_nan=True)
    if name != 'faces':                                     # (no NaN columns: they compare unequal to themselves)
        drawn = preproc_pcd(p, _eye_gts(), few, radius=1.5, flip_xy=flip, want_float64=True, voxel_size=c['v'])[1].cpu().numpy()
        cols = {tuple(col) for col in _columns(q, want, flip, want.size).T.tolist()}
        assert all(tuple(col) in cols for col in drawn.T.tolist()) and len({tuple(col) for col in drawn.T.tolist()}) == few


def test_preproc_pcd_over_a_sweep_set():
    """ego box, radius and voxel in one chain, then the gather: values inside the bound of tests/sweeps_contract.py, the own sweep's
    bit for bit"""
    from efgh_amd.data import preproc_pcd
    c = CASES['ego_radius_voxel']
    want = VC.expected(c)
    q, b1, _ = SC.positions(c['sweeps'], c['transforms'], None, c['ego_box'])
    npts = want.size + 3
    o64 = preproc_pcd(_set(c), _eye_gts(), npts, radius=c['radius'], want_float64=True, voxel_size=c['v'])[1].cpu().numpy()
    ref = _columns(q, want, False, npts)
    bound = np.zeros((3, npts))
    bound[:, :want.size] = b1[want].T
    assert SC.within(o64, ref, bound)
    own = want < c['sweeps'][0].shape[0]
    assert own.any() and np.array_equal(o64[:, :want.size][:, own], ref[:, :want.size][:, own])


def _wrap_voxel_entry_points(monkeypatch):
    from efgh_amd import _C
    L, calls = _C.lib(), []
    for name in ('efgh_prep_voxel_workspace', 'efgh_prep_voxel_keep', 'efgh_prep_sweeps_voxel_keep'):
        fn = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _fn=fn, _name=name: (calls.append(_name), _fn(*a))[1])
    return calls


def test_without_voxel_size_nothing_changes(monkeypatch):
    """voxel_size=None and the argument left out: identical bits, and neither call reaches the new entry points"""
    from efgh_amd.data import preproc_gt, preproc_pcd
    gts = preproc_gt(0.1, -0.05, 0.3, 0.2, 0.1, -0.3, 0.0)
    calls = _wrap_voxel_entry_points(monkeypatch)
    for c, npts in ((CASES['n513'], 300), (CASES['n257/stride3'], 400), (CASES['lengths'], 512), (CASES['ego_radius_voxel'], 2048)):
        src = (lambda: c['sweeps'][0]) if len(c['sweeps']) == 1 else (lambda: _set(c))
        n_keep = VC.candidates(VC.case(c['sweeps'], c['v'], c['transforms'], ego_box=c['ego_box'], radius=1.9))[0].size
        sel = np.random.default_rng(2).permutation(n_keep)[:npts] if npts < n_keep else None
        a = preproc_pcd(src(), gts, npts, radius=1.9, sampled_indices=sel, want_float64=True)
        b = preproc_pcd(src(), gts, npts, radius=1.9, sampled_indices=sel, want_float64=True, voxel_size=None)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))
    assert calls == []
    preproc_pcd(CASES['n513']['sweeps'][0], gts, 300, radius=1.9, voxel_size=0.2)
    preproc_pcd(_set(CASES['lengths']), gts, 300, radius=1.9, voxel_size=0.2)
    assert calls == ['efgh_prep_voxel_workspace', 'efgh_prep_voxel_keep', 'efgh_prep_voxel_workspace', 'efgh_prep_sweeps_voxel_keep']


@pytest.mark.parametrize('kind', ['plain', 'sweeps'])
def test_one_host_read_per_thinned_sample(monkeypatch, kind):
    """radius filter + thinning + padding under a device that refuses to be waited for: the one read is `_read_counts`"""
    from efgh_amd.data import prepare, preproc_gt, preproc_pcd
    gts = preproc_gt(0.1, -0.05, 0.3, 0.2, 0.1, -0.3, 0.0)
    c = CASES['n513'] if kind == 'plain' else CASES['ego_radius_voxel']
    src = torch.from_numpy(c['sweeps'][0]).cuda() if kind == 'plain' else _set(c)
    want = preproc_pcd(src, gts, 2048, radius=1.9, voxel_size=0.2)              # staged and warm; the reference bits
    reads, real = [], prepare._read_counts

    def read(counts):
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode('default')
        try:
            reads.append(1)
            return real(counts)
        finally:
            torch.cuda.set_sync_debug_mode(mode)

    monkeypatch.setattr(prepare, '_read_counts', read)
    got = []
    run = lambda: got.append(preproc_pcd(src, gts, 2048, radius=1.9, voxel_size=0.2))
    waits_for_nothing(run)
    if got:                                                 # the guard has teeth: the same read outside the allowed place is refused
        with pytest.raises(RuntimeError):
            waits_for_nothing(lambda: real(torch.zeros(2, dtype=torch.int32, device='cuda')))
    else:                                                   # a build that cannot flag waits: the count is what is left to check
        run()
    assert len(reads) == 1
    assert torch.equal(got[0].view(torch.int32), want.view(torch.int32))


def test_process_classes_read_voxel_size(golden_dir):
    from efgh_amd.data import ProcessKITTIODOM, ProcessRELLIS, SweepSet, preproc_gt, preproc_pcd
    G, cases = SC.load_cases(golden_dir)
    c = cases['odomA']
    ss = lambda: SweepSet(c['sweeps'], c['transforms'], own_order=c['own_order'])
    for cls, cal, flip in ((ProcessKITTIODOM, {'P2': G['P2'], 'Tr': G['Tr']}, False), (ProcessRELLIS, {'P': G['P2'], 'Tr': G['Tr']}, True)):
        args = {'raw_cam_img_size': [12, 24], 'num_points': c['num_points'], 'test': True, 'lidar_line': None, 'voxel_size': 5.0}
        pc = cls(args)(ss(), G['odomA.img'], cal, G['pose_ji'], 'x', rand_init=c['rand_init'])[0]
        T = preproc_gt(*c['rand_init'])['rand_init_l']
        ref = preproc_pcd(ss(), {'rand_init_l': T}, c['num_points'], flip_xy=flip, voxel_size=5.0)
        assert torch.equal(pc.view(torch.int32), ref.view(torch.int32))
        plain = cls(dict(args, voxel_size=None))(ss(), G['odomA.img'], cal, G['pose_ji'], 'x', rand_init=c['rand_init'])[0]
        assert not torch.equal(pc, plain)


def test_example_loop_thins_accumulated_sweeps():
    """examples/train_synthetic.py --accumulate-sweeps 1 --voxel 0.2: the option reaches the sample preparation and the loop runs"""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'train_synthetic.py')
    spec = importlib.util.spec_from_file_location('train_synthetic_voxel', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hist = mod.main(['--iters', '1', '--batch', '1', '--accumulate-sweeps', '1', '--voxel', '0.2', '--raw', '128', '256', '--points', '2048'])
    assert len(hist) == 1 and np.isfinite(hist[0])
