"""Multi-sweep accumulation, host side (no GPU): the index / walk / transform helpers of efgh_amd.data against what the
unmodified reference loaders did (tests/golden/sweeps.npz, make_golden_sweeps.py), the float64 restatement of the chain
(tests/sweeps_contract.py) against the reference's recorded clouds, and SweepSet's argument checks."""
import numpy as np
import pytest

from tests import sweeps_contract as SC


@pytest.fixture(scope='module')
def fx(golden_dir):
    return SC.load_cases(golden_dir)


def test_accumulation_indices_equal_the_reference_walks(fx):
    """both ends of the sequence (the walk breaks at the first frame outside), skip 2 and 3, num = 0, num past both ends"""
    from efgh_amd.data import accumulation_indices
    G, _ = fx
    seen = set()
    for row in G['odom.walks']:
        own, n_frames, num, skip, n_prev, n_next = [int(v) for v in row[:6]]
        frames = [int(v) for v in row[6:6 + n_prev + n_next]]
        prev, nxt = accumulation_indices(own, n_frames, num, skip)
        assert prev == frames[:n_prev] and nxt == frames[n_prev:], (own, num, skip)
        seen.add((n_prev < num, n_next < num, num == 0, skip > 1))
    assert {(True, False, False, False), (False, True, False, False), (False, False, True, False)} <= seen
    assert any(s[3] for s in seen)
    for name in ('odomA', 'odomB', 'odomC', 'rellisA'):
        c = fx[1][name]
        prev, nxt = accumulation_indices(c['own'], int(G[name + '.meta'][6]), c['num'], c['skip'])
        assert [c['own']] + prev + nxt == [int(f) for f in G[name + '.frames']]


def test_nusc_walk_equals_the_reference_walks(fx):
    from efgh_amd.data import nusc_walk
    G, _ = fx
    for row in G['nusc.walks']:
        own, n_rec, num, skip, n_next, n_prev = [int(v) for v in row[:6]]
        frames = [int(v) for v in row[6:6 + n_next + n_prev]]
        recs = {str(i): {'token': str(i), 'next': str(i + 1) if i + 1 < n_rec else '', 'prev': str(i - 1) if i > 0 else ''}
                for i in range(n_rec)}
        nxt = nusc_walk(recs[str(own)], recs.__getitem__, 'next', num, skip)
        prev = nusc_walk(recs[str(own)], recs.__getitem__, 'prev', num, skip)
        assert [int(t) for t in nxt] == frames[:n_next] and [int(t) for t in prev] == frames[n_next:], (own, num, skip)
    assert [int(f) for f in G['nuscA.frames']] == [4, 5, 6, 7, 3, 2, 1]


def test_transform_helpers_equal_the_recorded_matrices_bit_for_bit(fx):
    from efgh_amd.data import accumulation_transform, nusc_accumulation_transform
    G, cases = fx
    n = 0
    for name in ('odomA', 'odomB', 'odomC', 'rellisA'):
        poses, frames = G[name + '.poses'], [int(f) for f in G[name + '.frames']]
        Tr = None if name == 'rellisA' else G['Tr']
        for f, M in zip(frames[1:], G[name + '.M']):
            assert np.array_equal(accumulation_transform(poses[frames[0]], poses[f], Tr), M), (name, f)
            n += 1
    P_o, P_vl = G['nuscA.P_o'], G['nuscA.P_vehicle_lidar']
    frames = [int(f) for f in G['nuscA.frames']]
    for f, M in zip(frames[1:], G['nuscA.M']):
        got = nusc_accumulation_transform(np.linalg.inv(P_o[frames[0]]), P_o[f], np.linalg.inv(P_vl), P_vl)
        assert np.array_equal(got, M), f
        n += 1
    assert n == 6 + 20 + 2 + 2 + 6


def test_contract_reproduces_the_reference(fx):
    """the restatement keeps exactly the rows the reference keeps, in its order, and its float64 values lie inside its own
    bound of the reference's: the reference alone satisfies what the GPU test asks of the kernels"""
    from efgh_amd.data import preproc_gt
    G, cases = fx
    for name, c in cases.items():
        T = preproc_gt(*c['rand_init'])['rand_init_l']
        r = SC.chain_of(c, T)
        assert np.array_equal(r['keep'], c['keep']), name
        assert r['out64'].shape == c['out_pc'].shape
        assert SC.within(r['out64'], c['out_pc'], r['bound']), name
        assert float(r['bound'].max()) < 1e-12, name                    # the bound is a few ulp of float64, not a tolerance
        if c['acc'] is not None:
            assert r['acc'].shape == c['acc'].shape
            assert SC.within(r['acc'], c['acc'], r['acc_bound']), name
            n_own = int(SC.positions(c['sweeps'][:1], [], None, c['ego_box'])[2].sum())
            assert np.array_equal(r['acc'][:n_own].view(np.int64), c['acc'][:n_own].astype(np.float64).view(np.int64)), name


def test_fixture_conditions(fx):
    """what make_golden_sweeps.py asserts, re-checked: transformed points keep clear of +-radius by 1e-6, the directed boundary
    points stand in the own sweeps, a sweep is removed entirely by the radius and one by the ego box, and the lengths are
    the ones at which a compaction can go wrong"""
    G, cases = fx
    f32 = np.float32
    for name, c in cases.items():
        q, _, ego = SC.positions(c['sweeps'], c['transforms'], c['own_order'], c['ego_box'])
        n_own = c['sweeps'][0].shape[0]
        far = np.abs(np.abs(q[n_own:, :2]) - 50.0)
        assert far.size == 0 or far.min() > 1e-6, name
    a = cases['odomA']
    assert [s.shape[0] for s in a['sweeps']] == [257, 0, 63, 64, 65, 1, 700]
    own = a['sweeps'][0]
    nb = lambda v, up: np.nextafter(f32(v), f32(np.inf if up else -np.inf))
    for v in (f32(50), f32(-50), nb(50, True), nb(50, False), nb(-50, True), nb(-50, False)):
        assert (own[:, 0] == v).any() and (own[:, 1] == v).any()
    assert np.isnan(own[:, 0]).any() and (np.signbit(own[:, 0]) & (own[:, 0] == 0)).any()
    kept_sweep = np.searchsorted(np.cumsum([s.shape[0] for s in a['sweeps']]), a['keep'], side='right')
    assert 2 not in kept_sweep and {0, 3, 4, 6} <= set(kept_sweep.tolist())          # the radius removes sweep 2 entirely
    assert a['keep'].size < a['num_points']                                          # zero-pad tail
    assert len(cases['odomB']['sweeps']) == 21 and cases['odomB']['keep'].size > cases['odomB']['num_points']
    assert cases['odomC']['lidar_line'] == 32 and len(cases['odomC']['sweeps']) == 3
    n = cases['nuscA']
    own = n['sweeps'][0]
    for b in (f32(0.8), f32(2.7)):
        col = 0 if b == f32(0.8) else 1
        for v in (b, nb(b, True), nb(b, False)):
            assert (own[:, col] == v).any() and (own[:, col] == -v).any()
    off = np.concatenate([[0], np.cumsum([s.shape[0] for s in n['sweeps']])])
    ego_kept = G['nuscA.ego_keep']
    per_sweep = [int(((ego_kept >= off[k]) & (ego_kept < off[k + 1])).sum()) for k in range(7)]
    assert per_sweep[2] == 0 and min(per_sweep[:2] + per_sweep[3:]) > 0             # the ego box removes sweep 2 entirely
    assert n['sweeps'][0].shape[1] == 3 and a['sweeps'][0].shape[1] == 4            # row stride 3 and row stride 4


def test_sweepset_argument_checks():
    from efgh_amd._C import EfghError
    from efgh_amd.data import SweepSet, preproc_gt, preproc_pcd
    p4, p3, I = np.zeros((5, 4), np.float32), np.zeros((5, 3), np.float32), np.eye(4)
    s = SweepSet([p4, np.zeros((0, 4), np.float32), p4], [I, I], own_order=[4, 3, 2, 1, 0], ego_box=(0.8, 2.7))
    assert (s.K, s.n_total, s.lengths, s.stride) == (3, 10, [5, 0, 5], 4)
    assert SweepSet([p3] * 64, [I] * 63).K == 64
    for bad in (lambda: SweepSet([p3] * 65, [I] * 64),                               # K = 65
                lambda: SweepSet([]),
                lambda: SweepSet([np.zeros((0, 3), np.float32), p3], [I]),           # empty own sweep
                lambda: SweepSet([p3, p3], [I, I]),                                  # one transform too many
                lambda: SweepSet([p3, p3]),
                lambda: SweepSet([p3, p4], [I]),                                     # mixed strides
                lambda: SweepSet([np.zeros((5, 5), np.float32)]),
                lambda: SweepSet([np.zeros(15, np.float32)]),
                lambda: SweepSet([p3, p3], [np.eye(3)]),
                lambda: SweepSet([p3], own_order=[0, 1, 2, 3, 3]),
                lambda: SweepSet([p3], own_order=[0, 1, 2]),
                lambda: SweepSet([p3], ego_box=(0.8, -1.0))):
        with pytest.raises(EfghError):
            bad()
    with pytest.raises(EfghError, match='lidar_line'):                               # no loader of the reference combines the two
        preproc_pcd(s, preproc_gt(0, 0, 0, 0, 0, 0, 0), 8, lidar_line=32)
