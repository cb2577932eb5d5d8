"""Voxel thinning, host side (no GPU): the numpy contract (tests/voxel_contract.py) against np.unique, the directed fixtures
against the properties they are named for, planted faults in the contract against the fixtures, and the argument checks of
the C ABI and of the Python entry points."""
import ctypes

import numpy as np
import pytest

from tests import voxel_contract as VC


@pytest.fixture(scope='module')
def cases():
    return VC.cases()


def test_contract_equals_numpy_unique_on_random_clouds():
    """first occurrences of np.unique over the voxel indices, merged with the rows that have no index"""
    rng = np.random.default_rng(0)
    for n, v, spread in ((1, 0.2, 1.0), (50, 0.2, 1.0), (2000, 0.1, 3.0), (2000, 0.5, 1e6), (3000, 0.25, 1.5)):
        q = rng.uniform(-spread, spread, (n, 3))
        if n > 10:
            q[rng.integers(0, n, 5), 2] = np.nan
            q[rng.integers(0, n, 5), 1] = np.inf
        t = VC.indices(q, v)
        with np.errstate(invalid='ignore'):
            rep = np.isfinite(t).all(axis=1) & (np.abs(t) < VC.LIM).all(axis=1)
        rows = np.nonzero(rep)[0]
        _, first = np.unique(t[rows].astype(np.int64), axis=0, return_index=True)
        want = np.sort(np.concatenate([rows[first], np.nonzero(~rep)[0]]))
        got = VC.keep(q, v)
        assert np.array_equal(got, want), n
        if spread > 1e5:
            assert (~rep).sum() > 10                      # indices past 2^20 really occur in that cloud


def test_key_layout():
    assert VC.pack(-VC.LIM + 1, 0, 0) == 1 | VC.LIM << 21 | VC.LIM << 42
    top = VC.pack(VC.LIM - 1, VC.LIM - 1, VC.LIM - 1)
    assert top == (1 << 63) - 1 and top != (1 << 64) - 1                       # 63 bits: never the empty marker
    assert VC.mix64(0) == 0 and VC.mix64(1) == 0xb456bcfc34c2cb2c              # the published fmix64 of MurmurHash3
    assert [VC.capacity(n) for n in (0, 1, 2, 3, 4, 5, 2048, 2049, 4000, 4096)] == [2, 2, 4, 8, 8, 16, 4096, 8192, 8192, 8192]


def test_collision_and_wrap_fixtures_have_their_properties():
    for fixture, wrapped in ((VC.collision_fixture, False), (VC.wrap_fixture, True)):
        c, info = fixture()
        n = c['sweeps'][0].shape[0]
        assert n == info['n'] and VC.capacity(n) == info['cap'] == 32
        key, rep = VC.keys(c['sweeps'][0][:, :3].astype(np.float64), c['v'])
        assert rep.all()
        homes = {}
        for k in set(key.tolist()):
            homes.setdefault(VC.home(k, info['cap']), set()).add(k)
        assert {s: len(ks) for s, ks in homes.items()} == {s: len(ts) for s, ts in info['chains'].items()}
        for s, ts in info['chains'].items():
            assert homes[s] == {VC.pack(*t) for t in ts}
        assert max(len(ks) for ks in homes.values()) >= 3                      # a chain of three distinct keys on one home slot
        if wrapped:
            assert len(homes[info['cap'] - 1]) >= 3 and 0 in homes and 1 in homes     # it runs over slot cap-1 into taken slots
        assert np.array_equal(VC.expected(c), np.arange(n // 2))               # each voxel twice: the first half stays


def test_directed_fixtures(cases):
    c = cases['131_in_one']
    assert np.array_equal(VC.expected(c), [0]) and c['sweeps'][0].shape[0] == 131
    assert np.array_equal(VC.expected(cases['two_in_one']), [0]) and np.array_equal(VC.expected(cases['n1']), [0])
    assert np.array_equal(VC.expected(cases['first_is_last_of_block']), np.arange(256))
    f = cases['faces']
    p = f['sweeps'][0]
    assert np.array_equal(p[:, :3] * 8, np.round(p[:, :3] * 8), equal_nan=True)       # multiples of v / 2: every operation exact
    t = VC.indices(p[:, :3], f['v'])
    fin = t[np.isfinite(t)]
    assert {VC.LIM - 1, VC.LIM, -(VC.LIM - 1), -VC.LIM, -1, 0}.issubset(set(fin.tolist()))
    assert np.isnan(p[:, 2]).sum() == 4 and np.isinf(p[:, 2]).sum() >= 6
    assert (np.signbit(p[:, 0]) & (p[:, 0] == 0)).any()
    key, rep = VC.keys(p[:, :3], f['v'])
    kept = VC.expected(f)
    assert set(np.nonzero(~rep)[0].tolist()) <= set(kept.tolist()) and (~rep).sum() >= 20      # kept alone, every time
    half = p.shape[0] // 2
    assert not (rep[kept] & (kept >= half)).any()                              # the second copy of a representable row never stays
    k3 = cases['k3_identical']
    assert np.array_equal(VC.expected(k3), VC.expected(VC.case(k3['sweeps'][:1], k3['v'])))    # exactly the own sweep thinned
    d = cases['distinct3000']
    assert VC.expected(d).size == 3000 and VC.capacity(d['sweeps'][0].shape[0]) == 8192
    assert [s.shape[0] for s in cases['lengths']['sweeps']] == [257, 0, 63, 64, 65, 1, 700]
    assert len(cases['k21']['sweeps']) == 21
    for name in ('k21', 'lengths', 'ego_radius_voxel', 'lidar_line', 'lengths/rellis'):
        c = cases[name]
        cand, _ = VC.candidates(c)
        kept = VC.expected(c)
        n_own = c['sweeps'][0].shape[0]
        assert kept.size < cand.size and (kept >= n_own).any() and (cand[~np.isin(cand, kept)] >= n_own).any(), name
        assert not any(np.array_equal(T, np.eye(4)) for T in c['transforms'])
    e = cases['ego_radius_voxel']
    assert VC.candidates(e)[0].size < sum(s.shape[0] for s in e['sweeps']) - 40


def test_every_non_exact_fixture_holds_the_margin(cases):
    """every row, every axis: no row is left out of any comparison"""
    for name, c in cases.items():
        q = VC.SC.positions(c['sweeps'], c['transforms'], c['own_order'], c['ego_box'])[0]
        if c['exact']:
            assert all(np.array_equal(T, np.eye(4)) for T in c['transforms']) and c['v'] == 0.25, name
            continue
        assert VC.margin(q, c['v']) > VC.MARGIN, name
        assert VC.radius_margin(c) > VC.MARGIN, name
        _, b1, _ = VC.SC.positions(c['sweeps'], c['transforms'], c['own_order'], c['ego_box'])
        assert float(b1.max()) / c['v'] < 1e-12, name                          # what two evaluations can differ by, in voxels


def test_planted_faults_change_a_fixture(cases):
    changed = {f: [] for f in VC.FAULTS}
    good = {name: VC.expected(c) for name, c in cases.items()}
    for fault in VC.FAULTS:
        for name, c in cases.items():
            if not np.array_equal(VC.expected(c, fault), good[name]):
                changed[fault].append(name)
    assert all(changed.values()), changed
    assert 'f32_division' in changed['f32_division'] and 'faces' in changed['merge_unrepresentable']
    assert 'faces' in changed['trunc'] and '131_in_one' in changed['last_seen']


# ---- argument checks -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from efgh_amd import build
    L = ctypes.CDLL(build.build())
    L.efgh_last_error.restype = ctypes.c_char_p
    L.efgh_prep_voxel_workspace.restype = ctypes.c_int64
    return L


def test_workspace_size(lib):
    ws = lambda n: lib.efgh_prep_voxel_workspace(ctypes.c_int32(n))
    assert ws(-1) == -1 and ws(1 << 29) == -1
    for n in (0, 1, 255, 256, 257, 4000, 243040):
        assert ws(n) == 12 * VC.capacity(n) + 4 * n + 4 * ((n + 255) // 256), n


def test_cabi_refusals_name_the_argument(lib):
    """every refusal is EFGH_E_INVALID with a message naming what was wrong, before anything is launched (there is no device here)"""
    i32, f64 = ctypes.c_int32, ctypes.c_double
    pts = (ctypes.c_float * 64)()                          # host memory: never dereferenced by a refused call
    ws = (ctypes.c_uint64 * 64)()
    out, cnt = (ctypes.c_int32 * 16)(), (ctypes.c_int32 * 2)(-7, -7)
    wsp = ctypes.cast(ws, ctypes.c_void_p)
    base = ctypes.addressof(pts)
    p16 = ctypes.c_void_p(base + (-base) % 16)

    def plain(pts=p16, stride=4, rows=8, keep_in=None, n=8, n_dev=None, v=0.2, ws=wsp, out=out, cnt=cnt):
        return lib.efgh_prep_voxel_keep(pts, i32(stride), i32(rows), keep_in, i32(n), n_dev, f64(v), ws, out, cnt, None)

    for kw, word in (({'v': 0.0}, 'voxel'), ({'v': -0.2}, 'voxel'), ({'v': float('nan')}, 'voxel'), ({'v': float('inf')}, 'voxel'),
                     ({'n': -1}, 'n_cap'), ({'n': 9}, 'n_cap'), ({'ws': None}, 'workspace'),
                     ({'ws': ctypes.c_void_p(wsp.value + 4)}, 'workspace'), ({'out': None}, 'keep_out'), ({'cnt': None}, 'count'),
                     ({'pts': None}, 'pts'), ({'rows': 0}, 'n_rows'), ({'stride': 5}, 'stride'),
                     ({'pts': ctypes.c_void_p(p16.value + 4)}, 'stride')):
        assert plain(**kw) == -1, kw
        assert word in lib.efgh_last_error().decode(), (kw, lib.efgh_last_error())
    off, M, ident = (ctypes.c_int32 * 2)(0, 8), (ctypes.c_double * 12)(), (ctypes.c_int32 * 1)(1)

    def sweeps(K=1, n_total=8, n=8, v=0.2, ws=wsp):
        return lib.efgh_prep_sweeps_voxel_keep(p16, i32(4), off, M, ident, i32(K), i32(n_total), None, i32(n), None, f64(v), ws, out,
                                               cnt, None)

    for kw, word in (({'K': 65}, 'K = 65'), ({'n_total': 0}, 'n_total'), ({'v': 0.0}, 'voxel'), ({'n': -3}, 'n_cap'),
                     ({'n': 9}, 'n_cap'), ({'ws': None}, 'workspace')):
        assert sweeps(**kw) == -1, kw
        assert word in lib.efgh_last_error().decode(), (kw, lib.efgh_last_error())
    assert list(cnt) == [-7, -7] and not any(out)


def test_python_argument_errors_name_the_argument():
    from efgh_amd._C import EfghError
    from efgh_amd.data import ProcessKITTIODOM, SweepSet, preproc_gt, preproc_pcd, voxel_keep
    p = np.zeros((5, 4), np.float32)
    gts = preproc_gt(0, 0, 0, 0, 0, 0, 0)
    for bad in (0, -0.1, float('nan'), float('inf'), 'a', [0.1]):
        for call in (lambda: voxel_keep(p, bad), lambda: preproc_pcd(p, gts, 8, voxel_size=bad),
                     lambda: preproc_pcd(SweepSet([p]), gts, 8, voxel_size=bad), lambda: SweepSet([p]).kept_indices(voxel_size=bad),
                     lambda: ProcessKITTIODOM({'raw_cam_img_size': [8, 8], 'lidar_line': None, 'num_points': 8, 'test': True,
                                               'voxel_size': bad})):
            with pytest.raises(EfghError, match='voxel_size'):
                call()
    with pytest.raises(EfghError, match='points'):
        voxel_keep(np.zeros((5, 5), np.float32), 0.2)
    with pytest.raises(EfghError, match='points'):
        voxel_keep(np.zeros((0, 3), np.float32), 0.2)
    assert ProcessKITTIODOM({'raw_cam_img_size': [8, 8], 'lidar_line': None, 'num_points': 8, 'test': True}).voxel_size is None
