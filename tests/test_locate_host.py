"""CPU-side checks of the lattice point query: the invariants of tests/golden/locate.npz (the reference's answers for points that
did not build the lattice), the inversion restatement on offsets that hold -1, and the C-ABI entry points."""
import ctypes
import os

import numpy as np
import pytest

import bcl_layer_contract as K
import locate_contract as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'locate.npz')
ULP1 = 2.0 ** -23            # float32 spacing at 1
# points by number of corners found (0..4) over all 2048 points of a set at scale 1.0 (H = 6068), as the fixture was specified
CLASSES_S100 = {'other': [431, 377, 421, 427, 392], 'jit': [0, 112, 442, 711, 783], 'far': [1849, 90, 55, 38, 16],
                'self': [0, 0, 0, 0, 2048]}


@pytest.fixture(scope='module')
def G():
    return np.load(GOLDEN)


@pytest.mark.parametrize('s', Q.SCALES)
@pytest.mark.parametrize('name', Q.SETS + ('alias',))
def test_fixture_invariants(G, s, name):
    t = Q.tag(s)
    H = int(G[f'{t}.H'])
    bary, off = G[f'{t}.{name}.bary'], G[f'{t}.{name}.off'].astype(np.int64)
    n = Q.N_QUERY if name != 'alias' else G[f'{t}.alias.pts'].shape[1]
    assert bary.shape == off.shape == (n, 4) and bary.dtype == np.float32
    assert np.abs(bary.astype(np.float64).sum(1) - 1.0).max() <= 4 * ULP1
    found = off >= 0
    assert (off[found] < H).all() and (off[~found] == -1).all()
    assert G[f'{t}.{name}.missing'].tolist() == [int((~found).sum()), int((found.sum(1) == 0).sum())]
    if name == 'alias':
        mask = G[f'{t}.alias.mask'].astype(bool)
        assert mask.any(1).all() and (off[mask] == -1).all()
        return
    cls = G[f'{t}.{name}.classes2048'].tolist()
    assert sum(cls) == Q.N_POINTS
    if s == 1.0:
        assert H == 6068 and cls == CLASSES_S100[name]
        if name == 'other':
            assert (np.bincount(found.sum(1), minlength=5) > 0).all()          # every class among the stored points as well
        if name == 'far':
            assert int(G[f'{t}.far.outbox2048']) == 6547
    if name == 'far':
        assert int(G[f'{t}.far.outbox2048']) >= 6000 and not found[:, :].all()
    if name == 'self':
        assert found.all() and cls == [0, 0, 0, 0, Q.N_POINTS]
        assert np.array_equal(off, G[f'{t}.lattice_offset'])                     # the reference's pc1_lattice_offset rows


@pytest.mark.parametrize('s', Q.SCALES)
@pytest.mark.parametrize('name', Q.SETS + ('alias',))
def test_inversion_counts_the_absent_corners(G, s, name):
    """the restatement of efgh_offsets_invert leaves out exactly the stored number of absent corners, and lists every other one"""
    t = Q.tag(s)
    H, off = int(G[f'{t}.H']), G[f'{t}.{name}.off']
    vseg, lst, bad = K.invert_lists(off, H)
    assert bad == int(G[f'{t}.{name}.missing'][0])
    assert len(lst) == off.size - bad and int(vseg[:, 1].sum()) == len(lst)
    assert (off.reshape(-1)[lst] >= 0).all()


def test_masked_offsets_give_the_same_slice(G):
    """-1 replaced by row 0 with weight 0 (what the float64 restatements are fed) is the sum over the present corners"""
    t = Q.tag(1.0)
    H = int(G[f'{t}.H'])
    bary, off = G[f'{t}.other.bary'], G[f'{t}.other.off'].astype(np.int64)
    feat = np.random.default_rng(0).standard_normal((H, 4))
    b0, o0 = Q.masked(bary, off)
    got, _ = K.slice_ref(feat, b0, o0)
    want = np.zeros_like(got)
    for p in range(off.shape[0]):
        for r in range(4):
            if off[p, r] >= 0:
                want[p] += np.float64(bary[p, r]) * feat[off[p, r]]
    assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max()


def test_cabi_symbols():
    from efgh_amd import build
    lib = ctypes.CDLL(build.build())
    for n in ('efgh_lattice_index_bytes', 'efgh_lattice_index_build', 'efgh_lattice_locate'):
        assert hasattr(lib, n), n
    hdr = open(os.path.join(ROOT, 'include', 'efgh_hip.h')).read()
    for n in ('efgh_lattice_index_bytes(', 'efgh_lattice_index_build(', 'efgh_lattice_locate('):
        assert n in hdr
    lib.efgh_lattice_index_bytes.restype = ctypes.c_int64
    lib.efgh_lattice_neighbors_r_workspace.restype = ctypes.c_int64
    # table of >= 2 H slots (load <= 1/2) of 12 bytes, + the key boxes
    assert lib.efgh_lattice_index_bytes(ctypes.c_int32(6068), ctypes.c_int32(2)) >= 2 * 6068 * 12 + 2 * 32
    assert lib.efgh_lattice_index_bytes(ctypes.c_int32(0), ctypes.c_int32(1)) == 0
    lib.efgh_last_error.restype = ctypes.c_char_p
    assert lib.efgh_lattice_index_build(*([None] * 13)) == -1
    assert b'invalid argument' in lib.efgh_last_error()
    assert lib.efgh_lattice_locate(*([None] * 14)) == -1


def test_layer_eval_is_the_restatement(G):
    """locate_contract.layer_eval at float64 gives bcl_layer_contract.layer_ref's numbers (it exists to evaluate the same
    restatement in float32), on a small made-up lattice with absent corners among the out points"""
    import torch
    rng = np.random.default_rng(3)
    H, n, C = 40, 50, 8
    cfg = dict(K._BASE, num_output=[16, 12])
    lat = dict(H=H, bary=torch.from_numpy(rng.random((n, 4))), off=torch.from_numpy(rng.integers(0, H, (n, 4))),
               nbr=torch.from_numpy(rng.integers(-1, H, (H, 15))))
    params = {'blur_conv.0.weight': torch.from_numpy(rng.standard_normal((16, C, 15, 1))), 'blur_conv.0.bias': torch.from_numpy(rng.standard_normal(16)),
              'blur_conv.2.weight': torch.from_numpy(rng.standard_normal((12, 16, 1, 1))), 'blur_conv.2.bias': torch.from_numpy(rng.standard_normal(12)),
              'bias': torch.from_numpy(rng.standard_normal(12))}
    ob, oo = Q.masked(rng.random((30, 4)), rng.integers(-1, H, (30, 4)))
    ob, oo = torch.from_numpy(ob), torch.from_numpy(oo)
    x = torch.from_numpy(rng.standard_normal((n, C)))
    assert torch.equal(K.layer_ref(cfg, params, x, lat, ob, oo), Q.layer_eval(cfg, params, x, lat, ob, oo, torch.float64))
