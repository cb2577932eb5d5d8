"""CPU-side checks of the BCL neighbourhood radius (scale_map's second column, r = 1, 2, 3): the E net's parameter layout against the
reference's at every radius, the tap offsets and their mirror permutation against the reference's radius2offset, the refusal of
other values, and the C-ABI entry points of the radius-r kernels."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from bcl_radius_tables import neighbor_table
from efgh_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'bcl_radius.npz')
VARIANTS = ('r2', 'r3', 'mixed')
SCALES = (1., 0.75, 0.5, 0.25, 0.125)


@pytest.fixture(scope='module')
def G():
    return np.load(GOLDEN)


def _args(radii):
    return dict(syn.default_args((128, 256), 'cpu'), scale_map=[[s, r] for s, r in zip(SCALES, radii)])


@pytest.mark.parametrize('tag', VARIANTS)
def test_enet_state_dict_matches_reference(G, tag):
    """the E net at radius 2 / 3 / mixed has the reference's state-dict names and shapes (blur weights (C0, C, F, 1))"""
    from efgh_amd.nets.enet import Enet
    m = Enet(_args([int(r) for r in G[f'{tag}.radii']]))
    sd = m.state_dict()
    assert list(sd.keys()) == [str(n) for n in G[f'{tag}.sd_names']]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(G[f'{tag}.sd_shapes']))


def test_builder_weight_shape():
    from efgh_amd.nets.builders import BilateralConvFlex
    for r, F in ((1, 15), (2, 65), (3, 175)):
        assert tuple(BilateralConvFlex(36, [32, 32], r).blur_conv[0].weight.shape) == (32, 36, F, 1)
    assert tuple(BilateralConvFlex(36, [32, 32]).blur_conv[0].weight.shape) == (32, 36, 15, 1)


def test_offsets_and_mirror_match_reference(G):
    from efgh_amd import lattice
    for r in (1, 2, 3):
        off, inv = lattice.filter_offsets(r)
        assert np.array_equal(off, G[f'radius2offset{r}']), r
        assert len(off) == lattice.filter_size(r) == (r + 1) ** 4 - r ** 4
        assert np.array_equal(off[inv], -off) and np.array_equal(inv[inv], np.arange(len(off)))
    assert lattice.filter_offsets(1)[1].tolist() == [0] + [15 - t for t in range(1, 15)]
    assert [lattice.table_ld(lattice.filter_size(r)) for r in (1, 2, 3)] == [16, 68, 184]


def test_neighbour_relation_symmetric_with_aliases(G):
    """the reference's tables are symmetric INCLUDING key2int's aliased hits (key2int is affine in the key): nbr[h][t] == m  <=>
    nbr[m][inv t] == h.  This is what lets the radius-r data gradient run as a gather through the same table."""
    from efgh_amd import lattice
    n_alias = 0
    for r in (2, 3):
        off, inv = lattice.filter_offsets(r)
        for l in range(5):
            nbr, hits_ = neighbor_table(G[f'alias.r{r}.keys{l}'], G[f'alias.r{r}.kmin{l}'], G[f'alias.r{r}.kmax{l}'], off)    # [F][H]
            F, H = nbr.shape
            assert H == int(G[f'alias.r{r}.H{l}'])
            t, h = np.nonzero(nbr >= 0)
            m = nbr[t, h]
            assert np.array_equal(nbr[inv[t], m], h), (r, l)
            hits = G[f'alias.r{r}.hits{l}']
            assert np.array_equal(hits, hits_)
            n_alias += len(hits)
            if len(hits):
                assert (nbr[hits[:, 1], hits[:, 0]] >= 0).all()
                assert np.array_equal(nbr[inv[hits[:, 1]], nbr[hits[:, 1], hits[:, 0]]], hits[:, 0])
    assert n_alias == 0          # (none of the scenes tried has one: tests/golden/make_golden_bcl_radius.py)
    off, inv = lattice.filter_offsets(3)
    for l in range(5):                                     # the sweep: radius-3 tables
        nbr = neighbor_table(G[f'lat.keys{l}'], G[f'lat.kmin{l}'], G[f'lat.kmax{l}'], off)[0].astype(np.int64)
        assert nbr.shape == (175, int(G[f'lat.H{l}']))
        h, t = np.nonzero(nbr.T >= 0)
        assert np.array_equal(nbr[inv[t], nbr[t, h]], h), l


@pytest.mark.parametrize('bad', [0, -1, 4, 2.5, True])
def test_bad_radius_raises(bad):
    from efgh_amd._C import EfghError
    from efgh_amd.nets.builders import BilateralConvFlex
    from efgh_amd.nets.enet import Enet
    radii = [1, 2, bad, 1, 1]
    with pytest.raises(EfghError, match=r'level 2'):
        Enet(_args(radii))
    with pytest.raises(EfghError, match=re.escape(repr(bad))):
        Enet(_args(radii))
    with pytest.raises(EfghError):
        BilateralConvFlex(36, [32, 32], bad)


def test_dim_not_3_raises():
    from efgh_amd._C import EfghError
    from efgh_amd.nets.enet import Enet
    with pytest.raises(EfghError, match='dim'):
        Enet(dict(_args([1] * 5), dim=2))


def test_radius_entry_points_exported():
    from efgh_amd import build
    so = build.build()
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'efgh_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(so)
    for n in ('efgh_lattice_neighbors_r_workspace', 'efgh_lattice_neighbors_r', 'efgh_blur_r_gemm', 'efgh_blur_r_wgrad'):
        assert re.search(r'\b' + n + r'\s*\(', hdr), n
        assert hasattr(lib, n), n
    lib.efgh_version.restype = ctypes.c_int
    assert lib.efgh_version() == 4
    lib.efgh_lattice_neighbors_r_workspace.restype = ctypes.c_int64
    assert lib.efgh_lattice_neighbors_r_workspace(ctypes.c_int32(1000), ctypes.c_int32(2)) > 1000 * 16
    # argument validation before any device work
    assert lib.efgh_blur_r_gemm(None, ctypes.c_int32(68), None) == -1
    assert lib.efgh_blur_r_wgrad(None, ctypes.c_int32(68), None, ctypes.c_int64(0), None, None, None) == -1
    assert lib.efgh_lattice_neighbors_r(*([None] * 17)) == -1
