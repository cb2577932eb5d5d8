"""CPU-side checks of the BCL as a layer (BilateralConvFlex with slice, bias and lattice-side input): the module's parameter layout
against the reference's for the five golden variants and for the E net's call, the float64 restatement of tests/bcl_layer_contract.py
against the reference's recorded outputs and gradients, the C-ABI entry points of the slice kernels, and the refusals."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import bcl_layer_contract as K
from bcl_radius_tables import neighbor_table
from efgh_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'bcl_layer.npz')


@pytest.fixture(scope='module')
def G():
    return np.load(GOLDEN)


@pytest.fixture(scope='module')
def LAT(G):
    """the two lattice levels of the golden's scene on the CPU: bary / off from the C restatement of the lattice build (checked
    against the golden's off), the radius-1 and radius-2 tables from the vertex keys stored with bcl_radius.npz"""
    from efgh_amd import lattice
    from oracle import lattice as OL
    R = np.load(os.path.join(ROOT, 'tests', 'golden', 'bcl_radius.npz'))
    gen = OL.generate_data(syn.lidar_sweep(K.N_POINTS, K.SCENE_SEED), K.SCALES)
    out = {}
    for l in (0, 3):
        d = gen[l]
        assert d['H'] == int(G[f'H{l}']) and np.array_equal(d['off'], G[f'off{l}'])
        for r in (1, 2):
            nbr = neighbor_table(R[f'lat.keys{l}'], R[f'lat.kmin{l}'], R[f'lat.kmax{l}'], lattice.filter_offsets(r)[0])[0]
            out[l, r] = dict(H=int(d['H']), bary=torch.from_numpy(d['bary'].T.copy()).double(),
                             off=torch.from_numpy(d['off'].T.copy()).long(), nbr=torch.from_numpy(nbr.T.astype(np.int64)))
        assert np.array_equal(out[l, 1]['nbr'].numpy().T, d['nbr'])
    return out


def _module(v):
    from efgh_amd.nets import BilateralConvFlex
    return BilateralConvFlex(v['num_input'], v['num_output'], v['radius'], d=3, DEVICE='cpu', use_bias=v['use_bias'],
                             use_leaky=v['use_leaky'], use_norm=v['use_norm'], do_splat=v['do_splat'], do_slice=v['do_slice'],
                             last_relu=v['last_relu'], chunk_size=-1)


@pytest.mark.parametrize('tag', sorted(K.VARIANTS))
def test_state_dict_matches_reference(G, tag):
    v = K.VARIANTS[tag]
    names, shapes = [str(n) for n in G[f'{tag}.sd_names']], json.loads(str(G[f'{tag}.sd_shapes']))
    from efgh_amd.nets import BilateralConvFlex
    ref_order = BilateralConvFlex(3, v['radius'], v['num_input'], v['num_output'], 'cpu', v['use_bias'], v['use_leaky'], v['use_norm'],
                                  v['do_splat'], v['do_slice'], v['last_relu'])          # the reference's own positional order
    for m in (_module(v), ref_order):
        sd = m.state_dict()
        assert list(sd.keys()) == names
        assert [list(t.shape) for t in sd.values()] == shapes
    if v['do_slice'] and v['use_bias']:
        assert float(m.bias.detach().abs().max()) == 0.0 and m.bias.requires_grad
    assert torch.equal(m.feat_indices, torch.arange(v['num_input']))


def test_enet_call_state_dict_unchanged():
    """the E net's positional call registers what it always did, with bcn_use_bias either way (do_slice=False: no bias, as in the
    reference), in the manifest's order"""
    from efgh_amd.nets.builders import BilateralConvFlex
    from efgh_amd.nets.enet import Enet
    man = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'state_dict_manifest.json')))['state_dict']
    want = [(k[len('E.bcn1.'):], list(s)) for k, s, _ in man if k.startswith('E.bcn1.')]
    for m in (BilateralConvFlex(36, [32, 32]), BilateralConvFlex(36, [32, 32], 1, use_bias=False)):
        assert [(k, list(t.shape)) for k, t in m.state_dict().items()] == want
    for ub in (True, False):
        e = Enet(dict(syn.default_args((128, 256), 'cpu'), bcn_use_bias=ub))
        assert ['E.' + k for k in e.state_dict()] == [k for k, _, _ in man if k.startswith('E.')]


@pytest.mark.parametrize('tag', sorted(K.VARIANTS))
def test_restatement_reproduces_reference(G, LAT, tag):
    """every recorded output and gradient of the reference, within twice the float32 error the generator measured for it"""
    v = K.VARIANTS[tag]
    lat = LAT[v['level'], v['radius']]
    names, shapes = [str(n) for n in G[f'{tag}.sd_names']], json.loads(str(G[f'{tag}.sd_shapes']))
    p64 = {k: t.double().requires_grad_(True) for k, t in K.variant_weights(tag, names, shapes).items()}
    rows = lat['bary'].shape[0] if v['do_splat'] else lat['H']
    x = torch.from_numpy(K.variant_input(tag, rows, v['num_input'])).double().requires_grad_(True)
    ob = oo = None
    if v['select']:
        idx = torch.from_numpy(K.select_idx(lat['bary'].shape[0]))
        assert np.array_equal(idx.numpy(), G['idx'])
        ob, oo = lat['bary'][idx], lat['off'][idx]
    out = K.layer_ref(v, p64, x, lat, ob, oo)
    (out * K.loss_weights(out.shape[1], out.shape[0])).sum().backward()
    got = {'out': out.detach().numpy(), 'grad.input': x.grad.numpy()}
    got.update({'grad.' + k: p.grad.numpy() for k, p in p64.items()})
    keys = [k[len(tag) + 1:] for k in G.files if k.startswith(tag + '.') and not k.startswith(tag + '.sd_')]
    assert sorted(keys) == sorted(got)
    for k in keys:
        f64 = got[k]
        sub = f64[::K.row_stride(f64.shape[0])] if k in ('out', 'grad.input') else f64
        err = float(np.abs(G[f'{tag}.{k}'].astype(np.float64) - sub).max() / np.abs(f64).max())
        assert err <= 2 * float(G[f'err.{tag}.{k}']), (k, err, float(G[f'err.{tag}.{k}']))


def test_inversion_restatement():
    off = np.array([[2, 0, 2, 5], [0, 2, -1, 6], [2, 2, 2, 2]])
    vseg, lst, bad = K.invert_lists(off, 6)
    assert bad == 2
    assert vseg.tolist() == [[0, 2], [2, 0], [2, 7], [9, 0], [9, 0], [9, 1]]
    assert lst.tolist() == [1, 4, 0, 2, 5, 8, 9, 10, 11, 3]


def test_slice_entry_points_exported():
    from efgh_amd import build
    so = build.build()
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'efgh_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(so)
    for n in ('efgh_slice', 'efgh_slice_bwd', 'efgh_offsets_invert', 'efgh_offsets_invert_workspace', 'efgh_slice_bwd_workspace'):
        assert re.search(r'\b' + n + r'\s*\(', hdr), n
        assert hasattr(lib, n), n
    lib.efgh_version.restype = ctypes.c_int
    assert lib.efgh_version() == 4
    lib.efgh_offsets_invert_workspace.restype = ctypes.c_int64
    lib.efgh_slice_bwd_workspace.restype = ctypes.c_int64
    assert lib.efgh_offsets_invert_workspace(ctypes.c_int32(1000), ctypes.c_int32(300)) >= 4 * 300 + 16 * 1000
    assert lib.efgh_slice_bwd_workspace(ctypes.c_int32(64)) >= 4 * 64
    # argument validation before any device work
    assert lib.efgh_slice(*([None] * 12)) == -1
    assert lib.efgh_slice_bwd(*([None] * 15)) == -1
    assert lib.efgh_offsets_invert(*([None] * 8)) == -1


def test_module_refusals():
    from efgh_amd._C import EfghError
    from efgh_amd.nets import BilateralConvFlex
    with pytest.raises(EfghError, match='d = 2'):
        BilateralConvFlex(8, [8], d=2)
    with pytest.raises(EfghError, match='multiples of 4'):
        BilateralConvFlex(6, [8])
    with pytest.raises(EfghError, match='multiples of 4'):
        BilateralConvFlex(8, [8, 6], do_slice=True)
    with pytest.raises(EfghError, match='radius'):
        BilateralConvFlex(8, [8], 4)
    with pytest.raises(EfghError, match='CPU tensor'):
        BilateralConvFlex(8, [8], do_slice=True)(torch.zeros(16, 8), None)
