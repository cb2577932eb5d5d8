"""Golden data of the reference's BilateralConvFlex layer (nets/bilateralNN.py:55-263: splat, blur stack, slice, bias), run
UNMODIFIED on the CPU through ref_harness.py.
Run:  python tests/golden/make_golden_bcl_layer.py  ->  tests/golden/bcl_layer.npz (data only; inputs and weights are regenerated
from seeds by tests/bcl_layer_contract.py).

Lattice: the reference's GenerateData on syn.lidar_sweep(2048, 3), level 0 (scale 1.0) and level 3 (scale 0.25: few vertices, long
lists); radius 2 for variant d.  The five variants are bcl_layer_contract.VARIANTS (B = 1):
    a   8 -> [16, 12], splat + slice + bias, use_norm, no last activation, radius 1, level 0
    b   8 -> [12] (a single convolution), last_relu + use_leaky, slice, no bias, no normalisation, level 3
    c   8 -> [8, 8, 4], last_relu without leaky, do_splat=False (random [H][8] lattice rows), slice + bias onto 777 points drawn
        with repetition from the level's points (bary[:, idx], off[:, idx]), level 0
    d   radius 2, 8 -> [16, 16], splat + slice + bias, level 0
    e   do_splat=False, do_slice=False, 8 -> [16, 8], level 3
Stored per variant: state-dict names and shapes, the eval output, the gradients of the scalar loss (out * linspace(-1, 1)).sum()
w.r.t. the input and every parameter - as ROWS [n][C] (the reference's (1, C, n) transposed) - and for every stored quantity
`err.<key>`: the reference's own float32 error against the float64 restatement (bcl_layer_contract.layer_ref), max |ref - f64| /
max |f64|, asserted finite and below 1e-4 here.  Per-point / per-vertex arrays keep every row_stride(n)-th row (at most 256 rows
each): the full arrays would be 0.7 MB of floats that do not compress.  The recorded rows can therefore only catch a deviation
that shows on the kept rows; the `err.*` figures are taken over the FULL arrays, and the GPU test checks every row against the
float64 restatement, which the host test ties to these recorded rows.  `off0` / `off3` (int16: every vertex index fits) and `idx` are stored whole."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import ref_harness as rh            # noqa: E402
import bcl_layer_contract as K      # noqa: E402
from efgh_amd import synthetic as syn  # noqa: E402

torch.set_num_threads(1)
nets, losses, tu = rh.import_reference()
import nets.generate_data as gdm    # noqa: E402
from nets.bilateralNN import BilateralConvFlex  # noqa: E402


def lattice(pc, radius):
    gd = gdm.GenerateData(3, [[s, radius] for s in K.SCALES], 'cpu')
    _, gen = gd(torch.from_numpy(pc))
    return gen


def main():
    store = {}
    pc = syn.lidar_sweep(K.N_POINTS, K.SCENE_SEED)
    gens = {r: lattice(pc, r) for r in (1, 2)}
    for l in (0, 3):
        store[f'off{l}'] = gens[1][l]['pc1_lattice_offset'][0].numpy().astype(np.int16)
        store[f'H{l}'] = np.int64(gens[1][l]['pc1_hash_cnt'])
        assert np.array_equal(store[f'off{l}'], gens[2][l]['pc1_lattice_offset'][0].numpy())
    for tag, v in K.VARIANTS.items():
        g = gens[v['radius']][v['level']]
        bary, off, nbr, H = g['pc1_barycentric'], g['pc1_lattice_offset'], g['pc1_blur_neighbors'], int(g['pc1_hash_cnt'])
        n_in = bary.shape[-1]
        m = BilateralConvFlex(3, v['radius'], v['num_input'], v['num_output'], 'cpu', v['use_bias'], v['use_leaky'], v['use_norm'],
                              v['do_splat'], v['do_slice'], v['last_relu'])
        names = list(m.state_dict().keys())
        shapes = [list(t.shape) for t in m.state_dict().values()]
        store[f'{tag}.sd_names'] = np.array(names)
        store[f'{tag}.sd_shapes'] = np.array(json.dumps(shapes))
        sd = dict(m.state_dict())
        sd.update(K.variant_weights(tag, names, shapes))
        m.load_state_dict(sd, strict=True)
        m.eval()
        rows = n_in if v['do_splat'] else H
        x_rows = K.variant_input(tag, rows, v['num_input'])
        x = torch.from_numpy(x_rows.T.copy())[None].requires_grad_(True)              # (1, C, rows)
        ob = oo = None
        if v['do_slice']:
            ob, oo = bary, off
            if v['select']:
                idx = K.select_idx(n_in)
                store['idx'] = idx
                ob, oo = bary[:, :, idx], off[:, :, idx]
        out = m(x, bary, off, nbr, ob, oo)                                          # (1, C_last, n_out)
        w = torch.linspace(-1, 1, out.numel()).view_as(out)
        (out * w).sum().backward()
        got = {'out': out.detach()[0].t().numpy(), 'grad.input': x.grad[0].t().numpy()}
        for name, p in m.named_parameters():
            got['grad.' + name] = p.grad.numpy()
        # ---- the float64 restatement on the same data
        lat = dict(H=H, bary=bary[0].t().double(), off=off[0].t().long(), nbr=nbr[0].t().long())
        p64 = {k: t.double().requires_grad_(True) for k, t in sd.items() if t.dtype == torch.float32}
        x64 = torch.from_numpy(x_rows).double().requires_grad_(True)
        o64 = K.layer_ref(v, p64, x64, lat, None if ob is None else ob[0].t().double(), None if oo is None else oo[0].t().long())
        (o64 * K.loss_weights(o64.shape[1], o64.shape[0])).sum().backward()
        want = {'out': o64.detach().numpy(), 'grad.input': x64.grad.numpy()}
        for name in got:
            if name.startswith('grad.') and name != 'grad.input':
                want[name] = p64[name[5:]].grad.numpy()
        for name, val in got.items():
            ref = want[name]
            assert val.shape == ref.shape, (tag, name, val.shape, ref.shape)
            err = float(np.abs(val.astype(np.float64) - ref).max() / np.abs(ref).max())
            assert np.isfinite(err) and err < 1e-4, (tag, name, err)
            store[f'err.{tag}.{name}'] = np.float64(err)
            if name in ('out', 'grad.input'):
                val = val[::K.row_stride(val.shape[0])]
            store[f'{tag}.{name}'] = val.astype(np.float32)
        print(tag, 'H', H, 'n_in', n_in, {k: '%.1e' % float(store[f'err.{tag}.{k}']) for k in got})
    path = os.path.join(HERE, 'bcl_layer.npz')
    np.savez_compressed(path, **store)
    print('bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
