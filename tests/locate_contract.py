"""What tests/golden/locate.npz holds and how its inputs are regenerated (test helper, shared by make_golden_locate.py,
test_locate_host.py and test_gpu_locate.py): the query of ARBITRARY points on a built lattice level (OutPoints.locate,
efgh_lattice_locate) against the reference's own get_keys_and_barycentric (nets/generate_data.py:56-112).

Scene: syn.lidar_sweep(N_POINTS, SCENE_SEED).  One single-level reference lattice per scale of SCALES (the scale applies at
whichever level it is used, so a one-level pyramid at 0.25 is a legitimate lattice).  Query sets, N_QUERY points each:
    self    the scene's first points                       every corner found, off = the build's own lattice_offset
    other   a second sweep (seed 4)                        at scale 1.0 points with 0, 1, 2, 3 and 4 corners found
    jit     the scene + N(0, 0.3) noise (RandomState 11)    mostly found
    far     the scene times 3                               mostly outside the lattice's key box
    alias   stored in the file (built from the reference's keys): points around k + delta for vertices k, where delta leaves
            key2int (transforms.py:62-77, no range check) unchanged: a corner whose KEY INTEGER is a vertex's but whose key is
            not - a query that forms the key integer before testing the key against the key box returns a wrong vertex there
Per scale tag t ('s100' / 's025') and set: '<t>.<set>.bary' [n][4] float32, '<t>.<set>.off' [n][4] int16 (-1 = the lattice has no
such vertex: looked up key tuple -> pc1_lattice_offset), '<t>.<set>.missing' = (absent corners, points without any corner);
'<t>.H', '<t>.lattice_offset' [N_QUERY][4] (pc1_lattice_offset of the scene's first points, as the reference stores it),
'<t>.alias.pts' (3, n), '<t>.alias.mask' [n][4] (1 = the aliased corner); '<t>.<set>.classes2048' = points by number of corners
found (0..4) and '<t>.<set>.outbox2048' = corners outside the key box, over all N_POINTS points of the set."""
import numpy as np

SCALES = (1.0, 0.25)
N_POINTS, SCENE_SEED, OTHER_SEED, N_QUERY = 2048, 3, 4, 512
SETS = ('self', 'other', 'jit', 'far')


def tag(s):
    return 's%03d' % round(100 * s)


def scene():
    from efgh_amd import synthetic as syn
    return syn.lidar_sweep(N_POINTS, SCENE_SEED)


def query_full(name):
    """all N_POINTS points of a query set, (3, N_POINTS) float32"""
    from efgh_amd import synthetic as syn
    pc = scene()
    if name == 'self':
        return pc
    if name == 'other':
        return syn.lidar_sweep(N_POINTS, OTHER_SEED)
    if name == 'jit':
        return pc + np.random.RandomState(11).normal(0, 0.3, pc.shape).astype(np.float32)
    if name == 'far':
        return pc * np.float32(3)
    raise KeyError(name)


def query(name):
    """the N_QUERY points of a set that the file stores answers for"""
    return np.ascontiguousarray(query_full(name)[:, :N_QUERY])


def masked(bary, off):
    """(bary, off) with every absent corner turned into weight 0 on row 0: the same sums for restatements that index with off"""
    bary, off = np.array(bary, copy=True), np.array(off, copy=True).astype(np.int64)
    gone = off < 0
    bary[gone] = 0
    off[gone] = 0
    return bary, off


def layer_eval(cfg, params, feat, lat, out_bary, out_off, dtype):
    """bcl_layer_contract.layer_ref evaluated in `dtype` (torch.float64: the same numbers, checked by test_locate_host.py;
    torch.float32: the restatement's own float32 error, what the GPU layer's error is measured against).  Same arguments; every
    tensor is cast to dtype here"""
    import torch
    H, nbr = lat['H'], lat['nbr']
    feat = feat.to(dtype)
    params = {k: v.to(dtype) for k, v in params.items()}
    C = feat.shape[1]
    if cfg['do_splat']:
        b, o = lat['bary'].to(dtype), lat['off'].reshape(-1)
        v = (b[:, :, None] * feat[:, None, :]).reshape(-1, C)
        x = torch.zeros(H, C, dtype=dtype).index_add(0, o, v)
        if cfg['use_norm']:
            w = torch.zeros(H, dtype=dtype).index_add(0, o, b.reshape(-1))
            x = x * (1.0 / (w + 1e-5))[:, None]
    else:
        x = feat
    convs = sorted({int(k.split('.')[1]) for k in params if k.startswith('blur_conv.')})
    for j, i in enumerate(convs):
        w, bi = params['blur_conv.%d.weight' % i], params['blur_conv.%d.bias' % i]
        if j == 0:
            s = torch.cat([x, torch.zeros(1, C, dtype=dtype)], 0)
            g = s[torch.where(nbr >= 0, nbr, torch.full_like(nbr, H))]
            x = torch.einsum('hfc,ocf->ho', g, w[..., 0]) + bi
        else:
            x = x @ w[:, :, 0, 0].t() + bi
        if j < len(convs) - 1:
            x = torch.relu(x)
        elif cfg['last_relu']:
            x = torch.nn.functional.leaky_relu(x, 0.1) if cfg['use_leaky'] else torch.relu(x)
    if not cfg['do_slice']:
        return x
    x = (out_bary.to(dtype)[:, :, None] * x[out_off]).sum(1)
    if cfg['use_bias']:
        x = x + params['bias']
    return x


def layer_grads(cfg, weights, x_np, lat, out_bary, out_off, dtype):
    """out and the gradients of (out * bcl_layer_contract.loss_weights).sum() w.r.t. the input and every parameter, evaluated in
    dtype -> {'out', 'grad.input', 'grad.<parameter>'} as float64 numpy arrays"""
    import torch
    import bcl_layer_contract as K
    p = {k: t.to(dtype).requires_grad_(True) for k, t in weights.items()}
    x = torch.from_numpy(x_np).to(dtype).requires_grad_(True)
    o = layer_eval(cfg, p, x, lat, out_bary, out_off, dtype)
    (o * K.loss_weights(o.shape[1], o.shape[0]).to(dtype)).sum().backward()
    out = {'out': o.detach().double().numpy(), 'grad.input': x.grad.double().numpy()}
    out.update({'grad.' + k: t.grad.double().numpy() for k, t in p.items()})
    return out
