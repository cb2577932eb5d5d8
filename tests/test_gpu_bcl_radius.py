"""BCL neighbourhood radius 2 and 3 on the GPU: neighbour tables bit-exact with the reference (every build path, batches, the
aliasing scene), the radius-r blur forward / data gradient / weight gradient against float64 torch on the same table, the E net
against the reference's outputs and gradients, batch and run-to-run determinism, and the whole backbone in training."""
import os

import numpy as np
import pytest
import torch

from bcl_radius_tables import neighbor_table
from efgh_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'bcl_radius.npz')
SCALES = (1.0, 0.75, 0.5, 0.25, 0.125)
VARIANTS = ('r2', 'r3', 'mixed')
N = 2048


@pytest.fixture(scope='module')
def G():
    return np.load(GOLDEN)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _mask_bits(lv):
    """(h, t) of the taps the alias-mask words of lv's table mark"""
    F, nw = lv.F, (lv.F + 31) // 32
    words = lv.nbr[:, F:F + nw].cpu().numpy().view(np.uint32)
    bits = (words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    h, t = np.nonzero(bits.reshape(lv.H, nw * 32)[:, :F])
    return set(zip(h.tolist(), t.tolist()))


def _check_tables(lvs, G, radii, nbr_of, off_of, H_of, hits_of=None):
    for l, (lv, r) in enumerate(zip(lvs, radii)):
        assert lv.radius == r and lv.H == H_of(l), l
        assert lv.nbr.shape == (lv.H, lv.ld)
        assert np.array_equal(lv.nbr[:, :lv.F].cpu().numpy().T, nbr_of(l)), (r, l)
        assert np.array_equal(lv.off.cpu().numpy(), off_of(l)), (r, l)
        if hits_of is not None:
            assert _mask_bits(lv) == set(map(tuple, hits_of(l).tolist())), (r, l)
        pad = lv.nbr[:, lv.F + (lv.F + 31) // 32:]
        assert pad.numel() == 0 or int(pad.abs().max()) == 0


def _table(G, prefix, l, r):
    """the reference's [F][H] table of one level, rebuilt from the stored vertex keys (tests/bcl_radius_tables.py)"""
    from efgh_amd import lattice
    return neighbor_table(G[f'{prefix}keys{l}'], G[f'{prefix}kmin{l}'], G[f'{prefix}kmax{l}'], lattice.filter_offsets(r)[0])[0]


@pytest.mark.parametrize('tag', VARIANTS)
def test_tables_bit_exact_sweep(G, tag):
    from efgh_amd import lattice
    radii = [int(r) for r in G[f'{tag}.radii']]
    t3 = [_table(G, 'lat.', l, 3) for l in range(5)]
    pc = torch.from_numpy(syn.lidar_sweep(N, 3))[None].cuda()
    lattice._SIZES.clear()
    for _ in range(2):                                                      # level by level, then speculative
        lvs = lattice.build_pyramid_batched(pc, SCALES, radii)
        _check_tables(lvs, G, radii, lambda l: t3[l][G[f'{tag}.cols{l}']], lambda l: G[f'lat.off{l}'],
                      lambda l: int(G[f'lat.H{l}']))
        for l, lv in enumerate(lvs):
            assert len(_mask_bits(lv)) == int(G[f'{tag}.n_alias{l}'])


@pytest.mark.parametrize('r', (2, 3))
def test_tables_bit_exact_alias_scene(G, r):
    """a thin plane: the tables are bit-exact and the mask words mark exactly the reference's aliased hits (none on this scene)"""
    from efgh_amd import lattice
    pc = torch.from_numpy(G['alias.pc'])[None].cuda()
    lattice._SIZES.clear()
    for _ in range(2):
        lvs = lattice.build_pyramid_batched(pc, SCALES, [r] * 5)
        _check_tables(lvs, G, [r] * 5, lambda l: _table(G, f'alias.r{r}.', l, r), lambda l: G[f'alias.r{r}.off{l}'],
                      lambda l: int(G[f'alias.r{r}.H{l}']), lambda l: G[f'alias.r{r}.hits{l}'])


def test_tables_same_on_every_path_and_batched(monkeypatch):
    """speculative, level-by-level, forced-hash and big-bucket builds give the same radius-r tables; a batch of 3 equals 3 singles"""
    from efgh_amd import lattice
    radii = [2, 1, 3, 1, 2]
    pcs = [syn.lidar_sweep(4096, s) for s in (0, 5, 9)]
    pc = torch.from_numpy(np.stack(pcs)).cuda()
    lattice._SIZES.clear()
    ref = lattice.build_pyramid_batched(pc, SCALES, radii)                # level by level
    key = next(iter(lattice._SIZES))
    runs = [lattice.build_pyramid_batched(pc, SCALES, radii)]            # speculative
    lattice._BIG_LEVELS[key] = {0, 1, 2}
    runs.append(lattice.build_pyramid_batched(pc, SCALES, radii))
    lattice._HASH_LEVELS[key] = {0, 1, 2, 3, 4}
    runs.append(lattice.build_pyramid_batched(pc, SCALES, radii))
    assert {lv._mode[0] for lv in runs[-1]} == {'hash'}
    lattice._HASH_LEVELS[key], lattice._BIG_LEVELS[key] = set(), set()
    lattice._SIZES.clear()
    for run in runs:
        for u, v in zip(ref, run):
            assert u.H == v.H and torch.equal(u.nbr, v.nbr) and torch.equal(u.off, v.off)
    for b, p in enumerate(pcs):
        single = lattice.build_pyramid_batched(torch.from_numpy(p)[None].cuda(), SCALES, radii)
        for u, v in zip(ref, single):
            su = u.sample(b)
            assert su.H == v.H and torch.equal(su.nbr, v.nbr[:, :v.F]) and torch.equal(su.off, v.off)
            h0, h1 = u.seg[b], u.seg[b + 1]
            assert torch.equal(u.nbr[h0:h1, v.F:], v.nbr[:, v.F:])


def _blur_ref64(splat, nbr, F, w, b):
    """float64 torch: relu(sum_t W_t gather(splat, nbr[:, t]) + b)"""
    H = nbr.shape[0]
    s = torch.cat([splat.double(), torch.zeros(1, splat.shape[1], dtype=torch.float64, device=splat.device)], 0)
    idx = torch.where(nbr[:, :F] >= 0, nbr[:, :F].long(), torch.full_like(nbr[:, :F].long(), H))
    g = s[idx]                                                              # [H][F][C]
    return torch.einsum('hfc,ocf->ho', g, w.double()[..., 0]) + b.double()


@pytest.mark.parametrize('r', (2, 3))
def test_blur_kernels_against_float64(G, r):
    """forward, data gradient and weight gradient of the radius-r blur through the aliasing scene's level-0 table and the sweep's"""
    from efgh_amd import lattice, ops
    from efgh_amd.nets import layers as L
    import torch.nn as nn
    torch.manual_seed(0)
    for pcn in (G['alias.pc'], syn.lidar_sweep(N, 3)):
        lv = lattice.build_pyramid_batched(torch.from_numpy(pcn)[None].cuda(), SCALES, [r] * 5)[0]
        H, C, C0 = lv.H, 36, 32
        conv0, conv1 = nn.Conv2d(C, C0, (lv.F, 1)).cuda(), nn.Conv2d(C0, C0, 1).cuda()
        splat = torch.randn(H, C, device='cuda', requires_grad=True)
        before = list(ops.BLUR_R_HITS)
        with torch.no_grad():
            mid_ref = _blur_ref64(splat, lv.nbr, lv.F, conv0.weight, conv0.bias)
            mid = torch.empty(H, C0, device='cuda')
            ops.blur_r_gemm(splat, C, C, lv.F, ops.blur_r_pack(conv0.weight), C0, H, mid, C0, lv.nbr, bias=conv0.bias)
        assert _rel(mid.cpu(), mid_ref.cpu()) < 1e-5
        ctx = L.Ctx(True)
        out = L.blur_conv(ctx, splat, H, C, lv, conv0, conv1)
        gy = torch.randn_like(out)
        (out * gy).sum().backward()
        s64 = splat.detach().double().requires_grad_(True)
        w64, b64 = conv0.weight.detach().double().requires_grad_(True), conv0.bias.detach().double().requires_grad_(True)
        m64 = torch.relu(_blur_ref64(s64, lv.nbr, lv.F, w64, b64))
        o64 = m64 @ conv1.weight.detach().double()[..., 0, 0].t() + conv1.bias.detach().double()
        (o64 * gy.double()).sum().backward()
        assert _rel(out.detach().cpu(), o64.detach().cpu()) < 1e-5
        assert _rel(splat.grad.cpu(), s64.grad.cpu()) < 2e-4
        assert _rel(conv0.weight.grad.cpu(), w64.grad.cpu()) < 2e-4
        assert _rel(conv0.bias.grad.cpu(), b64.grad.cpu()) < 2e-4
        assert [a - b for a, b in zip(ops.BLUR_R_HITS, before)] == [2, 1, 1]


def _loss(r):
    w1 = torch.linspace(-1, 1, r['e_gn_sgn'].numel(), device=r['e_gn_sgn'].device).view_as(r['e_gn_sgn'])
    w2 = torch.linspace(1, 2, r['e_gn_abs'].numel(), device=r['e_gn_abs'].device).view_as(r['e_gn_abs'])
    return (r['e_gn_sgn'] * w1).sum() + (r['e_gn_abs'] * w2).sum()


def _enet(G, tag):
    import json
    from efgh_amd.nets.enet import Enet
    radii = [int(r) for r in G[f'{tag}.radii']]
    args = dict(syn.default_args((128, 256), 'cuda'), scale_map=[[s, r] for s, r in zip(SCALES, radii)])
    m = Enet(args)
    shapes = json.loads(str(G[f'{tag}.sd_shapes']))
    man = [['E.' + str(n), s, 'float32'] for n, s in zip(G[f'{tag}.sd_names'], shapes)
           if m.state_dict()[str(n)].dtype == torch.float32]
    sd = dict(m.state_dict())
    sd.update({k[2:]: v for k, v in syn.synthetic_state_dict(man, seed=1).items()})
    m.load_state_dict(sd, strict=True)
    return m.cuda(), sd


@pytest.mark.parametrize('tag', VARIANTS)
def test_enet_against_reference(G, tag):
    m, sd = _enet(G, tag)
    m.eval()
    pc = torch.from_numpy(syn.lidar_sweep(N, 3))[None].cuda()
    with torch.no_grad():
        r = m(pc)
    for k in ('e_gn_abs', 'e_gn_sgn', 'e_l'):
        assert _rel(r[k].cpu().numpy().reshape(G[f'{tag}.eval.{k}'].shape), G[f'{tag}.eval.{k}']) < 1e-4, k
    m.load_state_dict(sd, strict=True)
    m.train()
    r = m(pc)
    for k in ('e_gn_abs', 'e_gn_sgn'):
        assert _rel(r[k].detach().cpu().numpy().reshape(G[f'{tag}.train.{k}'].shape), G[f'{tag}.train.{k}']) < 2e-4, k
    _loss(r).backward()
    names = [str(n) for n in G[f'{tag}.param_names']]
    params = dict(m.named_parameters())
    gn = np.array([0.0 if params[n].grad is None else params[n].grad.double().norm().item() for n in names])
    ref = G[f'{tag}.grad_norm']
    skip = np.array([n.startswith('conv_gn_') and n.endswith('.bias') for n in names])
    assert np.abs(gn - ref)[~skip].max() <= 2e-3 * ref.max(), (np.abs(gn - ref)[~skip].max(), ref.max())
    for n in ('conv_in.0.0.weight', 'lin_gn_abs.weight', 'bcn3.blur_conv.2.bias', 'bcn5.blur_conv.0.bias'):
        assert _rel(params[n].grad.cpu().numpy(), G[f'{tag}.grad.{n}']) < 2e-3, n
    assert _rel(params['bcn1.blur_conv.0.weight'].grad[:2].cpu().numpy(), G[f'{tag}.grad.bcn1.blur_conv.0.weight[:2]']) < 2e-3


def test_batch_and_determinism(G):
    """radius 2 at B = 2 equals two single-sample runs; two training steps give bit-identical gradients"""
    m, sd = _enet(G, 'r2')
    m.eval()
    pcs = [syn.lidar_sweep(N, 3), syn.lidar_sweep(N, 11)]
    with torch.no_grad():
        rb = m(torch.from_numpy(np.stack(pcs)).cuda())
        for b, p in enumerate(pcs):
            rs = m(torch.from_numpy(p)[None].cuda())
            for k in ('e_gn_abs', 'e_gn_sgn'):
                assert _rel(rb[k][b].cpu(), rs[k][0].cpu()) < 1e-5, k
    grads = []
    for _ in range(2):
        m.load_state_dict(sd, strict=True)
        m.train()
        m.zero_grad()
        _loss(m(torch.from_numpy(np.stack(pcs)).cuda())).backward()
        grads.append([p.grad.clone() for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


@pytest.mark.parametrize('radii', ([2, 1, 3, 1, 2], [1] * 5))
def test_backbone_training_step(radii):
    """EFGHBackbone + EFGHCriterion + Trainer step with mixed radii: every parameter gets a finite gradient and the radius-r kernels
    ran (forward, data gradient, weight gradient of the three radius-r levels); at radius 1 they do not"""
    from efgh_amd import ops
    from efgh_amd.losses import EFGHCriterion
    from efgh_amd.nets import EFGHBackbone
    from efgh_amd.train import Trainer
    raw = (128, 256)
    args = dict(syn.default_args(raw, 'cuda'), scale_map=[[s, r] for s, r in zip(SCALES, radii)])
    torch.manual_seed(0)
    m = EFGHBackbone(args).cuda()
    tr = Trainer(m, EFGHCriterion(args), lr=1e-3)
    b = syn.make_batch(raw, 2048, 2)
    inp = [torch.from_numpy(b[k]).cuda() for k in ('pc', 'img', 'calib', 'A')]
    gt = {k: torch.from_numpy(v) for k, v in b['gt'].items()}
    before = list(ops.BLUR_R_HITS)
    losses, _ = tr.step(*inp, gt)
    assert torch.isfinite(losses['total'])
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    hits = [a - b for a, b in zip(ops.BLUR_R_HITS, before)]
    assert hits == ([0, 0, 0] if radii == [1] * 5 else [3, 3, 3]), hits
