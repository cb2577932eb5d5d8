"""The float64 contract of the F correlation head (tests/corr_contract.py) against independent evaluations, on the CPU: float64 torch
autograd of the reference expression at every case shape, on inputs with ties at both extrema; the two MFMA formulations (camera
segments, Toeplitz planes) rebuilt from the contract's re-layouts; and, for every listed mutation of the contract, an element at which
the mutant is further from the contract than the largest ceiling of the shape allows - which is what makes the comparison on the GPU
mean something."""
import pytest
import torch
import torch.nn.functional as F

import corr_contract as CC
from oracle import efgh_oracle as O

REL = 1e-12


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _close(a, b):
    return float((a - b).abs().max()) <= REL * max(float(b.abs().max()), 1e-300)


def contract_head(cam, rng, ds):
    """the whole head through the contract, float64 end to end -> dict(logit, score, dcam, drng, ...)"""
    wr = rng.shape[2]
    off = int(wr / 8)
    cam_mm, rng_mm = CC.minmax(cam), CC.minmax(rng)
    rp, _ = CC.normalise_pad(rng, rng_mm, off, wr + 2 * off)
    cam_n, _ = CC.normalise(cam, cam_mm)
    logit, S = CC.logits_from(rp, cam_n)
    s, _, _ = CC.score(logit, S)
    dl = ds.double() * s * (1 - s) / 16
    dcam_n, _, drp, _ = CC.corr_bwd(rp, cam_n, dl)
    drng_n, _ = CC.unpad(drp, wr, off)
    dcam, _ = CC.norm_bwd(cam, dcam_n, cam_mm)
    drng, _ = CC.norm_bwd(rng, drng_n, rng_mm)
    return dict(logit=logit, S_logit=S, score=s, dl=dl, rp=rp, cam_n=cam_n, dcam_n=dcam_n, drp=drp, dcam=dcam, drng=drng)


def autograd_head(cam, rng, ds):
    """fnet.py:57,64,78-81 per sample in float64, differentiated by torch"""
    wr = rng.shape[2]
    c64, r64 = _nchw(cam).double().requires_grad_(True), _nchw(rng).double().requires_grad_(True)
    logits = []
    for b in range(cam.shape[0]):
        c = c64[b:b + 1] / (c64[b].max() - c64[b].min())
        r = r64[b:b + 1] / (r64[b].max() - r64[b].min())
        logits.append(F.conv2d(O.circular_assign(r, int(wr / 8)), c).view(1, -1) / 16)
    logit = torch.cat(logits, 0)
    s = torch.sigmoid(logit)
    s.backward(ds.double())
    return dict(logit=logit.detach(), score=s.detach(), dcam=c64.grad.permute(0, 2, 3, 1), drng=r64.grad.permute(0, 2, 3, 1))


@pytest.mark.parametrize('case', CC.CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_contract_matches_float64_autograd(case):
    cam, rng, ds = CC.head_inputs(*case)
    # the inputs tie at both extrema: the plateau of sample 0 holds the minimum about n/3 times
    n = cam[0].numel()
    assert int((cam[0] == cam[0].min()).sum()) >= max(1, n // 3) and int((rng[0] == rng[0].min()).sum()) >= rng[0].numel() // 3
    if case[0] > 1:
        assert int((cam[1] == cam[1].max()).sum()) == 1 and int((cam[1] == cam[1].min()).sum()) == 1
        assert cam[1].flatten()[-1] == cam[1].max() and cam[1].flatten()[0] == cam[1].min()
    got, ref = contract_head(cam, rng, ds), autograd_head(cam, rng, ds)
    assert float(got['dl'].abs().max()) > 1e-4           # the sigmoid is not saturated: the backward has something to carry
    for k in ('logit', 'score', 'dcam', 'drng'):
        assert got[k].shape == ref[k].shape and _close(got[k], ref[k]), k


def test_minmax_takes_signed_zeros_as_equal():
    x = torch.tensor([[0.0, -0.0, 1.0, 0.0, -0.0, 2.0]])
    mm = CC.minmax(x)
    assert float(mm[0, 0]) == 0.0 and float(mm[0, 1]) == 2.0
    dx, S = CC.norm_bwd(x, torch.ones_like(x), mm)
    # T = 3, d = 2: four tied minima share +3/4, the maximum takes -3/4
    assert torch.equal(dx, torch.tensor([[0.5 + 0.1875] * 2 + [0.5] + [0.5 + 0.1875] * 2 + [0.5 - 0.75]], dtype=torch.float64))
    assert torch.equal(S, torch.tensor([[0.5 + 0.1875] * 2 + [0.5] + [0.5 + 0.1875] * 2 + [0.5 + 0.75]], dtype=torch.float64))


@pytest.mark.parametrize('case', [(2, 7, 33, 85), (1, 17, 65, 150), (3, 12, 37, 150), (2, 1, 1, 8)], ids=lambda c: 'x'.join(map(str, c)))
def test_relayouts_rebuild_both_mfma_formulations(case):
    """camera segments x row groups (efgh_corr_pack_cam, the mode-3 GEMM, efgh_corr_fold) and Toeplitz planes (efgh_corr_planes /
    _toeplitz / _unplanes around two plane GEMMs) give the contract's logit and gradients; paddings are zero"""
    B, h, wc, wr = case
    cam, rng, ds = CC.head_inputs(*case)
    g, ref = CC.geometry(h, wc, wr), contract_head(cam, rng, ds)
    wp, nj, segw, nseg, nsplit, T = g['wp'], g['nj'], g['segw'], g['nseg'], g['nsplit'], g['T']
    rpz, _ = CC.normalise_pad(rng, CC.minmax(rng), g['off'], wp + segw)
    assert float(rpz[:, :, wp:].abs().max()) == 0.0
    Wc, _ = CC.pack_cam(cam, CC.minmax(cam), segw, nseg, nsplit)
    assert Wc.shape == (B, nsplit, nseg, T, segw * 16)
    logit = torch.zeros((B, nj), dtype=torch.float64)
    for s in range(nseg):
        seg = Wc[:, :, s].reshape(B, h, segw, 16)
        if s >= g['nseg_real']:
            assert float(seg.abs().max()) == 0.0
        if s * segw + nj + segw - 1 <= wp + segw:
            logit += CC.logits_from(rpz[:, :, s * segw:s * segw + nj + segw - 1], seg)[0]
    assert _close(logit, ref['logit'])

    wpP, wcP = CC.ceil4(wp), CC.ceil4(wc)
    rp32, dl32 = ref['rp'].float(), ref['dl'].float()
    rpT, camT = CC.planes(rp32, None, wp, wpP), CC.planes(cam, CC.minmax(cam), wc, wcP)
    assert float(rpT[..., wp:].abs().sum()) == 0.0 and float(camT[..., wc:].abs().sum()) == 0.0
    assert CC.exact(CC.unplanes(rpT.float(), h, wp).float(), rp32.double()) == 0          # planes then unplanes: the identity
    Tz, TTz = CC.toeplitz(dl32, wc, wp, wpP, 0), CC.toeplitz(dl32, wp, wc, wcP, 1)
    assert float(Tz[..., wp:].abs().sum()) == 0.0 and float(TTz[..., wc:].abs().sum()) == 0.0
    assert torch.equal(TTz[..., :wc], CC.dl_toeplitz(dl32.double(), wc, wp))
    assert torch.equal(Tz[..., :wp], CC.dl_toeplitz(dl32.double(), wc, wp).transpose(1, 2))
    want = CC.corr_bwd(rp32.double(), ref['cam_n'], dl32.double())
    assert _close(CC.unplanes(rpT @ Tz.transpose(1, 2), h, wc), want[0])
    assert _close(CC.unplanes(camT @ TTz.transpose(1, 2), h, wp), want[2])


# ------------------------------------------------------------------------------------------------ discrimination
MUT_CASE = (2, 7, 33, 85)            # B > 1; off = int(10.6) = 10 != round; segw = 2; nsplit = 7 row groups of T = 1


def _mutant_logit(cam, rng, pad='contract', off=None, inv=16.0, drop_col=None, drop_rows=0):
    wr = rng.shape[2]
    off = int(wr / 8) if off is None else off
    xn, _ = CC.normalise(rng, CC.minmax(rng))
    left = torch.flip(xn[:, :, wr - off:], dims=[2]) if pad != 'left pad not mirrored' else xn[:, :, wr - off:]
    right = xn[:, :, :off] if pad != 'right pad mirrored' else torch.flip(xn[:, :, :off], dims=[2])
    cam_n, _ = CC.normalise(cam, CC.minmax(cam))
    if drop_col is not None:
        cam_n[:, :, drop_col] = 0
    if drop_rows:
        cam_n[:, cam_n.shape[1] - drop_rows:] = 0
    logit, S = CC.logits_from(torch.cat([left, xn, right], 2), cam_n)
    return logit * 16 / inv, S


def _mutant_norm_bwd(x, dxn, mm, kind):
    B = x.shape[0]
    xf, gf = x.reshape(B, -1).double(), dxn.reshape(B, -1).double()
    d = (mm[:, 1].double() - mm[:, 0].double()).view(B, 1)
    T = (gf * xf).sum(1, keepdim=True)
    out = gf / d
    for col, sign in ((1, -1.0), (0, 1.0)):
        tied = xf == mm[:, col].double().view(B, 1)
        if kind == 'all tie mass given to the first tied element':
            first = torch.zeros_like(tied)
            first[torch.arange(B), tied.int().argmax(1)] = True
            tied = first
        out = out + sign * tied * (T / (d * d))           # 'tie count ignored': k = 1 on every tied element
    return out.reshape(x.shape)


MUTANTS = ['left pad not mirrored', 'right pad mirrored', 'off = round(wr/8)', 'all tie mass given to the first tied element',
           'tie count ignored (k = 1)', '1/16 replaced by 1/(16 B)', 'one camera column dropped at a segment boundary',
           'last row group dropped']


@pytest.mark.parametrize('mutant', MUTANTS)
def test_ceilings_separate_the_mutant(mutant):
    B, h, wc, wr = MUT_CASE
    cam, rng, ds = CC.head_inputs(*MUT_CASE)
    g = CC.geometry(h, wc, wr)
    if 'tie' in mutant:
        ref = contract_head(cam, rng, ds)
        seen = 0
        for x, dxn in ((cam, ref['dcam_n']), (rng, CC.unpad(ref['drp'], wr, g['off'])[0])):
            mm = CC.minmax(x)
            want, S = CC.norm_bwd(x, dxn, mm)
            got = _mutant_norm_bwd(x, dxn, mm, mutant)
            seen += int(((got - want).abs() > CC.ceil_norm(x[0].numel()) * S + CC.DELTA).sum())
        assert seen > 0
        return
    kw = {'left pad not mirrored': dict(pad=mutant), 'right pad mirrored': dict(pad=mutant), 'off = round(wr/8)': dict(off=round(wr / 8)),
          '1/16 replaced by 1/(16 B)': dict(inv=16.0 * B), 'one camera column dropped at a segment boundary': dict(drop_col=g['segw']),
          'last row group dropped': dict(drop_rows=g['T'])}[mutant]
    assert round(wr / 8) != int(wr / 8) and g['segw'] > 1 and B > 1 and g['off'] >= 2
    want, S = CC.logits(cam, rng)
    got, _ = _mutant_logit(cam, rng, **kw)
    nj = min(want.shape[1], got.shape[1])
    ceiling = max(CC.ceil_logit(True, h, wc, wr), CC.ceil_logit(False, h, wc, wr))
    assert int(((got[:, :nj] - want[:, :nj]).abs() > ceiling * S[:, :nj] + CC.DELTA).sum()) > 0


def test_unmutated_helpers_are_the_contract():
    """the mutants' scaffolding with no mutation switched on reproduces the contract bit for bit (so a separation is the mutation's)"""
    cam, rng, ds = CC.head_inputs(*MUT_CASE)
    assert torch.equal(_mutant_logit(cam, rng)[0], CC.logits(cam, rng)[0])


def test_ceilings_are_small_multiples_of_the_unit_roundoff():
    assert CC.CEIL_ELEM <= 8 * CC.U and CC.CEIL_UNPAD <= 8 * CC.U and CC.CEIL_SIGMOID <= 8 * CC.U
    for B, h, wc, wr in CC.CASES:
        g = CC.geometry(h, wc, wr)
        assert CC.ceil_logit(False, h, wc, wr) == (wc + h + CC.C_OPERANDS) * CC.U
        assert CC.ceil_logit(True, h, wc, wr) == (g['T'] * g['segw'] * 16 + g['nsplit'] * g['nseg'] + CC.C_OPERANDS) * CC.U
        assert g['nseg_real'] <= 32 and g['nseg'] * g['segw'] >= wc
    assert CC.minmax_groups(2048) == 1 and CC.minmax_groups(2052) == 2 and CC.minmax_groups(2099200) == 1024
    assert CC.ceil_norm(2099200) == (9 + 19) * CC.U and CC.ceil_norm(16) == 20 * CC.U
