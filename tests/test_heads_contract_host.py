"""tests/heads_contract.py without a GPU: the fold against `F.conv_transpose2d` in float64, the unfold against autograd and the adjoint
identity, the softmax pair against `torch.softmax` and its autograd, the layout functions against `permute`; every entry of MUTATIONS
fails on a case of the lists the GPU module runs; the fp32 yardstick of the softmax constant is recomputed and the derived ceilings hold
for an fp32 CPU evaluation of each formula; and the eight entry points refuse bad arguments before any launch."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_contract as HC  # noqa: E402
from heads_contract import U, cmp, out_size, view2  # noqa: E402


def _wcol(w):
    """layers._convt_wcol: row (kh*3+kw)*O+o = W[:, o, kh, kw]"""
    Cw, O = w.shape[:2]
    return w.reshape(Cw, O, 9).permute(2, 1, 0).reshape(9 * O, Cw)


@pytest.mark.parametrize('O', [1, 2, 3, 4])
@pytest.mark.parametrize('pad', [0, 1])
@pytest.mark.parametrize('opad', [0, 1])
def test_col2im_is_conv_transpose2d(O, pad, opad):
    torch.manual_seed(O * 10 + pad * 2 + opad)
    for B, Hin, Win in [(1, 1, 1), (2, 3, 5), (1, 4, 1)]:
        Cw = 8
        x = torch.randn(B, Cw, Hin, Win, dtype=torch.float64)
        w = torch.randn(Cw, O, 3, 3, dtype=torch.float64)
        scale, shift = torch.randn(4, dtype=torch.float64), torch.randn(4, dtype=torch.float64)
        Y = (x.permute(0, 2, 3, 1).reshape(-1, Cw) @ _wcol(w).t()).contiguous()
        Ho, Wo = out_size(Hin, pad, opad), out_size(Win, pad, opad)
        for act in (0, 1, 2):
            ref, S = HC.col2im(Y.reshape(-1), 9 * O, B, Hin, Win, Ho, Wo, O, pad, scale, shift, act, 0.2)
            want = F.conv_transpose2d(x, w, None, 2, pad, opad) * scale[:O, None, None] + shift[:O, None, None]
            want = want if act == 0 else (F.relu(want) if act == 1 else F.leaky_relu(want, 0.2))
            assert want.shape == (B, O, Ho, Wo)
            assert float((ref[..., :O].permute(0, 3, 1, 2) - want).abs().max()) < 1e-12
            assert float(ref[..., O:].abs().max()) == 0 if O < 4 else True
            assert bool((S >= ref.abs() - 1e-12).all())


@pytest.mark.parametrize('O', [1, 3, 4])
@pytest.mark.parametrize('pad,opad', HC.PAD_OPAD)
def test_im2col_is_the_gradient_of_col2im_and_its_adjoint(O, pad, opad):
    torch.manual_seed(O + pad)
    for B, Hin, Win in [(1, 1, 1), (2, 3, 4), (1, 1, 5)]:
        Ho, Wo = out_size(Hin, pad, opad), out_size(Win, pad, opad)
        ldy, ldg = HC.ceil4(9 * O) + 4, 8
        Y = torch.randn(B * Hin * Win * ldy, dtype=torch.float64, requires_grad=True)
        G = torch.randn(B * Ho * Wo * ldg, dtype=torch.float64)
        out, _ = HC.col2im(Y, ldy, B, Hin, Win, Ho, Wo, O, pad, None, None, 0, 0.0)
        g4 = view2(G, 0, ldg, B * Ho * Wo, 4).reshape(B, Ho, Wo, 4)
        lhs = (out * g4).sum()
        (dY,) = torch.autograd.grad(lhs, Y)
        un = HC.im2col(G.float(), ldg, B, Hin, Win, Ho, Wo, O, pad, ldy)
        assert un.dtype == torch.float32 and un.shape == (B * Hin * Win, ldy)
        assert torch.equal(un.double(), dY.reshape(-1, ldy).float().double())            # exact copy or zero; pad columns zero
        assert float(un[:, 9 * O:].abs().max()) == 0
        rhs = (view2(Y.detach(), 0, ldy, B * Hin * Win, ldy) * un.double()).sum()
        lhs32 = (out.detach() * g4.float().double()).sum()
        assert abs(float(lhs32 - rhs)) <= 1e-12 * float((out.detach().abs() * g4.abs()).sum() + 1)


def test_softmax_pair_is_torch_softmax_and_its_autograd():
    lg = torch.cat([HC.gen_logits(c) for c in HC.softmax_cases()])
    y0, y1, S0, S1 = HC.softmax2(lg[:, 0], lg[:, 1])
    want = torch.softmax(lg.double(), 1)
    for got, w in ((y0, want[:, 0]), (y1, want[:, 1])):
        nan = torch.isnan(w)
        assert torch.equal(torch.isnan(got), nan) and int(nan.sum()) >= 8
        assert float((got[~nan] - w[~nan]).abs().max()) < 1e-15
    # (+inf, 0), (-inf, -inf) and a NaN in one slot give NaN in both components, as torch.softmax does
    for a, c in ((float('inf'), 0.0), (float('-inf'), float('-inf')), (float('nan'), 0.0), (0.0, float('nan'))):
        r = HC.softmax2(torch.tensor([a]), torch.tensor([c]))
        assert bool(torch.isnan(r[0]).all()) and bool(torch.isnan(r[1]).all())
    r = HC.softmax2(torch.tensor([float('-inf')]), torch.tensor([0.0]))
    assert float(r[0]) == 0.0 and float(r[1]) == 1.0
    x = (3 * torch.randn(2, 2, 37, dtype=torch.float64)).requires_grad_(True)
    y = torch.softmax(x, 1)
    g = torch.randn_like(y)
    (dx,) = torch.autograd.grad((y * g).sum(), x)
    d0, d1, S0, S1 = HC.softmax2_bwd(y[:, 0].detach(), y[:, 1].detach(), g[:, 0], g[:, 1])
    assert float((d0 - dx[:, 0]).abs().max()) < 1e-14 and float((d1 - dx[:, 1]).abs().max()) < 1e-14
    ref, S = HC.softmax2_to_nchw_bwd(y.detach(), g, 2, 37, 7)
    assert ref.shape == (74, 7) and float(ref[:, 2:].abs().max()) == 0
    assert float((ref[:, :2].reshape(2, 37, 2).permute(0, 2, 1) - dx).abs().max()) < 1e-14
    # the heads: depth a copy, the mask the same softmax, channel 3 of dx +0.0, an absent gradient zeros
    xh = torch.randn(2 * 37 * 4)
    depth, mask, _ = HC.heads_fwd(xh, 2, 37)
    v = xh.reshape(2, 37, 4)
    assert torch.equal(depth, v[..., 0].reshape(-1))
    assert float((mask - torch.softmax(v[..., 1:3].double(), 2).permute(0, 2, 1)).abs().max()) < 1e-15
    dd = torch.randn(74)
    ref, S = HC.heads_bwd(y.detach().float(), g.float(), dd, 2, 37)
    assert torch.equal(ref[:, 0], dd.double()) and float(S[:, 0].abs().max()) == 0 and float(ref[:, 3].abs().max()) == 0
    assert float(HC.heads_bwd(y.detach().float(), None, None, 2, 37)[0].abs().max()) == 0
    assert float(HC.heads_bwd(y.detach().float(), None, dd, 2, 37)[0][:, 1:].abs().max()) == 0


def test_layout_functions_are_permute():
    for case in HC.LAYOUT_CASES:
        B, Cs, HW, Cd = case
        buf = HC.gen_planar(case)
        x = buf[HC.LAYOUT_OFF:HC.LAYOUT_OFF + B * Cs * HW].reshape(B, Cs, HW)
        got = HC.nchw_to_nhwc(buf, B, Cs, HW, Cd, HC.LAYOUT_OFF)
        want = torch.zeros(B, HW, Cd)
        want[..., :Cs] = x.permute(0, 2, 1)
        assert got.shape == (B * HW, Cd) and torch.equal(HC.bits(got), HC.bits(want.reshape(B * HW, Cd)))
        for ld in HC.nhwc_lds(Cs):
            rb = HC.gen_rows(B, Cs, HW, ld)
            r = view2(rb, HC.LAYOUT_OFF, ld, B * HW, Cs)
            back = HC.nhwc_to_nchw(rb, ld, B, Cs, HW, HC.LAYOUT_OFF)
            assert torch.equal(HC.bits(back), HC.bits(r[:, :Cs].reshape(B, HW, Cs).permute(0, 2, 1).contiguous()))
    f = HC.special_floats(64, 1)
    assert bool(torch.isnan(f).any()) and bool(((f == 0) & torch.signbit(f)).any()) and bool(((f != 0) & (f.abs() < 1e-38)).any())


# ------------------------------------------------------------------------------------------------ planted misreadings
def _failures(mut):
    """number of cases of the GPU module's lists on which the reference under `mut`, rounded to fp32 as a kernel's output is, fails cmp"""
    n = 0
    if mut in (None, 'tap_parity', 'pad_sign', 'last_col_dropped', 'opad_ignored'):
        for case in HC.col2im_cases():
            B, Hin, Win, O, pad, opad, ldy, ldo, affine, act = case
            buf, scale, shift = HC.gen_col2im(case)
            ref, S = HC.ref_col2im(case)
            got, _ = HC.col2im(buf, ldy, B, Hin, Win, out_size(Hin, pad, opad), out_size(Win, pad, opad), O, pad, scale, shift, act,
                               HC.SLOPE, HC.COL2IM_OFF, mut=mut)
            n += cmp('col2im', str(case), got.float(), ref, S) > 0
        for case in HC.im2col_cases():
            B, Hin, Win, O, pad, opad, ldg = case
            buf, off = HC.gen_im2col(case)
            a = (buf, ldg, B, Hin, Win, out_size(Hin, pad, opad), out_size(Win, pad, opad), O, pad, HC.ceil4(9 * O))
            n += cmp('copy', str(case), HC.im2col(*a, off, mut=mut), HC.im2col(*a, off)) > 0
    if mut in (None, 'channels_swapped', 'no_max_subtract', 'depth_into_ch1'):
        for case in HC.softmax_cases():
            B, HW, rot = case
            lg = HC.gen_logits(case)
            ref, S = HC.softmax2_to_nchw(lg.reshape(-1), 2, B, HW)
            n += cmp('softmax', str(case), HC.softmax2_to_nchw(lg.reshape(-1), 2, B, HW, mut=mut)[0].float(), ref, S) > 0
            x4 = torch.cat([torch.full((B * HW, 1), 0.25), lg, torch.full((B * HW, 1), HC.POISON)], 1).reshape(-1)
            d, m, S = HC.heads_fwd(x4, B, HW)
            dm, mm, _ = HC.heads_fwd(x4, B, HW, mut=mut)
            n += (cmp('softmax', str(case), mm.float(), m, S) + cmp('copy', str(case), dm, d)) > 0
    if mut in (None, 'bwd_without_dot', 'depth_into_ch1', 'channels_swapped'):
        for case in HC.bwd_cases():
            B, HW, kind = case
            y, dm, dd = HC.gen_bwd(case)
            ref, S = HC.softmax2_to_nchw_bwd(y, dm, B, HW, 4)
            n += cmp('softmax_bwd', str(case), HC.softmax2_to_nchw_bwd(y, dm, B, HW, 4, mut=mut)[0].float(), ref, S) > 0
            ref, S = HC.heads_bwd(y, dm, dd, B, HW)
            n += cmp('softmax_bwd', str(case), HC.heads_bwd(y, dm, dd, B, HW, mut=mut)[0].float(), ref, S) > 0
    if mut in (None, 'pad_channel_copied', 'plane_stride_Cd'):
        for case in HC.LAYOUT_CASES:
            B, Cs, HW, Cd = case
            buf = HC.gen_planar(case)
            n += cmp('copy', str(case), HC.nchw_to_nhwc(buf, B, Cs, HW, Cd, HC.LAYOUT_OFF, mut=mut),
                     HC.nchw_to_nhwc(buf, B, Cs, HW, Cd, HC.LAYOUT_OFF)) > 0
    return n


def test_the_reference_passes_its_own_comparison():
    assert _failures(None) == 0


@pytest.mark.parametrize('mut', HC.MUTATIONS)
def test_every_planted_misreading_fails_on_a_case_of_the_gpu_lists(mut):
    n = _failures(mut)
    print(mut, 'fails', n, 'cases')
    assert n >= 1


def test_cmp_rules():
    one, S = torch.ones(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64)
    nan, inf = float('nan'), float('inf')
    assert cmp('softmax', 't', torch.tensor([nan, inf, 1.0, 1.0]), torch.tensor([nan, inf, 1.0, 1.0], dtype=torch.float64), S) == 0
    assert cmp('softmax', 't', torch.tensor([nan, 1.0, inf, -inf]), torch.tensor([1.0, nan, 1.0, inf], dtype=torch.float64), S) == 4
    assert cmp('col2im', 't', torch.tensor([1 + 8 * 2.0 ** -23] * 4), one, S) == 4 and cmp('col2im', 't', torch.tensor([1 + 2.0 ** -23] * 4), one, S) == 0
    assert cmp('softmax', 't', torch.tensor([1e-38]), torch.tensor([0.0], dtype=torch.float64), torch.zeros(1)) == 0     # (the floor)
    assert cmp('softmax', 't', torch.tensor([2e-38]), torch.tensor([0.0], dtype=torch.float64), torch.zeros(1)) == 1
    assert cmp('copy', 't', torch.tensor([0.0]), torch.tensor([-0.0])) == 1 and cmp('copy', 't', torch.tensor([nan]), torch.tensor([nan])) == 0


# ------------------------------------------------------------------------------------------------ ceilings
def test_softmax_constant_lies_between_one_and_four_times_the_fp32_yardstick():
    t, three = HC.softmax_yardstick()
    print('fp32 CPU yardstick in S U: torch.softmax %.3f, three-line formula %.3f; constant %.3f' % (t, three, HC.CEIL['softmax'] / U))
    y = max(t, three)
    assert abs(y - HC.SOFTMAX_YARDSTICK) <= 0.02 * y, (y, HC.SOFTMAX_YARDSTICK)       # the figure written beside the constant
    assert y <= HC.CEIL['softmax'] / U <= 4 * y


def test_derived_ceilings_hold_for_an_fp32_cpu_evaluation():
    HC.OBSERVED.clear()
    for case in HC.col2im_cases():
        B, Hin, Win, O, pad, opad, ldy, ldo, affine, act = case
        buf, scale, shift = HC.gen_col2im(case)
        ref, S = HC.ref_col2im(case)
        got, _ = HC.col2im(buf, ldy, B, Hin, Win, out_size(Hin, pad, opad), out_size(Win, pad, opad), O, pad, scale, shift, act,
                           float(torch.tensor(0.2)), HC.COL2IM_OFF, dt=torch.float32)
        assert got.dtype == torch.float32 and cmp('col2im', 'fp32 cpu %s' % (case,), got, ref, S) == 0, case
    for case in HC.bwd_cases():
        B, HW, kind = case
        y, dm, dd = HC.gen_bwd(case)
        r0, r1, S0, S1 = HC.softmax2_bwd(y[:, 0], y[:, 1], dm[:, 0], dm[:, 1])
        g0, g1, _, _ = HC.softmax2_bwd(y[:, 0], y[:, 1], dm[:, 0], dm[:, 1], dt=torch.float32)
        assert cmp('softmax_bwd', 'fp32 cpu %s' % (case,), g0, r0, S0) == 0 and cmp('softmax_bwd', 'fp32 cpu %s' % (case,), g1, r1, S1) == 0
    print({k: v for k, v in HC.OBSERVED.items()})


# ------------------------------------------------------------------------------------------------ refusals (nothing launched)
A, A2, A3, A4, MIS = 0x10000, 0x20000, 0x30000, 0x40000, 0x10004        # fake pointers: a call that passed validation would fault


def _refused(rc, lib, src):
    msg = lib.efgh_last_error().decode()
    return rc == -1 and 'invalid argument' in msg and src in msg


@pytest.mark.parametrize('kw', [dict(O=0), dict(O=5), dict(ldy=17), dict(ldo=6), dict(ldo=0), dict(Y=None), dict(out=None), dict(out=MIS),
                                dict(out=A2 + 8), dict(B=0), dict(Wo=0)], ids=lambda kw: ','.join('%s=%s' % kv for kv in kw.items()))
def test_col2im_refuses_bad_arguments_before_any_device_work(kw):
    from efgh_amd import _C
    lib = _C.lib()
    a = dict(Y=A, ldy=18, B=1, Hin=2, Win=2, Ho=4, Wo=4, O=2, pad=1, out=A2, ldo=4)
    a.update(kw)
    rc = lib.efgh_convt_col2im(a['Y'], a['ldy'], a['B'], a['Hin'], a['Win'], a['Ho'], a['Wo'], a['O'], a['pad'], None, None, 0, 0.0,
                               a['out'], a['ldo'], None)
    assert _refused(rc, lib, 'thin.hip')


@pytest.mark.parametrize('kw', [dict(O=0), dict(O=5), dict(ldy=17), dict(G=None), dict(Ycol=None), dict(Hin=0)],
                         ids=lambda kw: ','.join('%s=%s' % kv for kv in kw.items()))
def test_im2col_refuses_bad_arguments_before_any_device_work(kw):
    from efgh_amd import _C
    lib = _C.lib()
    a = dict(G=A, ldg=4, B=1, Hin=2, Win=2, Ho=4, Wo=4, O=2, pad=1, Ycol=A2, ldy=20)
    a.update(kw)
    rc = lib.efgh_convt_im2col(a['G'], a['ldg'], a['B'], a['Hin'], a['Win'], a['Ho'], a['Wo'], a['O'], a['pad'], a['Ycol'], a['ldy'], None)
    assert _refused(rc, lib, 'thin.hip')


def test_softmax_and_heads_refuse_bad_arguments_before_any_device_work():
    from efgh_amd import _C
    lib = _C.lib()
    for x, ld, y, B, HW in [(A, 1, A2, 1, 4), (A, 0, A2, 1, 4), (None, 2, A2, 1, 4), (A, 2, None, 1, 4), (A, 2, A2, 0, 4), (A, 2, A2, 1, 0)]:
        assert _refused(lib.efgh_softmax2_to_nchw(x, ld, y, B, HW, None), lib, 'elementwise.hip')
    for x, d, m, B, HW in [(MIS, A2, A3, 1, 4), (A + 8, A2, A3, 1, 4), (None, A2, A3, 1, 4), (A, None, A3, 1, 4), (A, A2, None, 1, 4),
                           (A, A2, A3, 0, 4), (A, A2, A3, 1, 0)]:
        assert _refused(lib.efgh_heads_to_nchw(x, d, m, B, HW, None), lib, 'elementwise.hip')
    for y, dm, dd, B, HW, dx in [(A, A2, A3, 1, 4, MIS + 0x30000), (A, A2, A3, 1, 4, A4 + 8), (A, None, None, 1, 4, A4 + 4), (None, A2, A3, 1, 4, A4),
                                 (A, A2, A3, 1, 4, None), (A, A2, A3, 0, 4, A4), (A, A2, A3, 1, 0, A4)]:
        assert _refused(lib.efgh_heads_bwd(y, dm, dd, B, HW, dx, None), lib, 'backward.hip')
    for y, dy, B, HW, dx, ld in [(A, A2, 1, 4, A3, 1), (A, A2, 1, 4, A3, 0), (None, A2, 1, 4, A3, 2), (A, None, 1, 4, A3, 2), (A, A2, 1, 4, None, 2),
                                 (A, A2, 0, 4, A3, 2), (A, A2, 1, 0, A3, 2)]:
        assert _refused(lib.efgh_softmax2_bwd(y, dy, B, HW, dx, ld, None), lib, 'backward.hip')


def test_layout_converters_refuse_bad_arguments_before_any_device_work():
    from efgh_amd import _C
    lib = _C.lib()
    for x, y, B, Cs, HW, Cd in [(A, A2, 1, 4, 8, 3), (A, A2, 1, 0, 8, 4), (None, A2, 1, 3, 8, 4), (A, None, 1, 3, 8, 4), (A, A2, 0, 3, 8, 4),
                                (A, A2, 1, 3, 0, 4)]:
        assert _refused(lib.efgh_nchw_to_nhwc(x, y, B, Cs, HW, Cd, None), lib, 'elementwise.hip')
    for x, ld, y, B, Cs, HW in [(A, 3, A2, 1, 4, 8), (A, 4, A2, 1, 0, 8), (None, 4, A2, 1, 3, 8), (A, 4, None, 1, 3, 8), (A, 4, A2, 0, 3, 8),
                                (A, 4, A2, 1, 3, 0)]:
        assert _refused(lib.efgh_nhwc_to_nchw(x, ld, y, B, Cs, HW, None), lib, 'elementwise.hip')


def test_chain_ceilings_lie_between_one_and_four_times_the_fp32_cpu_run_of_the_same_modules():
    worst = HC.chain_yardstick()
    for fam, (e, label) in sorted(worst.items()):
        print('%-12s fp32 CPU against float64 CPU: %.3e (%s); ceiling %.3e' % (fam, e, label, HC.CHAIN_CEIL[fam]))
    assert set(worst) == set(HC.CHAIN_CEIL)
    for fam, (e, label) in worst.items():
        assert e <= HC.CHAIN_CEIL[fam] <= 4 * e, (fam, e, HC.CHAIN_CEIL[fam])
