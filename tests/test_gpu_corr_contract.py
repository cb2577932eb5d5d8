"""The F correlation head against the float64 contract of tests/corr_contract.py, element by element, on every route.

(a) The head at ten shapes, each four ways (eval / training, USE_MFMA_CORR on / off).  ops._L is wrapped by a recording proxy for the
    call: the set of correlation entry points that ran is asserted against what the selection rules of ops.corr_head / ops.corr1d_bwd
    give for the shape.  The forward (logit, score) is compared from the raw feature maps; the backward stage by stage, each stage
    against the contract on the fp32 operands it was actually given (rp, dcam_n, drp, drng_n, then dcam and drng), after which
    FN.CorrHeadFn's own score and gradients must be bit-equal to that staged chain - so every element of dcam and drng is held to
    tau * S of its own stage, and no stage hides behind the norm of a later one.  A second run is bit-identical.
(b) ops.minmax / ops.norm_bwd alone: the scalar path, one group, two groups, the cap at 1024 groups; the extremum in the first
    element, the last, and inside the last chunk; tie counts 1, 2 and n/3; all-positive, all-negative data, a minimum of mixed zeros.
(c) The re-layout kernels into oversized sentinel-filled buffers: payload per contract, padding exactly zero, everything outside the
    declared extent bit-unchanged.
The last test asserts that the eleven entry points all ran and prints the table the taus of corr_contract.TAU were taken from.

On the MI355X (60 tests, about 4 s), largest |got - ref| / S per class: re-layouts with 1/d 1.11 x 2^-24, logit 1.53, sigmoid 1.95,
correlation gradients 9.80, fold of the pad 1.00, gradient of the normalisation 1.31."""
import contextlib
import ctypes

import pytest
import torch

import corr_contract as CC

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENT = -7777.0
REQUIRED = list(CC.ENTRY_POINTS)
REACHED = set()
_QUERIES = ('_groups', 'efgh_last_error', 'efgh_version')


class _Proxy:
    """ops._L() stand-in: forwards every attribute of the library and records the efgh_* entry points that are fetched to be called"""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name.startswith('efgh_') and not any(q in name for q in _QUERIES):
            self._calls.append(name)
            REACHED.add(name)
        return f


@contextlib.contextmanager
def recording(mfma=None):
    """ops._L replaced by a recording proxy and, with `mfma` given, ops.USE_MFMA_CORR set; both restored whatever happens"""
    from efgh_amd import ops
    real, old, calls = ops._L, ops.USE_MFMA_CORR, []
    proxy = _Proxy(real(), calls)
    ops._L = lambda: proxy
    if mfma is not None:
        ops.USE_MFMA_CORR = mfma
    try:
        yield calls
    finally:
        ops._L, ops.USE_MFMA_CORR = real, old


def expected_route(train, flag, h):
    """the correlation entry points ops.corr_head (and, in training, ops.corr1d_bwd and the rest of CorrHeadFn.backward) must call:
    the MFMA forward with the flag on, in training only from h * 16 >= 128 (where its backward is on the MFMA as well); the backward
    on the MFMA with the flag on from h * 16 >= 128, or whenever the forward left rp with the MFMA pitch"""
    fwd_mfma = flag and (not train or h * 16 >= 128)
    names = {'efgh_minmax', 'efgh_corr_pad'} | ({'efgh_corr_pack_cam', 'efgh_corr_fold'} if fwd_mfma else {'efgh_corr1d'})
    bwd_mfma = (flag and h * 16 >= 128) or fwd_mfma
    if train:
        names |= {'efgh_corr_planes', 'efgh_corr_toeplitz', 'efgh_corr_unplanes'} if bwd_mfma else {'efgh_corr1d_bwd'}
        names |= {'efgh_corr_unpad', 'efgh_norm_bwd'}
    return names, fwd_mfma, bwd_mfma


def head_calls(calls):
    return {c for c in calls if c in CC.ENTRY_POINTS}


def _ids(c):
    return 'x'.join(map(str, c))


def check_forward(label, case, mfma, cam, rng, logit, score):
    B, h, wc, wr = case
    ref, S = CC.logits(cam, rng)
    ceiling = CC.ceil_logit(mfma, h, wc, wr)
    assert logit.shape == ref.shape and score.shape == ref.shape
    assert CC.cmp('logit', label, logit, ref, S, ceiling) == 0, (label, CC.OBSERVED['logit'])
    # the score given the kernel's own logit: its own roundings only (this is what tau['sigmoid'] is taken from) ...
    own = torch.sigmoid(logit.double())
    assert CC.cmp('sigmoid', label, score, own, own, CC.CEIL_SIGMOID) == 0, (label, CC.OBSERVED['sigmoid'])
    # ... and from the raw inputs: the logit's bound through the largest slope of the sigmoid, plus those roundings
    s, S4, Ss = CC.score(ref, S)
    bound = CC.tau_of('logit', ceiling) * S4 + CC.tau_of('sigmoid', CC.CEIL_SIGMOID) * Ss + CC.DELTA
    assert int(((score.double() - s).abs() > bound).sum()) == 0, label


# ------------------------------------------------------------------------------------------------ (a) the head on every route
@pytest.mark.parametrize('mfma', [True, False], ids=['mfma', 'valu'])
@pytest.mark.parametrize('case', CC.CASES, ids=_ids)
def test_head_eval(case, mfma):
    from efgh_amd import ops
    B, h, wc, wr = case
    cam, rng, _ = (t.to(DEV) for t in CC.head_inputs(*case))
    with recording(mfma) as calls:
        score, logit = ops.corr_head(cam, rng, want_logit=True)
        score2, logit2 = ops.corr_head(cam, rng, want_logit=True)
    torch.cuda.synchronize()
    want, fwd_mfma, _ = expected_route(False, mfma, h)
    assert head_calls(calls) == want and fwd_mfma == mfma
    assert torch.equal(score, score2) and torch.equal(logit, logit2)
    check_forward('eval %s %s' % (_ids(case), 'mfma' if mfma else 'valu'), case, fwd_mfma, cam, rng, logit, score)


@pytest.mark.parametrize('mfma', [True, False], ids=['mfma', 'valu'])
@pytest.mark.parametrize('case', CC.CASES, ids=_ids)
def test_head_training(case, mfma):
    from efgh_amd import ops
    from efgh_amd.nets import fn as FN
    B, h, wc, wr = case
    g = CC.geometry(h, wc, wr)
    off, wp = g['off'], g['wp']
    cam, rng, ds = (t.to(DEV) for t in CC.head_inputs(*case))
    label = 'train %s %s' % (_ids(case), 'mfma' if mfma else 'valu')
    runs = []
    with recording(mfma) as calls:
        for _ in range(2):
            cg, rg = cam.clone().requires_grad_(True), rng.clone().requires_grad_(True)
            s = FN.CorrHeadFn.apply(cg, rg)
            s.backward(ds)
            runs.append((s.detach(), cg.grad, rg.grad))
    torch.cuda.synchronize()
    want, fwd_mfma, bwd_mfma = expected_route(True, mfma, h)
    assert head_calls(calls) == want
    for a, b in zip(*runs):
        assert torch.equal(a, b)

    # the same chain stage by stage (what CorrHeadFn does), every stage against the contract on the operands it was given
    with recording(mfma):
        score, logit, rp, cam_mm, rng_mm = ops.corr_head(cam, rng, want_logit=True, want_aux=True)
        dl = (ds * score * (1 - score) / 16.0).contiguous()
        dcam_n, drp = ops.corr1d_bwd(rp, cam, cam_mm, dl, B, h, wc, wp)
        drng_n = ops.corr_unpad(drp, B, h, wr, 16, off)
        dcam, drng = ops.norm_bwd(cam, dcam_n.contiguous(), cam_mm), ops.norm_bwd(rng, drng_n.contiguous(), rng_mm)
    torch.cuda.synchronize()
    assert torch.equal(score, runs[0][0]) and torch.equal(dcam, runs[0][1]) and torch.equal(drng, runs[0][2])
    assert float(dl.abs().max()) > 1e-4

    assert torch.equal(cam_mm, CC.minmax(cam)) and torch.equal(rng_mm, CC.minmax(rng))
    pitch = rp.shape[2]
    assert pitch == (wp + g['segw'] if fwd_mfma else wp)
    ref, S = CC.normalise_pad(rng, rng_mm, off, pitch)
    assert CC.cmp('elem', label + ' rp', rp, ref, S, CC.CEIL_ELEM) == 0
    assert int((rp[:, :, wp:] != 0).sum()) == 0
    check_forward(label, case, fwd_mfma, cam, rng, logit, score)

    cam_n, _ = CC.normalise(cam, cam_mm)
    r_dcam, S_dcam, r_drp, S_drp = CC.corr_bwd(rp[:, :, :wp].double(), cam_n, dl.double())
    c_dcam, c_drp = CC.ceil_corr_bwd(bwd_mfma, h, wc, wr)
    assert dcam_n.shape == r_dcam.shape and drp.shape == r_drp.shape
    assert CC.cmp('corr_bwd', label + ' dcam_n', dcam_n, r_dcam, S_dcam, c_dcam) == 0, CC.OBSERVED['corr_bwd']
    assert CC.cmp('corr_bwd', label + ' drp', drp, r_drp, S_drp, c_drp) == 0, CC.OBSERVED['corr_bwd']
    ref, S = CC.unpad(drp.double(), wr, off)
    assert CC.cmp('unpad', label, drng_n, ref, S, CC.CEIL_UNPAD) == 0, CC.OBSERVED['unpad']
    for name, x, dxn, mm, got in (('dcam', cam, dcam_n, cam_mm, dcam), ('drng', rng, drng_n, rng_mm, drng)):
        ref, S = CC.norm_bwd(x, dxn, mm)
        assert CC.cmp('norm', label + ' ' + name, got, ref, S, CC.ceil_norm(x[0].numel())) == 0, (name, CC.OBSERVED['norm'])


# ------------------------------------------------------------------------------------------------ (b) minmax / norm_bwd alone
def _where(n, place):
    if place == 'first':
        return 0
    if place == 'last':
        return n - 1
    return (n - 1) // 2048 * 2048 + ((n - 1) % 2048) // 2        # inside the last chunk of 2048, not at its end


def reduction_inputs(n, place, B):
    """[B][n] fp32 on quarter steps.  Sample 0: all positive, maximum once at `place`, minimum once at the mirrored position.
    Sample 1: all negative, maximum twice (one of them at `place`), minimum on every third element (about n/3 ties).
    Sample 2: non-negative, the minimum a mix of -0.0 and +0.0 (one of them at `place`), the maximum once"""
    p, q = _where(n, place), n - 1 - _where(n, place)
    x = torch.stack([CC.quantised((n,), 40 + b, 0.5) for b in range(B)])
    x[0] += 10.0
    x[0, p], x[0, q] = CC.HI + 10.25, CC.LO + 9.75
    x[1] -= 10.0
    x[1, 1::3] = CC.LO - 10.25
    x[1, p], x[1, (p + n // 2) % n] = CC.HI - 9.75, CC.HI - 9.75
    if B > 2:
        x[2] = x[2].clamp_min(0.25)
        x[2, 0::5], x[2, 2::5] = 0.0, -0.0
        x[2, p] = -0.0
        x[2, (p + 1) % n] = CC.HI + 0.25
    dxn = torch.stack([CC.quantised((n,), 50 + b, 0.5) for b in range(B)])
    return x.to(DEV), dxn.to(DEV)


@pytest.mark.parametrize('place', ['first', 'last', 'tail'])
@pytest.mark.parametrize('n', [16, 2048, 2052, 4099, 2099200])
def test_minmax_and_norm_bwd(n, place):
    from efgh_amd import ops
    B = 2 if n > 100000 else 3
    x, dxn = reduction_inputs(n, place, B)
    k = [(int((x[b] == x[b].max()).sum()), int((x[b] == x[b].min()).sum())) for b in range(B)]
    assert k[0] == (1, 1) and k[1][0] == 2 and k[1][1] >= (n - 2) // 3 - 2 and bool((x[0] > 0).all()) and bool((x[1] < 0).all())
    if B > 2:
        zeros = x[2][x[2] == 0]
        assert bool(torch.signbit(zeros).any()) and not bool(torch.signbit(zeros).all()) and float(x[2].min()) == 0.0
    with recording() as calls:
        G = int(ops._L().efgh_minmax_groups(ctypes.c_int64(n)))
        mm, mm2 = ops.minmax(x), ops.minmax(x)
        dx, dx2 = ops.norm_bwd(x, dxn, mm), ops.norm_bwd(x, dxn, mm)
    torch.cuda.synchronize()
    assert head_calls(calls) == {'efgh_minmax', 'efgh_norm_bwd'}
    assert G == CC.minmax_groups(n) == {16: 1, 2048: 1, 2052: 2, 4099: 3, 2099200: 1024}[n]
    ref_mm = CC.minmax(x)
    assert torch.equal(mm, ref_mm) and torch.equal(mm, mm2)          # (== : the sign of a zero minimum is not specified)
    nz = ref_mm != 0
    assert CC.exact(mm[nz], ref_mm[nz].double()) == 0
    assert torch.equal(dx, dx2)
    ref, S = CC.norm_bwd(x, dxn, mm)
    label = 'norm_bwd alone n=%d %s' % (n, place)
    assert CC.cmp('norm', label, dx, ref, S, CC.ceil_norm(n)) == 0, CC.OBSERVED['norm']


# ------------------------------------------------------------------------------------------------ (c) padding and write extents
TAIL = 192


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def i32(v):
    return ctypes.c_int32(int(v))


def sentinel(n):
    return torch.full((int(n) + TAIL,), SENT, dtype=torch.float32, device=DEV)


def tail_unchanged(buf, n):
    return int((buf[int(n):] != SENT).sum()) == 0 and buf.numel() == int(n) + TAIL


def _call(name, *args):
    from efgh_amd import _C, ops
    _C.check(getattr(ops._L(), name)(*args, _C.stream_ptr()))


@pytest.mark.parametrize('case', [(2, 7, 33, 85), (3, 12, 37, 150), (1, 3, 10, 8)], ids=_ids)
def test_padding_and_write_extents(case):
    from efgh_amd import ops
    B, h, wc, wr = case
    g = CC.geometry(h, wc, wr)
    off, wp, nj, segw, nseg, nsplit, T = g['off'], g['wp'], g['nj'], g['segw'], g['nseg'], g['nsplit'], g['T']
    cam, rng, ds = (t.to(DEV) for t in CC.head_inputs(*case))
    label = 'extents ' + _ids(case)
    with recording() as calls:
        cam_mm, rng_mm = ops.minmax(cam), ops.minmax(rng)

        # efgh_corr_pad, wpitch > wp: payload, zeros in wp .. wpitch - 1, nothing behind the last row
        wpitch = wp + segw + 3
        n = B * h * wpitch * 16
        buf = sentinel(n)
        _call('efgh_corr_pad', P(rng), P(rng_mm), i32(B), i32(h), i32(wr), i32(16), i32(off), i32(wpitch), P(buf))
        torch.cuda.synchronize()
        rp = buf[:n].view(B, h, wpitch, 16)
        ref, S = CC.normalise_pad(rng, rng_mm, off, wpitch)
        assert CC.cmp('elem', label + ' pad', rp, ref, S, CC.CEIL_ELEM) == 0
        assert int((rp[:, :, wp:] != 0).sum()) == 0 and tail_unchanged(buf, n)

        # efgh_corr_toeplitz, both transposes, colsP > cols: dl where 0 <= j < nj, zero elsewhere and for c >= cols
        dl = ds[:, :nj].contiguous()
        for rows, cols, tr in ((wc, wp, 0), (wp, wc, 1)):
            colsP = CC.ceil4(cols) + 4
            n = B * rows * colsP
            tb = sentinel(n)
            _call('efgh_corr_toeplitz', P(dl), i32(B), i32(nj), i32(rows), i32(cols), i32(colsP), i32(tr), P(tb))
            torch.cuda.synchronize()
            Tg = tb[:n].view(B, rows, colsP)
            assert CC.exact(Tg, CC.toeplitz(dl, rows, cols, colsP, tr)) == 0
            assert int((Tg[:, :, cols:] != 0).sum()) == 0 and tail_unchanged(tb, n)

        # efgh_corr_planes, w_in_pitch > w and wP > w: a copy without mm, times 1/d with mm; zero in [w, wP)
        for x, mm, w, pitch in ((rp, None, wp, wpitch), (rp, rng_mm, wp, wpitch), (cam, cam_mm, wc, wc), (cam, None, wc, wc)):
            wP = CC.ceil4(w) + 4
            n = B * h * 16 * wP
            pb = sentinel(n)
            _call('efgh_corr_planes', P(x), ctypes.c_void_p(0) if mm is None else P(mm), i32(B), i32(h), i32(w), i32(pitch), i32(wP),
                  P(pb))
            torch.cuda.synchronize()
            pl = pb[:n].view(B, h * 16, wP)
            ref = CC.planes(x, mm, w, wP)
            if mm is None:
                assert CC.exact(pl, ref) == 0
            else:
                assert CC.cmp('elem', label + ' planes', pl, ref, ref.abs(), CC.CEIL_ELEM) == 0
            assert int((pl[:, :, w:] != 0).sum()) == 0 and tail_unchanged(pb, n)

            # efgh_corr_unplanes back from the padded planes: a copy of the payload, exactly B * h * w * 16 floats written
            m = B * h * w * 16
            ub = sentinel(m)
            _call('efgh_corr_unplanes', P(pl), i32(B), i32(h), i32(w), i32(wP), P(ub))
            torch.cuda.synchronize()
            assert CC.exact(ub[:m].view(B, h, w, 16), CC.unplanes(pl, h, w)) == 0 and tail_unchanged(ub, m)

        # efgh_corr_pack_cam: payload / d, zero for x >= wc and in the padded segments
        n = B * nsplit * nseg * T * segw * 16
        wb = sentinel(n)
        _call('efgh_corr_pack_cam', P(cam), P(cam_mm), i32(B), i32(h), i32(wc), i32(segw), i32(nseg), i32(nsplit), P(wb))
        torch.cuda.synchronize()
        Wc = wb[:n].view(B, nsplit, nseg, T, segw * 16)
        ref, S = CC.pack_cam(cam, cam_mm, segw, nseg, nsplit)
        assert CC.cmp('elem', label + ' pack_cam', Wc, ref, S, CC.CEIL_ELEM) == 0
        beyond = CC.pack_cam(torch.ones_like(cam), torch.tensor([[0.0, 1.0]] * B, device=DEV), segw, nseg, nsplit)[0] == 0
        assert int(beyond.sum()) == B * h * (nseg * segw - wc) * 16 and int((Wc[beyond] != 0).sum()) == 0
        assert tail_unchanged(wb, n)
    assert {'efgh_corr_pad', 'efgh_corr_toeplitz', 'efgh_corr_planes', 'efgh_corr_unplanes', 'efgh_corr_pack_cam'} <= set(calls)


def test_corr1d_bwd_rejected_call_launches_nothing():
    """wc * 64 + nj * 4 > 64 KiB of LDS: the argument error comes back and neither output is touched"""
    from efgh_amd import _C, ops
    B, h, wc, wp = 1, 1, 1000, 2000
    rp, cam = torch.ones(B, h, wp, 16, device=DEV), torch.ones(B, h, wc, 16, device=DEV)
    mm, dl = torch.tensor([[0.0, 1.0]], device=DEV), torch.ones(B, wp - wc + 1, device=DEV)
    dcam, drp = sentinel(B * h * wc * 16), sentinel(B * h * wp * 16)
    rc = ops._L().efgh_corr1d_bwd(P(rp), P(cam), P(mm), P(dl), i32(B), i32(h), i32(wc), i32(wp), P(dcam), P(drp), _C.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and b'invalid argument' in ops._L().efgh_last_error()
    assert int((dcam != SENT).sum()) == 0 and int((drp != SENT).sum()) == 0


# ------------------------------------------------------------------------------------------------ coverage and the measured table
def test_every_entry_point_was_reached_and_report():
    missing = [n for n in REQUIRED if n not in REACHED]
    assert not missing, missing
    print()
    for cls in CC.TAU:
        ratio, label = CC.OBSERVED.get(cls, (float('nan'), '-'))
        print('%-9s observed %.4e (%6.2f x 2^-24)  tau %s  [%s]' % (cls, ratio, ratio / CC.U, CC.TAU[cls], label))
    for cls, tau in CC.TAU.items():
        assert cls in CC.OBSERVED
        assert tau is None or CC.OBSERVED[cls][0] <= tau
