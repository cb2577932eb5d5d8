"""Photometric jitter on the device (csrc/jitter.hip through efgh_amd.data.color_jitter / preproc_img) against the numpy contract
(tests/jitter_contract.py) and the Pillow fixture (tests/golden/jitter.npz), byte for byte: every comparison is == on uint8."""
import itertools
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jitter_contract as JC  # noqa: E402

pytestmark = pytest.mark.gpu

FACTORS = (0, 0.3, 1, 1.4, 2)
HUES = (0, 0.1, -0.1, 0.5, -0.5)
ALL4 = ('brightness', 'contrast', 'saturation', 'hue')
ALL4_FACTORS = {'brightness': 1.3, 'contrast': 0.6, 'saturation': 1.7, 'hue': -0.21}


@pytest.fixture(scope='module')
def fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, 'jitter.npz'))
    return {k: z[k] for k in z.files}


def _img(h, w, seed=0):
    return np.random.RandomState(1000 + seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _params(order, factors):
    from efgh_amd.data import JitterParams
    return JitterParams(order, factors)


def _run(img, order, factors):
    from efgh_amd.data import color_jitter
    dev = torch.from_numpy(img).cuda()
    out = color_jitter(dev, _params(order, factors))
    assert out.dtype == torch.uint8 and out.shape == dev.shape and out.is_cuda and out.data_ptr() != dev.data_ptr()
    assert np.array_equal(dev.cpu().numpy(), img)                        # the input is never written
    return out.cpu().numpy()


# 1x1, 1x2, 1x3, 64x64: a pixel count of each residue mod 4; 1x5, 37x53 (1961), 3x4099: one workgroup and several; 1030x1021 is past the
# 1024 partial sums (1024 pixels each), so the fold sees a full table and the sum kernel strides
@pytest.mark.parametrize('hw', [(1, 1), (1, 5), (37, 53), (64, 64), (3, 4099), (1, 2), (1, 3), (1030, 1021)])
def test_all_four_ops_match_the_contract_at_every_shape(hw):
    img = _img(*hw, seed=hw[1])
    for order in (('brightness', 'saturation', 'contrast', 'hue'), ('hue', 'contrast', 'brightness', 'saturation')):
        factors = [ALL4_FACTORS[op] for op in order]
        assert np.array_equal(_run(img, order, factors), JC.apply(img, order, factors)), (hw, order)


def test_all_24_orders():
    img = _img(37, 53, seed=1)
    for order in itertools.permutations(ALL4):
        factors = [ALL4_FACTORS[op] for op in order]
        assert np.array_equal(_run(img, order, factors), JC.apply(img, order, factors)), order


def test_single_ops_match_pillow(fixture):
    for name in ('random', 'directed', 'gradient', 'mean_half', 'mean_below'):
        img = fixture['img/' + name]
        for op in ('brightness', 'contrast', 'saturation'):
            for f in FACTORS:                                            # (0 and 1 are the two copies of Image.blend)
                assert np.array_equal(_run(img, (op,), (f,)), fixture['out/%s/%s/%s' % (name, op, f)]), (name, op, f)
        for h in HUES:
            assert np.array_equal(_run(img, ('hue',), (h,)), fixture['out/%s/hue/%s' % (name, h)]), (name, h)


def test_composites_match_pillow(fixture):
    cases = json.loads(str(fixture['cases']))
    for name in ('random', 'directed', 'gradient', 'mean_half', 'mean_below'):
        for i, c in enumerate(cases):
            assert np.array_equal(_run(fixture['img/' + name], c['order'], c['factors']), fixture['out/%s/case%d' % (name, i)]), (name, c)


def test_mean_at_and_just_below_a_half(fixture):
    """contrast at factor 0 writes the mean itself: 10.5 -> 11, 10.496 -> 10; and a large image whose mean is exactly x.5"""
    assert (_run(fixture['img/mean_half'], ('contrast',), (0.,)) == 11).all()
    assert (_run(fixture['img/mean_below'], ('contrast',), (0.,)) == 10).all()
    big = np.full((1200, 1920, 3), 100, np.uint8)
    big[:600] = 101                                                      # mean 100.5 over 2.3 M pixels, 1024 partial sums
    assert (_run(big, ('contrast',), (0.,)) == 101).all()
    big[0, 0] = 100                                                      # one pixel less: just below
    assert (_run(big, ('contrast',), (0.,)) == 100).all()
    assert np.array_equal(_run(big, ('contrast',), (1.5,)), JC.contrast(big, 1.5))


def test_factors_that_round_to_the_copies():
    """the copies are decided on the float32 factor, as Blend.c does"""
    img = _img(9, 7, seed=2)
    for f in (1. - 1e-12, 1. + 1e-12, 1e-12, 1. - 1e-7, 1. + 2e-7):
        for op in ('brightness', 'contrast', 'saturation'):
            assert np.array_equal(_run(img, (op,), (f,)), getattr(JC, op)(img, f)), (op, f)


def test_image_that_is_not_dword_aligned():
    """a contiguous view at an odd byte offset takes the pixel-by-pixel path: same bytes, nothing outside the view touched"""
    from efgh_amd.data import color_jitter
    img = _img(37, 53, seed=3)
    order = ('saturation', 'contrast', 'hue', 'brightness')
    factors = [ALL4_FACTORS[op] for op in order]
    want = JC.apply(img, order, factors)
    for off in (1, 2, 3):
        buf = torch.full((img.size + 8,), 7, dtype=torch.uint8, device='cuda')
        view = buf[off:off + img.size].view(37, 53, 3)
        view.copy_(torch.from_numpy(img))
        assert view.data_ptr() % 4 == off
        out = color_jitter(view, _params(order, factors))
        assert np.array_equal(out.cpu().numpy(), want)
        assert np.array_equal(view.cpu().numpy(), img) and (buf[:off] == 7).all() and (buf[off + img.size:] == 7).all()


def test_no_ops_launches_nothing_and_returns_the_input():
    from efgh_amd.data import ColorJitter, color_jitter
    dev = torch.from_numpy(_img(5, 6)).cuda()
    assert color_jitter(dev, ColorJitter().sample()) is dev
    assert color_jitter(dev, _params((), ())) is dev


def _gts(rt=0.03):
    from efgh_amd.data import preproc_gt
    return preproc_gt(0, 0, 0, 0, 0, 0, rt)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_preproc_img_without_jitter_is_unchanged():
    from efgh_amd.data import ColorJitter, preproc_img
    img = _img(48, 64, seed=4)
    for rellis in (False, True):
        base = preproc_img(img, _gts(), (40, 60), rellis)                # the call as it was written before there was a jitter
        _same(base, preproc_img(img, _gts(), (40, 60), rellis, jitter=None))
        _same(base, preproc_img(img, _gts(), (40, 60), rellis, jitter=ColorJitter().sample()))


def test_preproc_img_jitters_the_source_once():
    """'in', 'raw', 'rot' and the mask are those of the jittered image; CHW and non-contiguous inputs are taken as before"""
    from efgh_amd.data import preproc_img
    img = _img(48, 64, seed=5)
    img[10:14, 20:30] = 0                                                # a black patch: stays black here, invalid in the mask as before
    order, factors = ('contrast', 'hue', 'brightness', 'saturation'), (1.3, 0.2, 0.7, 1.5)
    p = _params(order, factors)
    for rellis in (False, True):
        want = preproc_img(JC.apply(img, order, factors), _gts(), (40, 60), rellis)
        wide = torch.from_numpy(np.concatenate([img, img], axis=1)).cuda()
        chw = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).cuda()
        for src in (img, torch.from_numpy(img).cuda(), wide[:, :64], chw, np.ascontiguousarray(img.transpose(2, 0, 1))):
            before = src.clone() if torch.is_tensor(src) else src.copy()
            _same(want, preproc_img(src, _gts(), (40, 60), rellis, jitter=p))
            assert torch.equal(src, before) if torch.is_tensor(src) else np.array_equal(src, before)
    # a pixel the jitter turns into (0, 0, 0) is invalid in img_mask: the reference's own rule for black pixels
    dark = np.full((8, 8, 3), 3, np.uint8)
    got = preproc_img(dark, _gts(0.), (8, 8), jitter=_params(('brightness',), (0.3,)))
    assert (got['raw'] == 0).all() and (got['img_mask'] == 0).all()


def test_process_class_applies_the_drawn_jitter():
    import random
    from efgh_amd.data import ColorJitter, ProcessKITTIODOM, preproc_gt, preproc_img, rand_init_params
    jit = {'brightness': 0.4, 'contrast': 0.4, 'saturation': 0.4, 'hue': 0.1}
    args = {'raw_cam_img_size': (40, 60), 'lidar_line': None, 'num_points': 64, 'test': False,
            'dclb': {'l_rot_range': 0.1, 'l_trs_range': 0.2, 'c_rot_range': 0.05}, 'color_jitter': jit}
    img, pcd = _img(48, 64, seed=6), np.random.RandomState(7).randn(256, 4).astype(np.float32) * 10
    calibs = {'P2': np.eye(4), 'Tr': np.eye(4)}
    random.seed(31)
    _, img_in, _, _, gts, _ = ProcessKITTIODOM(args)(pcd, img, calibs, np.eye(4), 'f')
    random.seed(31)
    ri = rand_init_params(None, 0.1, 0.2, 0.05)                          # the seven draws of the mis-calibration come first
    p = ColorJitter(**jit).sample()
    assert len(p.order) == 4
    want = preproc_img(JC.apply(img, p.order, p.factors), preproc_gt(*ri), (40, 60))
    assert torch.equal(img_in, want['in']) and torch.equal(gts['img_rot'], want['rot']) and torch.equal(gts['img_raw'], want['raw'])
    args_t = dict(args, test=True)
    random.seed(31)
    state = random.getstate()
    _, img_t, _, _, _, _ = ProcessKITTIODOM(args_t)(pcd, img, calibs, np.eye(4), 'f', rand_init=(0,) * 7)
    assert random.getstate() == state
    assert torch.equal(img_t, preproc_img(img, preproc_gt(*(0,) * 7), (40, 60))['in'])


def test_two_runs_give_the_same_bytes():
    img = _img(300, 421, seed=8)
    order = ('hue', 'contrast', 'saturation', 'brightness')
    factors = [ALL4_FACTORS[op] for op in order]
    a, b = _run(img, order, factors), _run(img, order, factors)
    assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ every triplet through hue
@pytest.fixture(scope='module')
def hue_exhaustive():
    """all 2^24 triplets as a 4096 x 4096 image with what the contract gives at shifts 0 and 231 (computed once: the host numpy is the
    cost of this case, printed below; the device side is one launch each)"""
    t0 = time.time()
    trip = JC.all_triplets()
    hsv = JC.rgb_to_hsv(trip)
    want = {}
    for k in (0, 231):
        s = hsv.copy()
        s[..., 0] = ((s[..., 0].astype(np.int32) + k) % 256).astype(np.uint8)
        want[k] = JC.hsv_to_rgb(s)
    print('hue over all 2^24 triplets: contract on the host %.1f s' % (time.time() - t0))
    return trip, want


@pytest.mark.parametrize('hue,k', [(0.002, 0), (-25 / 255. - 1e-9, 231 - 256)])
def test_hue_on_all_triplets(hue_exhaustive, hue, k):
    """the one case that puts the device's float and double division, fmod, floor and round through every input"""
    trip, want = hue_exhaustive
    p = _params(('hue',), (hue,))
    assert p.hue_shift == k and k % 256 in want
    got = _run(trip, ('hue',), (hue,))
    bad = (got != want[k % 256]).any(axis=-1)
    assert not bad.any(), '%d of 2^24 triplets differ, first %s' % (int(bad.sum()), trip[bad][:4].tolist())
