"""Photometric jitter, host side: the numpy contract (tests/jitter_contract.py) against the Pillow fixture and against Pillow itself,
the draw sequence of ColorJitter.sample(), argument validation, the Process classes' use of it, and the C ABI's new symbols."""
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jitter_contract as JC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = (0, 0.3, 1, 1.4, 2)
HUES = (0, 0.1, -0.1, 0.5, -0.5)


@pytest.fixture(scope='module')
def fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, 'jitter.npz'))
    return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------ contract against the fixture
def test_contract_single_ops_match_the_fixture(fixture):
    names = [k[4:] for k in fixture if k.startswith('img/')]
    assert sorted(names) == ['directed', 'gradient', 'mean_below', 'mean_half', 'random']
    checked = 0
    for name in names:
        img = fixture['img/' + name]
        for op in ('brightness', 'contrast', 'saturation'):
            for f in FACTORS:
                assert np.array_equal(getattr(JC, op)(img, f), fixture['out/%s/%s/%s' % (name, op, f)]), (name, op, f)
                checked += 1
        for h in HUES:
            assert np.array_equal(JC.hue(img, h), fixture['out/%s/hue/%s' % (name, h)]), (name, h)
            checked += 1
    assert checked == 5 * 20


def test_contract_composites_match_the_fixture(fixture):
    cases = json.loads(str(fixture['cases']))
    assert len(cases) >= 12
    assert {c['order'].index('contrast') for c in cases if len(c['order']) == 4} == {0, 1, 2, 3}
    for name in ('random', 'directed', 'gradient', 'mean_half', 'mean_below'):
        for i, c in enumerate(cases):
            got = JC.apply(fixture['img/' + name], c['order'], c['factors'])
            assert np.array_equal(got, fixture['out/%s/case%d' % (name, i)]), (name, c)


def test_mean_rounds_half_up_and_truncates(fixture):
    assert JC.luma_mean(fixture['img/mean_half']) == 11                  # L = 10, 11: mean 10.5
    assert JC.luma_mean(fixture['img/mean_below']) == 10                 # 127 of 256 pixels at 11: mean 10.496
    # (contrast at factor 0 shows the mean itself)
    assert (fixture['out/mean_half/contrast/0'] == 11).all() and (fixture['out/mean_below/contrast/0'] == 10).all()


# ------------------------------------------------------------------------------------------------ contract against Pillow itself
@pytest.fixture(scope='module')
def triplets():
    return JC.all_triplets()


def test_luma_matches_pillow_on_all_triplets(triplets):
    Image = pytest.importorskip('PIL.Image')
    assert np.array_equal(np.asarray(Image.fromarray(triplets, 'RGB').convert('L')), JC.luma(triplets))


def test_rgb_to_hsv_matches_pillow_on_all_triplets(triplets):
    Image = pytest.importorskip('PIL.Image')
    assert np.array_equal(np.asarray(Image.fromarray(triplets, 'RGB').convert('HSV')), JC.rgb_to_hsv(triplets))


def test_hsv_to_rgb_matches_pillow_on_all_triplets(triplets):
    Image = pytest.importorskip('PIL.Image')
    assert np.array_equal(np.asarray(Image.fromarray(triplets, 'HSV').convert('RGB')), JC.hsv_to_rgb(triplets))


def test_blend_matches_pillow_on_all_value_pairs():
    Image = pytest.importorskip('PIL.Image')
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    A, B = Image.fromarray(a, 'L'), Image.fromarray(b, 'L')
    for f in FACTORS + (0.77, 1.9, 1. - 1e-12, 1. + 1e-12, 1e-12):       # (the last three round to 1, 1 and a tiny float32)
        assert np.array_equal(np.asarray(Image.blend(A, B, f)), JC.blend(a, b, f)), f


def test_fixture_is_what_this_pillow_gives(fixture):
    """the committed fixture against the Pillow that is installed (the generator run again, byte for byte)"""
    pytest.importorskip('PIL')
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import make_golden_jitter as G
    assert G.FACTORS == FACTORS and G.HUES == HUES
    from PIL import Image
    for name, arr in G.images().items():
        assert np.array_equal(arr, fixture['img/' + name])
        im = Image.fromarray(arr, 'RGB')
        for i, (order, factors) in enumerate(G.CASES):
            cur = im
            for op, f in zip(order, factors):
                cur = G.one(cur, op, f)
            assert np.array_equal(np.asarray(cur), fixture['out/%s/case%d' % (name, i)]), (name, i)


# ------------------------------------------------------------------------------------------------ ColorJitter
def test_sample_follows_the_written_out_draws():
    from efgh_amd.data import ColorJitter, JitterParams
    cj = ColorJitter(brightness=0.4, contrast=(0.5, 1.5), saturation=0.3, hue=0.1)
    assert cj.ranges == {'brightness': (0.6, 1.4), 'contrast': (0.5, 1.5), 'saturation': (0.7, 1.3), 'hue': (-0.1, 0.1)}
    for seed in range(20):
        random.seed(seed)
        got = cj.sample()
        random.seed(seed)
        order = ['brightness', 'contrast', 'saturation', 'hue']
        for i in (3, 2, 1):                                              # the order first: three draws
            j = int(random.random() * (i + 1))
            order[i], order[j] = order[j], order[i]
        drawn = {}
        for op in ('brightness', 'contrast', 'saturation', 'hue'):       # then one factor per op, in this order
            lo, hi = cj.ranges[op]
            drawn[op] = lo + (hi - lo) * random.random()
        assert isinstance(got, JitterParams)
        assert got.order == tuple(order) and got.factors == tuple(drawn[op] for op in order)
        assert got.hue_shift == int(drawn['hue'] * 255)
        after = random.random()
        random.seed(seed)
        for _ in range(7):
            random.random()
        assert random.random() == after                                  # seven draws, no more
    assert len({ColorJitter(0.4, 0.4, 0.4, 0.1).sample().order for _ in range(400)}) == 24


def test_absent_components_are_left_out_and_draw_nothing():
    from efgh_amd.data import ColorJitter
    random.seed(3)
    state = random.getstate()
    for cj in (ColorJitter(), ColorJitter(0, None, 0.0, None), ColorJitter(brightness=None, hue=0)):
        p = cj.sample()
        assert p.order == () and p.factors == () and p.hue_shift == 0
    assert random.getstate() == state
    cj = ColorJitter(contrast=0.5, hue=(-0.5, 0.5))
    random.seed(5)
    p = cj.sample()
    random.seed(5)
    swap = int(random.random() * 2) == 0                                 # one order draw for two ops
    c, h = 0.5 + 1.0 * random.random(), -0.5 + 1.0 * random.random()
    assert p.order == (('hue', 'contrast') if swap else ('contrast', 'hue'))
    assert dict(zip(p.order, p.factors)) == {'contrast': c, 'hue': h}
    assert ColorJitter(brightness=2.5).ranges == {'brightness': (0., 3.5)}          # max(0, 1 - x)


def test_hue_shift_truncates_toward_zero():
    from efgh_amd.data import JitterParams
    for h, k in ((0.1, 25), (-0.1, -25), (0.5, 127), (-0.5, -127), (0.0039, 0), (-0.0039, 0), (0, 0)):
        assert JitterParams(('hue',), (h,)).hue_shift == k == JC.hue_shift(h)
    assert JitterParams(('brightness',), (1.2,)).hue_shift == 0


def test_bad_values_raise_naming_the_component():
    from efgh_amd import _C
    from efgh_amd.data import ColorJitter, JitterParams, color_jitter
    bad = [dict(brightness=-0.1), dict(contrast=(1.2, 0.8)), dict(saturation=float('nan')), dict(hue=0.6), dict(hue=-0.1),
           dict(hue=(-0.6, 0.1)), dict(brightness=(0.5,)), dict(contrast='x'), dict(saturation=(-1, 1)), dict(brightness=float('inf'))]
    for kw in bad:
        with pytest.raises(_C.EfghError, match=list(kw)[0]):
            ColorJitter(**kw)
    for order, factors in ((('hue',), (0.7,)), (('brightness',), (-1.,)), (('contrast', 'contrast'), (1., 1.)),
                           (('gamma',), (1.,)), (('hue', 'contrast'), (0.1,))):
        with pytest.raises(_C.EfghError):
            JitterParams(order, factors)
    with pytest.raises(_C.EfghError):
        color_jitter(np.zeros((2, 2, 3), np.uint8), {'brightness': 1.2})


# ------------------------------------------------------------------------------------------------ the Process classes
def _process_args(test, **extra):
    a = {'raw_cam_img_size': (8, 8), 'lidar_line': None, 'num_points': 4, 'test': test, 'DEVICE': 'cpu',
         'dclb': {'l_rot_range': 0.1, 'l_trs_range': 0.2, 'c_rot_range': 0.05}}
    a.update(extra)
    return a


@pytest.fixture
def stubbed(monkeypatch):
    """the Process body without its device work: what preproc_img was handed is recorded"""
    from efgh_amd.data import prepare
    seen = []
    monkeypatch.setattr(prepare, 'preproc_img', lambda img, gts, size, rellis, device, jitter=None:
                        seen.append(jitter) or {'in': 0, 'raw': 1, 'rot': 2, 'img_mask': 3})
    monkeypatch.setattr(prepare, 'preproc_pcd', lambda *a, **k: None)
    return seen


def test_process_under_test_ignores_the_jitter_and_draws_nothing(stubbed):
    from efgh_amd.data import ProcessKITTIODOM, ProcessKITTIRAW, ProcessNUSC, ProcessRELLIS
    jit = {'brightness': 0.4, 'contrast': 0.4, 'saturation': 0.4, 'hue': 0.1}
    calibs = {'P2': np.eye(4), 'Tr': np.eye(4), 'P': np.eye(4), 'T_cam_velo': np.eye(4)[:3], 'posej_T_posei': np.eye(4)}
    for cls in (ProcessKITTIODOM, ProcessRELLIS, ProcessKITTIRAW, ProcessNUSC):
        proc = cls(_process_args(True, color_jitter=jit))
        assert proc.color_jitter is None
    random.seed(11)
    state = random.getstate()
    ProcessKITTIODOM(_process_args(True, color_jitter=jit))(None, None, calibs, np.eye(4), 'f', rand_init=(0,) * 7)
    ProcessNUSC(_process_args(True, color_jitter=jit))(None, None, calibs, 'tok', rand_init=(0,) * 7)
    assert random.getstate() == state and stubbed == [None, None]


def test_process_in_training_draws_after_the_seven_of_rand_init(stubbed):
    from efgh_amd.data import ColorJitter, ProcessKITTIODOM, ProcessRELLIS
    jit = {'brightness': 0.4, 'contrast': (0.8, 1.2), 'saturation': 0.4, 'hue': 0.1}
    calibs = {'P2': np.eye(4), 'Tr': np.eye(4), 'P': np.eye(4)}
    for cls in (ProcessKITTIODOM, ProcessRELLIS):
        del stubbed[:]
        random.seed(21)
        cls(_process_args(False, color_jitter=jit))(None, None, calibs, np.eye(4), 'f')
        random.seed(21)
        for _ in range(7):
            random.random()
        want = ColorJitter(**jit).sample()
        assert len(stubbed) == 1 and stubbed[0].order == want.order and stubbed[0].factors == want.factors
    del stubbed[:]
    random.seed(21)
    ProcessKITTIODOM(_process_args(False))(None, None, calibs, np.eye(4), 'f')          # no 'color_jitter': seven draws, no jitter
    after = random.random()
    random.seed(21)
    for _ in range(7):
        random.random()
    assert stubbed == [None] and random.random() == after
    from efgh_amd import _C
    with pytest.raises(_C.EfghError, match='hue'):
        ProcessKITTIODOM(_process_args(False, color_jitter={'hue': 0.9}))
    for bad in ({'gamma': 0.2}, 0.4):
        with pytest.raises(_C.EfghError, match='color_jitter'):
            ProcessKITTIODOM(_process_args(False, color_jitter=bad))


# ------------------------------------------------------------------------------------------------ header, binding, entry points
def test_header_and_binding_see_the_new_symbols():
    from efgh_amd import _C
    sigs = _C.signatures(open(_C.HEADER).read())
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert sigs['efgh_prep_jitter_partials'] == (i32, [i64])
    assert sigs['efgh_prep_jitter_sum'] == (ctypes.c_int, [vp, i64, vp, vp, i32, i32, vp, vp])
    assert sigs['efgh_prep_jitter_apply'] == (ctypes.c_int, [vp, i64, vp, vp, i32, i32, vp, vp, vp])
    lib = _C.lib()
    assert lib.efgh_version() == _C.ABI_VERSION == 4                    # additive: the ABI version stays
    for name in ('efgh_prep_jitter_partials', 'efgh_prep_jitter_sum', 'efgh_prep_jitter_apply'):
        assert getattr(lib, name).argtypes == sigs[name][1]
    # one partial per 1024 pixels (256 threads x 4 pixels), capped at 1024
    assert [lib.efgh_prep_jitter_partials(n) for n in (0, 1, 1024, 1025, 1 << 20, (1 << 20) + 1, 1 << 24)] == [0, 1, 1, 2, 1024, 1024, 1024]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """(addresses that are never dereferenced: every call below fails its argument checks on the host)"""
    from efgh_amd import _C
    lib = _C.lib()
    ops = lambda *v: (ctypes.c_int32 * len(v))(*v)
    fac = lambda *v: (ctypes.c_float * len(v))(*v)
    IN, OUT, PART = 1 << 20, 1 << 21, 1 << 22
    bad_apply = [
        (IN, 16, ops(0), fac(1.2), 0, 0, None, OUT),                   # no ops
        (IN, 16, ops(0, 1, 2, 3, 0), fac(1, 1, 1, 0, 1), 5, 0, PART, OUT),      # five
        (IN, 16, ops(0, 0), fac(1.2, 1.1), 2, 0, None, OUT),           # an op twice
        (IN, 16, ops(7), fac(1.2), 1, 0, None, OUT),                   # an unknown op
        (IN, 16, ops(0), fac(float('nan')), 1, 0, None, OUT),          # a factor that is not finite
        (IN, 16, ops(3), fac(0.), 1, 256, None, OUT),                  # a hue shift outside -255 .. 255
        (IN, 16, ops(1), fac(1.2), 1, 0, None, OUT),                   # contrast without its partial sums
        (IN, 16, ops(0), fac(1.2), 1, 0, PART, OUT),                   # partial sums without contrast
        (IN, 16, ops(0), fac(1.2), 1, 0, None, IN),                    # in place
        (IN, 16, ops(0), fac(1.2), 1, 0, None, IN + 45),               # overlapping
        (IN, 0, ops(0), fac(1.2), 1, 0, None, OUT), (None, 16, ops(0), fac(1.2), 1, 0, None, OUT),
        (IN, 16, None, fac(1.2), 1, 0, None, OUT), (IN, 16, ops(0), None, 1, 0, None, OUT),
    ]
    for a in bad_apply:
        assert lib.efgh_prep_jitter_apply(*a, None) == -1, a
        assert lib.efgh_last_error()
    bad_sum = [(IN, 16, ops(0), fac(1.2), 1, 0, PART),                 # no contrast: nothing to sum for
               (IN, 16, ops(1), fac(1.2), 1, 0, None), (IN, 16, ops(1), fac(1.2), 1, 0, PART + 4),
               (IN, 16, ops(1, 1), fac(1.2, 1.), 2, 0, PART)]
    for a in bad_sum:
        assert lib.efgh_prep_jitter_sum(*a, None) == -1, a
    with pytest.raises(ctypes.ArgumentError):
        lib.efgh_prep_jitter_apply(IN, 16.0, ops(0), fac(1.2), 1, 0, None, OUT, None)
