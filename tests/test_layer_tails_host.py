"""What GemmLayerFn hands to the library on the paths tests/test_layers_host.py does not hold, recorded by tests/layer_capture.py
in the same form (entry points of the forward and of backward() in order, a digest of every argument, of what the layer returns, of
the None gradients and the num_batches_tracked ticks) against tests/golden/layer_tails.json, entry by entry.

The fixture was written by this file (`python tests/test_layer_tails_host.py tests/golden/layer_tails.json`) on a checkout of commit
13738b9 ("Recompute the pooled 4-channel conv maps in training, do not store them"), the last one whose GemmLayerFn held the
epilogues of a layer as one nest of conditions in each direction, and is not regenerated from later code: a change of the table is a
change of what a layer launches and belongs in a pull request that says so.

The cases, each in the four (train, grad) contexts, all with ops.C4_POOL_RECOMPUTE_MIN_BYTES = 0 (the 384-MB bound keeps the
recompute path out of maps this small):
- the pooled 4-channel layers 3 -> 64 on 6x70, on 7x67 with a bias (odd last row and column, the saved padded bias), 3 -> 32 on
  4x4 (one unit), and (64, 'M', 128) through run_vgg (the recompute layer inside a trunk, its consumer's backward in front of it);
- the same four with C4_POOL_RECOMPUTE off and with POOL_REDUCE_FROM_Y off: both fall back to the stored-raw launches;
- the neighbours that must not take the recompute path: LeakyReLU (efgh_pool_bn_bwd_reduce) and 3 -> 16 (the thin route, with
  efgh_col_stats);
- 16 -> 10 pooled: the padded channel count sends the backward through efgh_maxpool2_bwd_affine and the generic reduce / apply
  although BatchNorm is in train mode.
A pooled layer without BatchNorm is not in the fixture (13738b9 ran its forward at full resolution and died three calls down in its
backward): its forward refuses it with an AssertionError, which the last test states on its own."""
import json
import os
import sys

import pytest

import layer_capture as LC

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'layer_tails.json')
SWITCHES = ('C4_POOL_RECOMPUTE', 'C4_POOL_RECOMPUTE_MIN_BYTES', 'POOL_REDUCE_FROM_Y')
SETTINGS = [('recompute', {}), ('C4_POOL_RECOMPUTE off', {'C4_POOL_RECOMPUTE': False}), ('POOL_REDUCE_FROM_Y off', {'POOL_REDUCE_FROM_Y': False})]
RECOMPUTE = ['efgh_c4_conv3x3_stats', 'efgh_c4_conv3x3_pooled_train', 'efgh_pool_bn_bwd_reduce_pooled_win', 'efgh_c4_pool_bwd_draw']
STORED_RAW = ['efgh_c4_conv3x3', 'efgh_maxpool2_affine', 'efgh_pool_bn_bwd_apply']


def cases():
    """[(name, {switch: value}, build)]"""
    c4 = [('C3->64 6x70 pool', LC.conv_case(3, 64, 3, 1, 6, 70, xgrad=False, pool=True)),
          ('C3->64 7x67 bias pool', LC.conv_case(3, 64, 3, 1, 7, 67, xgrad=False, pool=True, bias=True)),
          ('C3->32 4x4 pool', LC.conv_case(3, 32, 3, 1, 4, 4, xgrad=False, pool=True)),
          ('vgg 64 M 128 18x22', LC.vgg_case((64, 'M', 128), 18, 22, B=2))]
    out = [('%s | %s' % (n, s), sw, b) for s, sw in SETTINGS for n, b in c4]
    out += [('C3->64 6x70 pool leaky | recompute', {}, LC.conv_case(3, 64, 3, 1, 6, 70, xgrad=False, pool=True, act=2, slope=0.2)),
            ('C3->16 6x70 pool | recompute', {}, LC.conv_case(3, 16, 3, 1, 6, 70, xgrad=False, pool=True)),
            ('C16->10 8x8 pool | recompute', {}, LC.conv_case(16, 10, 3, 1, 8, 8, pool=True))]
    return out


def capture(cs):
    """{'<case> | train=t grad=g': [forward entry points | exception type, backward entry points, digest]}"""
    got = {}
    with LC.LayerCapture() as cap:
        old = {k: getattr(cap.ops, k) for k in SWITCHES}
        try:
            for name, sw, build in cs:
                for k in SWITCHES:
                    setattr(cap.ops, k, old[k])
                cap.ops.C4_POOL_RECOMPUTE_MIN_BYTES = 0
                for k, v in sw.items():
                    setattr(cap.ops, k, v)
                for t, g in LC.CONTEXTS:
                    got['%s | train=%d grad=%d' % (name, t, g)] = cap.case(build, t, g)
        finally:
            for k, v in old.items():
                setattr(cap.ops, k, v)
    return got


def _built():
    from efgh_amd import _C
    if not os.path.exists(_C.SO_PATH):
        pytest.fail('libefgh_hip.so is not built: run __graft_entry__.build() first')


@pytest.fixture(scope='module')
def tables():
    _built()
    return json.load(open(FIXTURE)), capture(cases())


def _entries(rows, key, ctx='train=1 grad=1'):
    return {e for n, r in rows.items() if key in n and n.endswith(ctx) for e in (r[0] + '+' + r[1]).split('+')}


def test_fixture_reaches_the_recompute_launches_and_nothing_raises(tables):
    want, got = tables
    assert sorted(want) == sorted(got), 'the case list changed: the fixture no longer describes it'
    assert not [e for e in RECOMPUTE if e not in _entries(want, '| recompute')]
    for rows in (want, got):
        assert not [n for n, r in rows.items() if not r[0].startswith('efgh_')]
    # with either switch off, and for the neighbours, the stored-raw launches and none of the recompute path's
    for key in ('C4_POOL_RECOMPUTE off', 'POOL_REDUCE_FROM_Y off', 'pool leaky', 'C3->16', 'C16->10'):
        met = _entries(want, key)
        assert met and not met & set(RECOMPUTE), key
    assert set(STORED_RAW) <= _entries(want, 'C3->64 6x70 pool | C4_POOL_RECOMPUTE off')
    assert 'efgh_pool_bn_bwd_reduce' in _entries(want, 'pool leaky')
    assert 'efgh_col_stats' in _entries(want, 'C3->16')
    assert {'efgh_maxpool2_bwd_affine', 'efgh_act_bn_bwd_reduce', 'efgh_act_bn_bwd_apply'} <= _entries(want, 'C16->10')


def test_tails_equal_the_recorded_table(tables):
    want, got = tables
    bad = [(n, want[n], got[n]) if want[n][:2] != got[n][:2] else (n, 'same entry points, digest differs') for n in want if want[n] != got[n]]
    assert not bad, (len(bad), bad[:6])


def test_pooled_layer_without_batchnorm_is_refused_in_the_forward():
    _built()
    got = capture([('C16 8x8 pool no bn', {}, LC.conv_case(16, 16, 3, 1, 8, 8, pool=True, bn=False))])
    # (LayerCapture.case records by its type alone an exception of the forward; one of backward() would propagate)
    for t in (0, 1):
        assert got['C16 8x8 pool no bn | train=%d grad=1' % t] == ['AssertionError', '', '']
        assert got['C16 8x8 pool no bn | train=%d grad=0' % t][0].startswith('efgh_')      # (no tape: pool is not asked for)


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(HERE))
    open(sys.argv[1], 'w').write(LC.RC.dumps(capture(cases())))
