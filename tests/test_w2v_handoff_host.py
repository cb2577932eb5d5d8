"""The input transform of a 2-D Winograd layer goes from its forward to its weight gradient on the layer's autograd node
(GemmLayerFn: ctx.kept_v): what layers.conv2d launches in a (train, grad) context, recorded without a GPU by
layer_capture.LayerCapture.  (tests/golden/layers.json pins the same hand-off for its 128- and 256-channel cases; these are the
cases its closed list does not hold.)"""
import os

import pytest
import torch.nn as nn

import layer_capture as LC

INPUT = 'efgh_wino2d_input'


@pytest.fixture(scope='module')
def cap():
    from efgh_amd import _C
    if not os.path.exists(_C.SO_PATH):
        pytest.fail('libefgh_hip.so is not built: run __graft_entry__.build() first')
    with LC.LayerCapture() as c:
        yield c


def _count(calls):
    return calls.split('+').count(INPUT)


def test_one_layer_backward_does_not_transform_again(cap):
    case = LC.conv_case(128, 128, 3, 1, 9, 13)
    fwd, bwd, _ = cap.case(case, True, True)
    assert _count(fwd) == 1 and 'efgh_wino2d_wfinish' in bwd
    assert _count(bwd) == 0
    cap.ops.W2V_KEEP = False
    try:
        fwd_off, bwd_off, _ = cap.case(case, True, True)
    finally:
        cap.ops.W2V_KEEP = True
    assert fwd_off == fwd
    assert _count(bwd_off) == 1
    assert [e for e in bwd_off.split('+') if e != INPUT] == bwd.split('+')


def _two_layers_one_input(grad):
    L = LC._layers()
    convs = [nn.Conv2d(128, 128, 3, 1, 1, bias=False) for _ in range(2)]
    bns = [nn.BatchNorm2d(128) for _ in range(2)]
    x = LC.T(2, 9, 13, 128, grad=grad)

    def run(ctx):
        return tuple(L.conv2d(ctx, x, m, b, 1, 0.0) for m, b in zip(convs, bns))
    return LC.P({'x': x}, 'm', *convs, *bns), bns, run


def test_two_layers_on_one_input_each_keep_their_own(cap):
    """(with the transform keyed by the input's address the second forward replaced the first one's entry, and the second backward
    transformed again)"""
    fwd, bwd, _ = cap.case(_two_layers_one_input, True, True)
    assert _count(fwd) == 2 and bwd.split('+').count('efgh_wino2d_wfinish') == 2
    assert _count(bwd) == 0
