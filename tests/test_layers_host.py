"""What the layer executors hand to the library: the table tests/layer_capture.py records from the public functions of
efgh_amd/nets/layers.py - the entry points of every forward and backward() in order, every argument handed to the library, shape,
strides and storage relation of what a layer returns, its _efgh_lazy / _efgh_bnsrc tags, which gradients come back as None, the
num_batches_tracked ticks - against tests/golden/layers.json, entry by entry.

The fixture was written by layer_capture.py at commit af8006b ("Route every gather-GEMM launch through one kernel-selection chain"),
the last one whose no-tape path (layers._run) and tape path (GemmLayerFn) each described a layer on their own, and is not regenerated
from later code: a change of the table is a change of what a layer launches and belongs in a pull request that says so.  (Torch-side
copies are not part of it: temporaries a layer allocates itself are 'tmp' whatever made them.)

The case list (layer_capture.cases), each case in the four (train, grad) contexts, under the default switches and with LAZY_ACT,
W2_BWD_FUSED, W2_BWD_FUSED_POOL, BN_MASK_BITS, USE_WINO2D and USE_THIN off in turn:
- conv2d 3x3 / 1x1 at stride 1 / 2 with 4 (3 real), 16, 32, 64, 128 and 256 channels on 6x7, 8x8 and 12x16 maps (both sides of the
  8 x 8 limit of the 2-D Winograd path), a 32-channel 200x320 map (the small-channel kernel's pixel threshold), 3 -> 64; with and
  without bias, BatchNorm and residual, out=(buf, coff), in_ch=, skip_out, pool, defer_act into a consumer that can and one that
  cannot apply it, 1 / 2 / 3 / 10 output channels;
- conv_transpose2d with padding 1 and output padding 1 / 0 at odd sizes, 64 / 32 / 3 / 2 / 1 output channels (<= 3: the col2im
  form), skip_out, defer_for, out=, with bias, without BatchNorm; run_convt_heads;
- linear_rows with BatchNorm1d, count, lda / a_off, out=;
- blur_conv on a bare table, on a radius-1 level with BLUR_DGRAD_FUSED on and off, on a radius-2 level, above the k-split row limit,
  and the weight-shape rejection (the one case that may raise);
- run_vgg, run_basic_block / run_resnet_layer with and without downsample and alias_in, run_convt_bn_relu, run_conv_bn_relu."""
import json
import os

import pytest

import layer_capture as LC

HERE = os.path.dirname(os.path.abspath(__file__))
# the entry points GemmLayerFn and layers._run reach at af8006b under these switches (taken from that capture)
REQUIRED = [
    'efgh_gather_gemm', 'efgh_thin_gemm', 'efgh_c4_conv3x3', 'efgh_c4_conv3x3_pooled', 'efgh_sc_conv3x3', 'efgh_wino_conv3x3',
    'efgh_wino_conv3x3_hpool', 'efgh_wino2d_input', 'efgh_wino2d_input_act', 'efgh_wino2d_output', 'efgh_wino2d_output_pooled',
    'efgh_plane_gemm', 'efgh_fold_planes', 'efgh_blur_r_gemm', 'efgh_gather_wgrad', 'efgh_thin_wgrad', 'efgh_c4n4_wgrad', 'efgh_c4_wgrad',
    'efgh_sc_wgrad', 'efgh_wino_wgrad', 'efgh_plane_wgrad_batched', 'efgh_wino2d_wfinish', 'efgh_wino2d_dy', 'efgh_blur_r_wgrad',
    'efgh_pack_weight_padded', 'efgh_unpack_weight', 'efgh_wino_pack', 'efgh_wino2d_pack',
    'efgh_scale_shift_act', 'efgh_scale_shift_act_bits', 'efgh_bn_finalize', 'efgh_col_stats', 'efgh_act_bn_bwd_reduce',
    'efgh_act_bn_bwd_apply', 'efgh_bwd_finalize_f32', 'efgh_wino2d_bwd_transforms', 'efgh_wino2d_bwd_transforms_pooled',
    'efgh_maxpool2', 'efgh_maxpool_v2', 'efgh_maxpool2_affine', 'efgh_maxpool2_bwd_affine', 'efgh_pool_bn_bwd_reduce',
    'efgh_pool_bn_bwd_reduce_pooled', 'efgh_pool_bn_bwd_apply', 'efgh_convt_col2im', 'efgh_convt_im2col', 'efgh_blur_dgrad_alias',
    'efgh_table_gather_transposed', 'efgh_table_scatter_add',
]


@pytest.fixture(scope='module')
def tables():
    from efgh_amd import _C
    if not os.path.exists(_C.SO_PATH):
        pytest.fail('libefgh_hip.so is not built: run __graft_entry__.build() first')
    got = LC.table()
    packed = json.load(open(os.path.join(HERE, 'golden', 'layers.json')))      # (the compact form: layer_capture.pack)
    assert packed['names'] == [len(got['names']), LC.RC._h(got['names'])], 'the case list changed: the fixture no longer describes it'
    return packed, LC.unpack(packed), got


def test_fixture_reaches_every_entry_point_and_only_the_rejections_raise(tables):
    packed, want, got = tables
    assert not [e for e in REQUIRED if e not in packed['entries']]
    assert sorted(want) == sorted(s[0] for s in LC.SETTINGS)
    for rows in want.values():
        raised = [n for n, r in zip(got['names'], rows) if not r[0].startswith('efgh_')]
        assert raised and all(n.split(' | ')[0] in LC.RAISES for n in raised), raised[:8]


def test_layers_equal_the_recorded_table(tables):
    _, want, got = tables
    bad = []
    for name, _ in LC.SETTINGS:
        w, g = want[name], got['settings'][name]
        assert len(w) == len(g) == len(got['names'])
        bad += [(name, case, wr, gr) if wr[:2] != gr[:2] else (name, case, 'same entry points, digest differs')
                for case, wr, gr in zip(got['names'], w, g) if wr != gr]
    assert not bad, (len(bad), bad[:6])
