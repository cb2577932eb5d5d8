"""Which kernel serves a launch: the table tests/route_capture.py records from ops.gather_gemm / ops.gather_wgrad - entry points
called, profile records, every argument handed to the library, the answers of stats_rows / pool_fusable / lazy_capable /
wgrad_lazy_capable, the return value - against tests/golden/routes.json, entry by entry.

The fixture was written by route_capture.py at commit fa9984f ("Make a plain benchmark run lean"), the last one with the dispatch as
an if / elif chain inside the two functions, and is not regenerated from later code: a change of the table is a change of
which kernel serves a shape, or of what it is handed, and belongs in a pull request that says so.  The one difference allowed for
is in calls that fail: a case that raises is recorded by its exception type alone (fa9984f launched efgh_gather_gemm before it
rejected an unserved `pool`).

The case list (route_capture.grid_cases, special_cases), run under every setting of route_capture.SETTINGS:
- 3x3 stride 1, 3x3 stride 2 and 1x1 over channels^2 x map sizes, plain / with statistics / with the pool pool_fusable offers, and
  the weight gradient; the full grid under the default switches (TLS.train_step off and on), a thinned one that keeps every family
  and both sides of every threshold (64 / 128 channels, 7 x 9 / 8 x 8 maps, 64000 pixels against SC_MIN_PIXELS_32) for the others;
- linear rows (mode 0, no geometry; N == 4 and C == 4 among them), the four transposed-convolution parity classes, the BCL blur on
  both sides of every k-split condition and with alias_mask, the batched correlation launches, M_dev and batch on shapes every family
  would serve, MODE_BLUR_R plain and with each argument it rejects, lazy / pre_v / pre_gy and pool=True / 'h' on routes that take
  them and on routes that do not, bn_bwd with BN_BWD_FUSED / BN_BWD_FUSED_2D on and off, unpack with FOLD_UNPACK on and off, the
  forward's input transform kept (keep_v=) and handed to the weight gradient (pre_v=) or not, 16- / 32-channel launches at
  a_off / out_off / res_off of 2 with and without statistics, and misaligned weight-gradient operands.
At fa9984f the table reaches every entry point of REQUIRED in tests/test_gpu_launch_contract.py (checked below on the fixture)."""
import json
import os
import re

import pytest

import route_capture as RC

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def tables():
    from efgh_amd import _C
    if not os.path.exists(_C.SO_PATH):
        pytest.fail('libefgh_hip.so is not built: run __graft_entry__.build() first')
    got = RC.table()
    packed = json.load(open(os.path.join(HERE, 'golden', 'routes.json')))      # (the compact form: route_capture.pack)
    # the fixture names its cases by one hash per grid: the case list of the code under test has to be the recorded one
    assert packed['names'] == {g: [len(n), RC._h(n)] for g, n in got['names'].items()}, 'the case list changed: the fixture no longer describes it'
    return RC.unpack(packed, got['names']), got


def test_fixture_reaches_every_required_entry_point_and_profile_list(tables):
    want, _ = tables
    src = open(os.path.join(HERE, 'test_gpu_launch_contract.py')).read()
    required = re.findall(r"'(efgh_\w+)'", re.search(r'REQUIRED = \[(.*?)\]', src, re.S).group(1))
    assert len(required) >= 25
    reached = {e for c in want['calls'] for e in c.split('+')}
    assert not [e for e in required if e not in reached]
    assert want['lists'] == sorted(RC.LISTS)
    assert sorted(want['settings']) == sorted(s[0] for s in RC.SETTINGS)


def test_routes_equal_the_recorded_table(tables):
    want, got = tables
    assert got['lists'] == want['lists']
    bad = []
    for name, _, _, grid in RC.SETTINGS:
        w, g = want['settings'][name], got['settings'][name]
        assert len(w) == len(g) == len(got['names'][grid])
        for case, wi, gi in zip(got['names'][grid], w, g):
            (wc, wh), (gc, gh) = want['records'][wi], got['records'][gi]
            if (want['calls'][wc], wh) != (got['calls'][gc], gh):
                bad.append((name, case, want['calls'][wc], got['calls'][gc], 'same digest' if wh == gh else 'digest differs'))
    assert not bad, (len(bad), bad[:12])
