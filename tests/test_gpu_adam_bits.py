"""efgh_adam_step, efgh_adam_step_guarded and efgh_adam_step_groups against recorded bits.  The other optimizer tests compare the
library with itself (grouped against ungrouped, guarded against plain); this one anchors all three to tests/golden/adam_bits.json,
written by tests/golden/gen_adam_bits.py before the three kernels were put on one written-out update: every case is replayed and
must leave the recorded sha256 of w, m and v after each of three steps (and, at n <= 7, the recorded bit patterns)."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import gen_adam_bits as gen  # noqa: E402

pytestmark = pytest.mark.gpu
RECORDED = json.load(open(gen.FIXTURE))


def test_the_fixture_holds_every_case():
    assert sorted(RECORDED) == sorted(gen.CASES)


@pytest.mark.parametrize('case', list(gen.CASES))
def test_recorded_bits(case):
    got, want = gen.run_case(case), RECORDED[case]
    for step, (g, w) in enumerate(zip(got.get('bits', []), want.get('bits', [])), 1):      # first: a failure here is readable
        assert g == w, (case, 'step %d' % step)
    assert got == want, case
    if case.startswith('guarded-n1025-skip'):              # step 2 held a NaN: nothing moved, and it did not count
        assert got['steps'][1] == got['steps'][0] != got['steps'][2]
        assert got['applied'] == [1, 1, 2]
