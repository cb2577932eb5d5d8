"""How lattice.build_pyramid_batched plans, enqueues and escalates the levels of a pyramid: what tests/lattice_capture.py records
from it on CPU tensors - every efgh_lattice_* launch with its arguments, every level's plan, capacities and counts, STATS and
the signature's _SIZES / _HASH_LEVELS / _BIG_LEVELS / _CLEAN after each build, the log messages - against
tests/golden/lattice_plans.json, build by build.

The fixture was written by `python tests/lattice_capture.py --write` at commit 207a803 ("Describe each GEMM layer once for the
inference and training paths"), the last one with the function as one body that carried the escalation rule twice and a plan
as a bare tuple of varying length, and is not regenerated from later code: a change of a digest is a change of what is launched
or of how a signature escalates, and belongs in a pull request that says so.

The scenarios (lattice_capture.scenarios; the stand-in supplies the counts and the ERR words): clean level-by-level and speculative
builds, one sample, three scales, need_off=False, radii (1, 2, 3) on partitioned, big-bucket and hash levels, PROFILE; in a
speculative build a count beyond capacity (ERR bit 0), a bucket overflow (bit 2) once, again in a later build, two and three times
in one call, on three levels in turn, on two levels at once, with bit 3, together with bit 0 on another level, on a hash level,
and the alias cap (bit 1); the same overflows inside the level-by-level path; ESCALATION_DECAY = 2 over seven builds (the
sequence test_escalations_expire_after_clean_builds asserts on the GPU), decay 0, an overflow between clean builds; a level the
partitioned build has no buckets for; changed B and N.

One case is left out of the fixture on purpose, and pinned by a test of its own below: a level that is ALREADY on the big-bucket
plan and overflows in the level-by-level path.  207a803 built it once more with the same big-bucket plan - the same launches on
the same input, which overflow again - before it took the hash build; the one escalation rule sends it to the hash build at once."""
import json

import pytest

import lattice_capture as LC


@pytest.fixture(scope='module')
def tables():
    from efgh_amd import _C
    import os
    if not os.path.exists(_C.SO_PATH):
        pytest.fail('libefgh_hip.so is not built: run __graft_entry__.build() first')
    return json.load(open(LC.GOLDEN)), LC.table()


def test_fixture_covers_the_paths(tables):
    want, _ = tables
    reached = {e for c in want['calls'] for e in c.split('+')}
    assert reached == {'part_build', 'part_neighbors', 'level_build', 'level_neighbors', 'neighbors_r'}
    assert len(want['scenarios']) >= 30 and sum(len(v) for v in want['scenarios'].values()) >= 90


def test_builds_equal_the_recorded_ones(tables):
    want, got = tables
    assert sorted(got['scenarios']) == sorted(want['scenarios']), 'the scenario list changed: the fixture no longer describes it'
    bad = []
    for name, w in want['scenarios'].items():
        g = got['scenarios'][name]
        assert len(w) == len(g), name
        for i, ((wc, wh), (gc, gh)) in enumerate(zip(w, g)):
            if (want['calls'][wc], wh) != (got['calls'][gc], gh):
                bad.append((name, i, want['calls'][wc], got['calls'][gc], 'same digest' if wh == gh else 'digest differs'))
    assert not bad, (len(bad), bad[:8])


def test_big_level_that_overflows_level_by_level_takes_the_hash_build():
    key = (None, 2, 512, LC.SCALES)
    with LC.Capture() as cap:
        cap.reset()
        cap.lat._BIG_LEVELS[key] = {1}
        rec = cap.build(script={(0, 1): (4, None)})
    assert [c[0] for c in rec['calls'][2:5]] == ['part_build', 'level_build', 'level_neighbors']
    assert rec['calls'][2][-2] == 1                              # (the build that overflowed was the big-bucket one)
    assert [lv[0] for lv in rec['levels']][1] == ['hash', 0, 0, False]
    assert rec['state'][2:4] == [[1], [1]] and rec['logs'] == []
