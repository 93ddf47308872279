"""CPU tests of tests/block_sequence_ref.py: run_oracle plays every sequence of tests/test_hip_block_transitions.py, and the inputs are
known to discriminate before anything reaches a GPU -- a change the oracle has a parameter for moves its final positions by at least
ten times the bound the device is later held to (rel_rms <= 1e-4, the bound of tests/test_hip_parity.py for a full run), a
transport-only change moves nothing, the stop condition fires in the block it is meant to and the NaN block leaves the mesh alone."""
import numpy as np
import pytest

import block_sequence_ref as B

ANCHOR_BOUND = 1e-4
VARIANTS = [(c, early) for c in B.CASES for early in ((False, True) if c.early else (False,))]


def _common(a, b):
    n = min(a.shape[0], b.shape[0])          # (the mesh with two spare slots against the plain one: the rows both have)
    return a[:n], b[:n]


@pytest.mark.parametrize('case,early', VARIANTS, ids=['%s%s' % (c.name, '-early' if e else '') for c, e in VARIANTS])
def test_oracle_plays_the_sequence_and_the_change_is_visible(case, early):
    steps, control = case.steps(early)
    a, b = B.run_oracle(steps), B.run_oracle(control)
    assert len(a) == len(steps) and all(x['error'] is None for x in a)
    assert [x['loopcount'] for x in a] == [s['search']['num_iters'] for s in steps]
    margin = B.rel_rms(*_common(a[-1]['positions'], b[-1]['positions']))
    print('%s%s: the change moves the oracle\'s final positions by %.3e of the bbox diagonal' % (case.name, ' (early)' if early else '', margin))
    if case.anchor is None:          # transport only, or no oracle parameter: nothing moves
        assert case.kind == 'transport' or case.why
        for x, y in zip(a, b):
            assert np.array_equal(x['positions'], y['positions']) and np.array_equal(x['tests'], y['tests'])
    elif case.anchor:
        assert margin >= 10 * ANCHOR_BOUND, margin
    else:
        assert case.why and 0 < margin < 10 * ANCHOR_BOUND          # dropped from the anchor for that reason, and for no other


def test_oracle_stop_fires_inside_the_long_block_and_not_in_the_next():
    blocks = B.run_oracle(B.stop_case(), 'm2', 'p4')
    lc = [b['loopcount'] for b in blocks]
    assert lc[:B.OPENING] == [3] * B.OPENING
    assert 3 < lc[B.OPENING] < B.STOP_LONG, lc          # fires in that block
    assert lc[B.OPENING + 1] == 3                        # history reset: all three iterations


def test_oracle_nan_block_leaves_the_mesh_at_the_last_good_iterate():
    steps = B.nan_case()
    blocks = B.run_oracle(steps)
    k = B.OPENING
    assert [b['error'] for b in blocks] == [None] * k + ['nan', None, None, None]
    assert np.array_equal(blocks[k]['mesh_positions'], blocks[k - 1]['mesh_positions'])
    assert blocks[k + 1]['loopcount'] == 3 and not np.array_equal(blocks[k + 1]['positions'], blocks[k - 1]['positions'])
    # the repaired block is the block the sequence would have run without the failure
    _, control = B.build([], tail=1)
    ref = B.run_oracle(control[:k + 1])
    assert np.array_equal(blocks[k + 1]['positions'], ref[k]['positions'])


@pytest.mark.parametrize('early', [False, True], ids=['late', 'early'])
def test_oracle_leaves_out_a_block_with_a_status_armed(early):
    """status_case: the armed block is left out (the reference raises before `self.f[:] = fnew`), so the block after it is, exactly,
    the block the control runs at the armed index -- for every status alike (the oracle has no parameter for which)."""
    k = 1 if early else B.OPENING
    runs = {}
    for name in ('nan', 'handoff'):
        steps, control = B.status_case(name, early)
        assert len(steps) == len(control) == k + 1 + B.STATUS_TAIL
        assert [s['raises'] for s in steps] == [None] * k + [name] + [None] * B.STATUS_TAIL
        assert all(s['pre'] == ([('raise_status', name)] if i == k else []) and s['search'] == control[i]['search'] for i, s in enumerate(steps))
        runs[name] = B.run_oracle(steps)
    ref = B.run_oracle(control)
    for name, blocks in runs.items():
        assert [b['error'] for b in blocks] == [None] * k + [name] + [None] * B.STATUS_TAIL
        assert np.array_equal(blocks[k]['mesh_positions'], blocks[k - 1]['mesh_positions']) and blocks[k]['positions'] is None
        for i in range(k):
            assert np.array_equal(blocks[i]['positions'], ref[i]['positions'])
        for i in range(k + 1, len(blocks)):          # shifted by the block that was left out: positions, and the `tests` history with them
            assert blocks[i]['loopcount'] == 3
            assert np.array_equal(blocks[i]['positions'], ref[i - 1]['positions'])
            assert np.array_equal(blocks[i]['tests'], ref[i - 1]['tests']) and np.array_equal(blocks[i]['ress'], ref[i - 1]['ress'])
        assert not np.array_equal(blocks[k + 1]['positions'], blocks[k - 1]['positions'])


def test_eviction_sequence_has_more_shapes_than_the_ring_has_slots():
    steps, n = B.eviction_case()
    shapes = [(s['search']['num_iters'], s['search']['pos']) for s in steps[B.OPENING:]]
    assert n == 10 and len(set(shapes[:n])) == 10 > 8
    assert shapes[n:] == shapes[:3] * B.EVICTION_REVISITS and B.EVICTION_REVISITS % 2 == 1
