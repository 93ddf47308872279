"""
GPU tests (run with -m gpu on an MI355X): the fit's own failure handling on a LIVE context -- the tail of nw_search_end
(csrc/nanowrap.hip, `if (st.status != 0)`) for every status a kernel of a single-rank block can raise, and what the Python mirror does
with the one that says "run the block again".

A block can end with a status that a kernel raised in the device state: NW_ERR_NAN, NW_ERR_SINGULAR, NW_ERR_INTERNAL (an invalid face
id out of the query) or NW_ERR_HANDOFF (the attraction workgroups appended to the query launch gave up waiting for their work item; they
rely on in-order dispatch, "observed, not promised": csrc/nw_nn.h).  nw_search_end then clears the sticky status, resets stop_at, for
the hand-off moves the attraction step into a launch of its own (handoff_off) and destroys every recorded graph, and returns the code.
Only NW_ERR_NAN had been driven through that tail on a context that was used afterwards (block_sequence_ref.nan_case).

The status is raised from the host: nw_debug(what = 8) arms the context, the next block's begin writes the code into the status word of
the device state in front of the block's first launch.  The block then takes the path of a status raised in its first iteration's
attraction step (the path nan_case runs): k_solve_update applies nothing and sets stop_at, nw_search_end meets the code.

What this does NOT execute, on purpose: the 200 ms poll in k_nn_wave and its give-up branch.  Reaching them means withholding a work
item's word so that a workgroup spins on a machine others share -- provoking a stall.  There is no knob for it and none is added.

The sequences (block_sequence_ref.status_case) run on that module's Scene: 642 vertices, 6000 localizations, blocks of 3 -- the smallest
at which all ten launches of an iteration are real -- and open with five identical blocks, so the query is warm and the attraction step
rides in the query launch when the status arrives; the `-early` variants arm the second block, while the layout is still changing.
_run_levels (tests/test_hip_block_transitions.py) holds profiling levels 0, 1 and 4 to each other bit for bit after EVERY block, the
failed one included, and checks that level 0 replays every block from a graph.  The control -- identical blocks, nothing armed, level 1
-- is run once for the module.  The hand-off after some iterations of a block have run exists only in tests/test_search_retry_cpu.py:
the injection always fails in iteration 0.
"""
import time

import numpy as np
import pytest

import block_sequence_ref as B
from test_hip_block_transitions import FIELDS, LEVELS, _anchor, _delta, _run_levels, _same_block

pytestmark = pytest.mark.gpu

NAMES = ('nan', 'singular', 'internal', 'handoff')
CAUSE = dict(nan='NaN', singular='singular', internal='invalid face id', handoff='separate launches')          # nw_last_error names the cause
NW_ERR_BADARG = -1
CONTROL_BLOCKS = B.OPENING + 5
_control_blocks = []


@pytest.fixture(scope='module', autouse=True)
def _module_duration():
    t0 = time.time()
    yield
    print('\ntests/test_hip_block_status.py: %.1f s' % (time.time() - t0))


def _control(n):
    """the first n blocks of a sequence of identical blocks with nothing armed (level 1), run once and left unchanged"""
    assert n <= CONTROL_BLOCKS
    if not _control_blocks:
        _, control = B.build([], after=CONTROL_BLOCKS, tail=0)
        _control_blocks.extend(B.run_device(control, 1)[0])
        assert all(b['error'] is None and b['loopcount'] == 3 and b['status_before'] == (0, 0) and b['status_info'] == (0, 0) for b in _control_blocks)
    return _control_blocks[:n]


def _equals_control(dev, ctrl, skip=()):
    return [k for k in _same_block(dev, ctrl) if k not in skip]


@pytest.mark.parametrize('name,early', [(n, e) for n in NAMES for e in (False, True)], ids=['%s%s' % (n, '-early' if e else '') for n in NAMES for e in (False, True)])
def test_a_status_raised_on_the_device_leaves_the_context_usable(name, early):
    steps, _ = B.status_case(name, early)
    k, n, code = 1 if early else B.OPENING, len(steps), B.STATUS_CODES[name]
    label = 'status_%s%s' % (name, '-early' if early else '')
    runs = _run_levels(label, steps, handoff_retries=0)
    ctrl = _control(n)
    for lv in LEVELS:
        dev = runs[lv][0]
        # the status arrives once, with its cause, and the mesh stays at the last good iterate
        assert [b['error'] for b in dev] == [None] * k + [name] + [None] * B.STATUS_TAIL, (lv, [b['error'] for b in dev])
        assert CAUSE[name] in dev[k]['message'], dev[k]['message']
        assert np.isfinite(dev[k]['mesh_positions']).all()
        assert np.array_equal(dev[k]['mesh_positions'], dev[k - 1]['positions'])
        assert len(dev[k]['tests']) == 0
        # stop_at was reset and the sticky status cleared: the blocks that follow run all their iterations
        for b in dev[k + 1:]:
            assert b['loopcount'] == 3 and len(b['tests']) == 3, (lv, b['loopcount'])
        # ... and are the blocks the sequence would have run anyway (for the hand-off: the attraction step as a launch of its own is
        # transport only)
        for i in range(k):
            assert _equals_control(dev[i], ctrl[i]) == [], 'level %d, block %d (before the status) differs from the control in %s' % (lv, i, _same_block(dev[i], ctrl[i]))
        for i in range(k + 1, n):
            assert _equals_control(dev[i], ctrl[i - 1]) == [], 'level %d, block %d differs from the control\'s block %d in %s' % (lv, i, i - 1, _same_block(dev[i], ctrl[i - 1]))
        # the knob: armed before block k, by one call that found nothing armed, and nowhere else; disarmed by the block itself
        assert dev[k]['armed'] == [(0, 0, 0)] and all(b['armed'] == [] for i, b in enumerate(dev) if i != k)
        assert [b['status_before'][0] for b in dev] == [0] * k + [code] + [0] * B.STATUS_TAIL
        assert [b['status_info'][0] for b in dev] == [0] * n
        # handoff_off: set by the hand-off's block and kept, untouched by the other three
        off = name == 'handoff'
        assert [b['status_info'][1] for b in dev] == [1 if off and i >= k else 0 for i in range(n)], (lv, [b['status_info'] for b in dev])
        assert [b['status_before'][1] for b in dev] == [1 if off and i > k else 0 for i in range(n)]
    dev = runs[0][0]
    if not early:          # (nothing is stated about recordings while the structural blocks are still changing)
        d = _delta(dev[k + 1])
        if name == 'handoff':          # every graph was destroyed, and the attraction step's place is in the key
            assert d['captured'] >= 1 and d['replayed'] == 1 and d['direct'] == 0, d
        else:                          # the key did not change and the ring was kept
            assert d == dict(captured=0, replayed=1, direct=0), d
    _anchor(label, dev, steps)


@pytest.mark.parametrize('early', [False, True], ids=['late', 'early'])
def test_search_runs_the_block_again_after_a_hand_off(early):
    """The default (ShrinkwrapMeshConjGrad.handoff_retries = 1): the caller sees nothing but the result."""
    steps, _ = B.status_case('handoff', early)
    k, n = 1 if early else B.OPENING, len(steps)
    steps[k] = dict(steps[k], raises=None)
    searches = [2 if i == k else 1 for i in range(n)]
    runs = _run_levels('handoff_retried%s' % ('-early' if early else ''), steps, searches=searches)
    ctrl = _control(n)
    for lv in LEVELS:
        dev = runs[lv][0]
        assert [b['error'] for b in dev] == [None] * n
        for i in range(n):
            assert _equals_control(dev[i], ctrl[i]) == [], 'level %d, block %d differs from the control in %s' % (lv, i, _same_block(dev[i], ctrl[i]))
        assert [b['loopcount'] for b in dev] == [3] * n
        assert [len(b['tests']) for b in dev] == [3] * n and [len(b['ress']) for b in dev] == [3] * n          # the armed block's logs neither lost nor doubled
        assert dev[k]['status_before'] == (B.STATUS_CODES['handoff'], 0)
        assert [b['status_info'] for b in dev] == [(0, 1 if i >= k else 0) for i in range(n)]
    if not early:          # the second call found every graph destroyed and another key: it recorded, and both calls were replayed
        d = _delta(runs[0][0][k])
        assert d['captured'] >= 1 and d['replayed'] == 2 and d['direct'] == 0, d


def test_a_hand_off_in_a_block_that_stays_on_the_device():
    """the armed block runs with to_host=False (both paths of search() retry); the first result brought to the host is the control's"""
    steps, _ = B.build([dict(pre=[('raise_status', 'handoff')], to_host=False), dict(to_host=True)], tail=1)
    k, n = B.OPENING, len(steps)
    runs = _run_levels('handoff_retried_on_the_device', steps, searches=[2 if i == k else 1 for i in range(n)])
    ctrl = _control(n)
    for lv in LEVELS:
        dev = runs[lv][0]
        assert [b['error'] for b in dev] == [None] * n and [b['loopcount'] for b in dev] == [3] * n
        assert dev[k]['positions'] is None and [len(b['tests']) for b in dev] == [3] * n
        assert _equals_control(dev[k], ctrl[k], skip=('positions', 'mesh_positions')) == []          # (not brought to the host in that block)
        for i in [i for i in range(n) if i != k]:
            assert _equals_control(dev[i], ctrl[i]) == [], 'level %d, block %d differs from the control in %s' % (lv, i, _same_block(dev[i], ctrl[i]))
        assert [b['status_info'] for b in dev] == [(0, 1 if i >= k else 0) for i in range(n)]


def test_back_inside_the_query_launch_after_a_hand_off():
    """separate_attraction(False) after a hand-off: the key is the opening's again, but every graph recorded under it was destroyed --
    none of those slots may be replayed; the block records anew and equals the control's."""
    steps, _ = B.build([dict(pre=[('raise_status', 'handoff')]), dict(pre=[('separate_attraction', False)])], tail=1)
    k, n = B.OPENING, len(steps)
    assert n == k + 3
    runs = _run_levels('handoff_then_back_inside', steps, searches=[2 if i == k else 1 for i in range(n)])
    ctrl = _control(n)
    for lv in LEVELS:
        dev = runs[lv][0]
        assert [b['error'] for b in dev] == [None] * n and [b['loopcount'] for b in dev] == [3] * n
        for i in range(n):
            assert _equals_control(dev[i], ctrl[i]) == [], 'level %d, block %d differs from the control in %s' % (lv, i, _same_block(dev[i], ctrl[i]))
        assert [b['status_info'][1] for b in dev] == [0] * k + [1, 0, 0]          # the getter reads 0 again
        assert dev[k + 1]['status_before'] == (0, 0)
    d = _delta(runs[0][0][k + 1])
    assert d['captured'] >= 1 and d['replayed'] == 1 and d['direct'] == 0, d


def test_the_knob_refuses_what_it_should():
    """nw_debug(what = 8) through ctypes on a live context: a code outside the four is NW_ERR_BADARG and changes nothing (neither a
    clean context nor an armed one), arming twice keeps the last code, code 0 disarms."""
    changes = [dict(pre=[('raise_status', 12345)]),
               dict(pre=[('raise_status', 'nan'), ('raise_status', 'singular')], raises='singular'),
               dict(pre=[('raise_status', 'internal'), ('raise_status', 0)]),
               dict(pre=[('raise_status', 'internal'), ('raise_status', -8)], raises='internal')]          # (-8, NW_ERR_REMOTE: a status, but no single-rank one)
    steps, _ = B.build(changes, tail=1)
    k, n = B.OPENING, len(steps)
    dev, _ = B.run_device(steps, 0, handoff_retries=0)
    ctrl = _control(n)
    assert [b['error'] for b in dev] == [None] * k + [None, 'singular', None, 'internal', None]
    assert dev[k]['armed'] == [(NW_ERR_BADARG, 0, 0)] and dev[k]['status_before'] == (0, 0)
    assert dev[k + 1]['armed'] == [(0, 0, 0), (0, B.STATUS_CODES['nan'], 0)] and dev[k + 1]['status_before'] == (B.STATUS_CODES['singular'], 0)
    assert CAUSE['singular'] in dev[k + 1]['message']
    assert dev[k + 2]['armed'] == [(0, 0, 0), (0, B.STATUS_CODES['internal'], 0)] and dev[k + 2]['status_before'] == (0, 0)
    assert dev[k + 3]['armed'] == [(0, 0, 0), (NW_ERR_BADARG, B.STATUS_CODES['internal'], 0)] and dev[k + 3]['status_before'] == (B.STATUS_CODES['internal'], 0)
    assert CAUSE['internal'] in dev[k + 3]['message']
    assert [b['status_info'] for b in dev] == [(0, 0)] * n
    # the blocks that ran are the control's, in order: two of the sequence's blocks did not count
    ran = [i for i in range(n) if dev[i]['error'] is None]
    assert ran == list(range(k + 1)) + [k + 2, k + 4]
    for j, i in enumerate(ran):
        assert _equals_control(dev[i], ctrl[j]) == [], 'block %d differs from the control\'s block %d in %s' % (i, j, _same_block(dev[i], ctrl[j]))
        assert dev[i]['loopcount'] == 3 and set(FIELDS) <= set(dev[i])
