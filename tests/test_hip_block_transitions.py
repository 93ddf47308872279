"""
GPU tests (run with -m gpu on an MI355X): ONE fit context kept alive across blocks while the caller changes something between them --
the path every real fit takes (membrane_mesh.py: a new optimiser per block on a shared NativeContext, another cloud, another mesh,
other weights, another block length), and the one on which a block is replayed from a hipGraph while "nothing it bakes in has changed"
(block_graph_key() in csrc/nanowrap.hip: a hand-kept hash beside kernels that take dozens of arguments by value).

tests/block_sequence_ref.py holds the sequences and plays them on the device (run_device) and through the oracle (run_oracle).  Every
sequence opens with five identical blocks, then the change (one block per stage), then two more identical blocks.  Each case asserts:

 1. replay equals direct launches, bit for bit: after EVERY block, profiling levels 0 (graphs), 1 (every launch from the host) and 4
    (head graph + live last iteration, what bench.py times) return array_equal positions, nearest faces, S, res, tests, ress, loopcount
    (the equality test_profiling_levels_do_not_change_the_result holds for unchanged blocks; no tolerance);
 2. the replay path ran: at level 0 every block is replayed from a graph and none launched directly, a changed key shows as exactly one
    more recording and a key that is still in the ring as none (_expected_recordings restates the ring and what the key holds; a block
    of a mesh with deferred rows alternates between the two halves of the result's staging buffer, whose address is in the key, so a
    shape is recorded once per half; where an address in the key depends on the allocator -- the log buffer after a longer block --
    nothing is stated); level 1 records and replays nothing (graph_stats(), nw_debug what = 7);
 3. the change is visible: the block after a value change differs from the same block of a control sequence without it (level 1) -- a
    stale graph would not show it --, a transport-only change (second lambda, to_host, optimize_layout, separate_attraction, reset of
    the history without a stop) leaves every block array_equal to the control's;
 4. an independent anchor: the device's positions after the last block lie within rel_rms <= 1e-4 of the oracle's (the bound of
    tests/test_hip_parity.py for a full run) and the last block's `ress` agree to rtol 1e-4 (test_against_oracle_fresh_inputs) -- for the
    cases whose change moves the oracle by at least ten times that bound (tests/test_block_sequence_ref.py, CPU) and for the
    transport-only ones; `last_step_off` and `refresh_normals` move it by less and are dropped from the anchor (block_sequence_ref.CASES).
"""
import time

import numpy as np
import pytest

import block_sequence_ref as B

pytestmark = pytest.mark.gpu

LEVELS = (0, 1, 4)
FIELDS = ('positions', 'mesh_positions', 'nearest_face', 'S', 'res', 'tests', 'ress')
ANCHOR_BOUND = 1e-4
VARIANTS = [(c, early) for c in B.CASES for early in ((False, True) if c.early else (False,))]


@pytest.fixture(scope='module', autouse=True)
def _module_duration():
    t0 = time.time()
    yield
    print('\ntests/test_hip_block_transitions.py: %.1f s' % (time.time() - t0))


def _same_block(a, b):
    """names of the fields in which two records of one block differ"""
    bad = [k for k in ('error', 'loopcount') if a[k] != b[k]]
    for k in FIELDS:
        x, y = a.get(k), b.get(k)
        if (x is None) != (y is None) or (x is not None and not np.array_equal(x, y)):
            bad.append(k)
    return bad


def _delta(b):
    return {k: b['after'][k] - b['before'][k] for k in ('captured', 'replayed', 'direct')}


def _expected_recordings(steps):
    """Restates, for the blocks that `stated` marks, the ring of recorded graphs (8 slots, round-robin) and the part of
    block_graph_key() these sequences touch: lam0, num_iters, the flags, the residual target, the quantum, the attraction step's place,
    whether the scatter accumulator must be zeroed first,
    where the result goes -- with deferred rows (TriMesh) the block's half of the staging buffer, which alternates --, and the structure
    of the first blocks of a context (cold query; projection re-sort and k-d list; from the fourth block on the list ordered by cost).
    Holds while no new grid is laid and nothing is uploaded: block_sequence_ref.build() marks no other block.  None: no statement."""
    half, out, most = 0, [], 0
    separate, quantum, dirty = False, None, False
    # What the ring may hold: per recording its key, how many recordings have been made since at least / at most (it is overwritten by
    # the eighth), and whether it is `stale`: made before the block's log buffer grew (num_iters above every block so far: freed and
    # allocated again; its address is in the key, and whether the allocator hands the old address back is not the library's to say)
    ring = []

    def visit(key):
        mine = [e for e in ring if e['key'] == key and e['least'] < 8]
        if any(not e['stale'] and e['most'] < 8 for e in mine):
            n = 0                                                   # certainly still there
        elif not mine:
            n = 1                                                   # never recorded, or certainly overwritten
        else:
            n = None                                                # no statement
        for e in ring:
            e['least'] += 1 if n == 1 else 0
            e['most'] += 0 if n == 0 else 1
        if n != 0:          # (now it is there, at the latest since this visit; if it was there already, for as long as the oldest candidate)
            ring.append(dict(key=key, least=0, most=max([e['most'] for e in mine], default=0), stale=False))
        return n

    def key_of(i, a, h):
        return (0 if i == 0 else (1 if i < 3 else 2), a['lams'][0], a['num_iters'], a['pos'], a['last_step'], a['regulariser'], a['data'], a['sigma_inv'], a['weights'], separate, quantum, dirty, h)

    prev = None
    for i, st in enumerate(steps):
        n = 0
        for what, arg in st['pre']:
            if what == 'separate_attraction':
                separate = bool(arg)
            elif what == 'quantum':
                quantum = arg
            elif what == 'refresh_normals':
                dirty = True          # (nw_refresh_normals sums in the scatter accumulator: the next block's first launch zeroes it, a flag it takes by value)
            elif what == 'optimize_layout' and prev is not None:
                n = visit(prev)           # pre-records a repeat of the last block as it was (its half of the staging buffer included)
        a = st['search']
        if a['num_iters'] > most:
            most = a['num_iters']
            for e in ring:
                e['stale'] = i > 0
        if a['to_host']:
            half ^= 1
        prev = key_of(i, a, half if a['to_host'] else None)
        m = visit(prev)
        dirty = False
        out.append(n + m if st['stated'] and n is not None and m is not None else None)
    return out


def _run_levels(name, steps, mesh0='m3', points0='p6', searches=None, **device):
    """searches: how many calls of nw_search each block makes (one, unless search() runs a block again: tests/test_hip_block_status.py);
    device: further arguments of run_device"""
    searches = [1] * len(steps) if searches is None else searches
    runs = {lv: B.run_device(steps, lv, mesh0, points0, **device) for lv in LEVELS}
    _report(name, steps, runs[0])
    # 1. replay equals direct launches, after every block
    for lv in (1, 4):
        for i, (a, b) in enumerate(zip(runs[0][0], runs[lv][0])):
            assert _same_block(a, b) == [], 'block %d: level 0 and level %d differ in %s' % (i, lv, _same_block(a, b))
    # 2. the replay path ran
    want = _expected_recordings(steps)
    got = [_delta(b)['captured'] for b in runs[0][0]]
    for i, b in enumerate(runs[0][0]):
        d = _delta(b)
        assert d['replayed'] == searches[i] and d['direct'] == 0, 'level 0, block %d was not replayed from a graph: %s' % (i, d)
        assert want[i] is None or d['captured'] == want[i], 'level 0, block %d: recordings per block %s, stated %s' % (i, got, want)
    n = sum(searches)
    assert runs[1][1] == dict(captured=0, replayed=0, direct=n), runs[1][1]
    head = sum(k for st, k in zip(steps, searches) if st['search']['num_iters'] > 1)
    assert runs[4][1]['replayed'] == head and runs[4][1]['direct'] == n - head, runs[4][1]
    return runs


def _report(name, steps, run0):
    blocks, stats = run0
    print('%s: level 0 made %d recordings and %d replays in %d blocks (recordings per block: %s)'
          % (name, stats['captured'], stats['replayed'], len(steps), ' '.join(str(_delta(b)['captured']) for b in blocks)))


def _anchor(name, dev, steps, mesh0='m3', points0='p6'):
    ora = B.run_oracle(steps, mesh0, points0)
    rms = B.rel_rms(dev[-1]['positions'], ora[-1]['positions'])
    print('%s: final positions against the oracle %.3e of the bbox diagonal (bound %.0e)' % (name, rms, ANCHOR_BOUND))
    assert dev[-1]['loopcount'] == ora[-1]['loopcount']
    assert rms <= ANCHOR_BOUND, rms
    assert np.allclose(np.asarray(dev[-1]['ress'], 'f8'), ora[-1]['ress'], rtol=1e-4)
    return ora


@pytest.mark.parametrize('case,early', VARIANTS, ids=['%s%s' % (c.name, '-early' if e else '') for c, e in VARIANTS])
def test_a_change_between_blocks_of_a_live_context(case, early):
    steps, control = case.steps(early)
    name = case.name + ('-early' if early else '')
    runs = _run_levels(name, steps)
    dev = runs[0][0]
    assert all(b['error'] is None and b['loopcount'] == st['search']['num_iters'] for b, st in zip(dev, steps))
    # 3. the change is visible (or, transport only, changes nothing)
    ctrl, _ = B.run_device(control, 1)
    first = 1 if early else B.OPENING
    if case.kind == 'transport':
        for i, (a, b) in enumerate(zip(dev, ctrl)):
            skip = ('positions', 'mesh_positions') if not steps[i]['search']['to_host'] else ()          # (not brought to the host in that block)
            assert [k for k in _same_block(a, b) if k not in skip] == [], 'block %d differs from the control in %s' % (i, _same_block(a, b))
    else:
        for i in range(first):
            assert _same_block(dev[i], ctrl[i]) == [], 'block %d (before the change) differs from the control' % i
        for i in range(first, len(steps)):
            assert 'positions' in _same_block(dev[i], ctrl[i]), 'block %d: the change made no difference' % i
    # 4. the oracle
    if case.anchor is not False:
        _anchor(name, dev, steps)


def test_a_stop_inside_a_block_then_a_reset_history():
    """The stop condition fires on the device inside the sixth block (600 iterations asked; the small well-posed sphere of
    test_stop_condition_fires_on_the_device on the 162-vertex mesh), then a new optimiser on the shared context (nw_reset_history only)
    and a block that must run all three iterations.  WHICH iteration the rule fires in is decided by 1e-7-level noise, so the oracle is
    held to what is well defined: it stops in that block too and not in the next, and both have converged onto the same surface."""
    steps = B.stop_case()
    runs = _run_levels('stop_then_reset_history', steps, 'm2', 'p4')
    dev = runs[0][0]
    k = B.OPENING
    assert [b['loopcount'] for b in dev[:k]] == [3] * k
    assert 3 < dev[k]['loopcount'] < B.STOP_LONG and len(dev[k]['tests']) == dev[k]['loopcount']
    assert dev[k + 1]['loopcount'] == 3
    ora = B.run_oracle(steps, 'm2', 'p4')
    print('stop: device after %d iterations of the long block, oracle after %d' % (dev[k]['loopcount'], ora[k]['loopcount']))
    assert 3 < ora[k]['loopcount'] < B.STOP_LONG and ora[k + 1]['loopcount'] == 3
    assert B.rel_rms(dev[-1]['positions'], ora[-1]['positions']) <= ANCHOR_BOUND
    assert np.allclose(np.asarray(dev[-1]['ress'], 'f8'), ora[-1]['ress'], rtol=1e-4)


def test_a_block_that_ends_in_nan_then_the_same_block_repaired():
    """NW_ERR_NAN is a status code, not a fault (test_nan_inside_an_iteration...): the mesh stays at the last good iterate, the context
    stays usable, and the repaired block -- replayed or launched directly -- is the block the sequence would have run anyway."""
    steps = B.nan_case()
    runs = _run_levels('nan_then_repaired', steps)
    dev = runs[0][0]
    k = B.OPENING
    assert [b['error'] for b in dev] == [None] * k + ['nan', None, None, None]
    assert np.isfinite(dev[k]['mesh_positions']).all()
    assert np.array_equal(dev[k]['mesh_positions'], dev[k - 1]['positions'])
    _, control = B.build([], tail=1)          # (six identical blocks)
    ctrl, _ = B.run_device(control, 1)
    assert _same_block(dev[k + 1], ctrl[k]) == [], _same_block(dev[k + 1], ctrl[k])
    _anchor('nan_then_repaired', dev, steps)


def test_ten_block_shapes_evict_and_re_record():
    """num_iters 2..6 x pos on / off in a row, then the first three again, three times over: the 8-slot ring with round-robin eviction
    has dropped them and records each again on its first revisit; the next visit with the same half of the staging buffer (the third:
    the halves alternate from block to block, and three is odd) replays that recording without another."""
    steps, n = B.eviction_case()
    runs = _run_levels('eviction', steps)
    blocks, stats = runs[0]
    assert stats['captured'] >= 11
    k = B.OPENING + n
    for b in blocks[k:k + 3]:
        assert _delta(b) == dict(captured=1, replayed=1, direct=0), _delta(b)
    for b in blocks[k + 6:k + 9]:
        assert _delta(b) == dict(captured=0, replayed=1, direct=0), _delta(b)
