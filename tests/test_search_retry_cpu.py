"""CPU tests of what ShrinkwrapMeshConjGrad.search does with the status nw_search returns: NW_ERR_HANDOFF ("run the block again",
include/nanowrap.h) makes it ask once more for the iterations that are left, every other status is raised as before.  A stub stands in
for the native library (self._L), in the style of test_driver.py's recorder: no GPU and no libnanowrap_hip.so are needed.

The case of a hand-off after two of five iterations exists ONLY here: the device injection of tests/test_hip_block_status.py
(nw_debug(what = 8)) always fails in a block's iteration 0, so on the GPU the second call always asks for the whole block."""
import ctypes

import numpy as np
import pytest

from ch_shrinkwrap_amd import _lib as nw
from ch_shrinkwrap_amd.mesh_conj_grad import ShrinkwrapMeshConjGrad
from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere

MESSAGES = {nw.NW_ERR_NAN: b'NaN detected', nw.NW_ERR_SINGULAR: b'singular subspace normal equations', nw.NW_ERR_INTERNAL: b'invalid face id',
            nw.NW_ERR_HANDOFF: b'separate launches: run the block again'}


class _StubLibrary(object):
    """every entry point returns NW_OK and is noted; nw_search plays `script`, a list of (status, iterations executed): it fills that
    many log records (test = 100 * call + iteration), the count, and -- where a result is asked for -- the result with the call's number"""

    def __init__(self, script):
        self.script, self.calls, self.searches, self.last = list(script), [], [], b''

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return nw.NW_OK
        return entry

    def nw_last_error(self, h):
        return self.last

    def nw_search(self, h, lams, n_lams, num_iters, flags, out, logs, lc):
        call = len(self.searches)
        code, executed = self.script[call]
        assert executed <= num_iters <= len(logs)
        self.searches.append(dict(num_iters=num_iters, flags=flags, n_lams=n_lams, out=None if out is None else out.value, logs=logs))
        self.calls.append(('nw_search', (num_iters,)))
        for i in range(executed):
            logs[i].test, logs[i].res_norm, logs[i].executed = 100.0 * call + i, 1.0, 1
        lc._obj.value = executed
        if out is not None:
            n = 3 * self.M
            (ctypes.c_float * n).from_address(out.value)[:] = [float(call + 1)] * n
        self.last = MESSAGES.get(code, b'')
        return code


class _StubNative(object):
    def __init__(self, L):
        self.L, self.h, self.points_key = L, ctypes.c_void_p(1), None

    def check(self, code):
        nw.check(self.L, self.h, code)


def _optimiser(script, retries=None):
    v, f = icosphere(1, 10.0)
    mesh = TriMesh(v, f)
    L = _StubLibrary(script)
    L.M = v.shape[0]
    pts = np.random.default_rng(5).normal(size=(30, 3)).astype('f4')
    cg = ShrinkwrapMeshConjGrad(mesh, pts, native=_StubNative(L))
    if retries is not None:
        cg.handoff_retries = retries
    del L.calls[:]
    return cg, L, mesh, pts


def _write_backs(L):
    return [args[1] for name, args in L.calls if name == 'nw_set_write_back']


def test_the_retry_count_is_a_class_attribute_of_one():
    assert ShrinkwrapMeshConjGrad.handoff_retries == 1


@pytest.mark.parametrize('to_host', [True, False], ids=['to_host', 'device_only'])
def test_a_hand_off_in_the_first_iteration_runs_the_whole_block_again(to_host):
    cg, L, mesh, pts = _optimiser([(nw.NW_ERR_HANDOFF, 0), (nw.NW_OK, 5)])
    out = cg.search(pts, lams=[10.0], num_iters=5, to_host=to_host)
    assert [s['num_iters'] for s in L.searches] == [5, 5]                    # two calls, the second with num_iters unchanged
    assert L.searches[0]['flags'] == L.searches[1]['flags'] and L.searches[0]['out'] == L.searches[1]['out']
    assert [float(t) for t in cg.tests] == [100.0, 101.0, 102.0, 103.0, 104.0]          # logs consumed once: the second call's
    assert len(cg.ress) == 5 and cg.loopcount == 5 and len(cg.iter_logs) == 5
    if to_host:
        ws = _write_backs(L)
        assert len(ws) == 2 and ws[0] is not None and ws[1] is None          # set once, nw_set_write_back(None) once
        assert out is cg.fs and out.shape == (L.M, 3) and out.dtype == np.float32 and (out == 2.0).all()      # the second call's result
        assert L.searches[0]['flags'] & nw.NW_FLAG_ROWS_ASYNC and mesh.__dict__['_rows_pending'] is not None
    else:
        assert out is None and _write_backs(L) == [] and L.searches[0]['out'] is None


@pytest.mark.parametrize('to_host', [True, False], ids=['to_host', 'device_only'])
def test_a_hand_off_after_two_of_five_iterations_asks_for_the_other_three(to_host):
    cg, L, mesh, pts = _optimiser([(nw.NW_ERR_HANDOFF, 2), (nw.NW_OK, 3)])
    cg.search(pts, lams=[10.0], num_iters=5, to_host=to_host)
    assert [s['num_iters'] for s in L.searches] == [5, 3]
    assert len(L.searches[1]['logs']) == 3
    assert [float(t) for t in cg.tests] == [0.0, 1.0, 100.0, 101.0, 102.0]          # 2 + 3 entries, in order, none lost or doubled
    assert cg.loopcount == 5 and len(cg.iter_logs) == 5
    assert len(_write_backs(L)) == (2 if to_host else 0)


@pytest.mark.parametrize('to_host', [True, False], ids=['to_host', 'device_only'])
def test_a_second_hand_off_is_raised(to_host):
    cg, L, mesh, pts = _optimiser([(nw.NW_ERR_HANDOFF, 0), (nw.NW_ERR_HANDOFF, 0), (nw.NW_OK, 5)])
    with pytest.raises(nw.NanoWrapError) as e:
        cg.search(pts, lams=[10.0], num_iters=5, to_host=to_host)
    assert e.value.code == nw.NW_ERR_HANDOFF and 'separate launches' in str(e.value)
    assert len(L.searches) == 2 and cg.tests == []
    if to_host:          # as for any other raise (compare test_other_statuses_are_raised_without_a_second_call): rows marked pending, write-back dropped
        assert mesh.__dict__['_rows_pending'] is not None
        ws = _write_backs(L)
        assert len(ws) == 2 and ws[1] is None
        mesh.vertices                                                         # (reading the mesh waits for the rows: nw_synchronize)
        assert mesh.__dict__['_rows_pending'] is None and L.calls[-1][0] == 'nw_synchronize'


@pytest.mark.parametrize('to_host', [True, False], ids=['to_host', 'device_only'])
def test_no_retries_gives_the_raw_code(to_host):
    cg, L, mesh, pts = _optimiser([(nw.NW_ERR_HANDOFF, 0), (nw.NW_OK, 5)], retries=0)
    with pytest.raises(nw.NanoWrapError) as e:
        cg.search(pts, lams=[10.0], num_iters=5, to_host=to_host)
    assert e.value.code == nw.NW_ERR_HANDOFF and len(L.searches) == 1
    assert len(_write_backs(L)) == (2 if to_host else 0)


@pytest.mark.parametrize('to_host', [True, False], ids=['to_host', 'device_only'])
@pytest.mark.parametrize('code,exc', [(nw.NW_ERR_NAN, AssertionError), (nw.NW_ERR_SINGULAR, np.linalg.LinAlgError), (nw.NW_ERR_INTERNAL, nw.NanoWrapError)],
                         ids=['nan', 'singular', 'internal'])
def test_other_statuses_are_raised_without_a_second_call(code, exc, to_host):
    cg, L, mesh, pts = _optimiser([(code, 0), (nw.NW_OK, 5)])
    with pytest.raises(exc) as e:
        cg.search(pts, lams=[10.0], num_iters=5, to_host=to_host)
    assert len(L.searches) == 1 and cg.tests == []
    assert MESSAGES[code].decode() in str(e.value)
    if exc is nw.NanoWrapError:
        assert e.value.code == nw.NW_ERR_INTERNAL
    if to_host:
        assert mesh.__dict__['_rows_pending'] is not None
        ws = _write_backs(L)
        assert len(ws) == 2 and ws[1] is None
