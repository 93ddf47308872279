"""
GPU tests of nw_remesh_device (csrc/nw_remesh_dev.hip) against its plain restatement, tests/remesh_device_ref.py, bit for bit: the unit is
built without contraction, keeps positions in float64, takes priorities from a hash and ids from prefix sums, so its arrays are a function
of its input -- the one the restatement writes down.  For every input of tests/remesh_edge_cases.py (dyadic lattices with thresholds on a
lattice edge, the smallest and largest degrees, one admission branch each, open and untidy meshes, many operations at once): the same faces,
the same bits in the float32 vertices, the same operation counts and largest degree, the mean edge to 1e-12 (a block-wise sum of at most a
few 10^4 doubles in another order), rounds per kind between the restatement's and two more per non-empty pass (what the host may run ahead),
and the same arrays from a second run.
"""
import numpy as np
import pytest

import remesh_edge_cases as C
from ch_shrinkwrap_amd import remesh as R
from remesh_device_ref import remesh_device_ref

pytestmark = pytest.mark.gpu


def _same(dv, df, st, rv, rf, info):
    assert df.shape == rf.shape and np.array_equal(df, rf)
    assert dv.shape == rv.shape and np.array_equal(dv.view('u4'), rv.view('u4'))
    for k in ('n_split', 'n_collapse', 'n_flip', 'max_valence'):
        assert st[k] == info[k], (k, st[k], info[k])
    assert abs(st['mean_edge_length'] - info['mean_edge_length']) <= 1e-12 * info['mean_edge_length']
    for k in range(3):
        assert info['rounds'][k] <= st['rounds'][k] <= info['rounds'][k] + 2 * info['passes'][k], (st['rounds'], info['rounds'], info['passes'])


@pytest.mark.parametrize('name', list(C.CASES))
def test_device_remesher_is_its_restatement(name):
    v, f = C.inputs(name)
    rv, rf, info, _ = C.reference(name)
    dv, df, st = R.remesh_device(v, f, return_stats=True, **{'target_edge_length' if k == 'L' else k: x for k, x in C.kwargs(name).items()})
    print(name, st, {k: info[k] for k in info if k != 'log'})
    _same(dv, df, st, rv, rf, info)
    dv2, df2 = R.remesh_device(v, f, **{'target_edge_length' if k == 'L' else k: x for k, x in C.kwargs(name).items()})
    assert np.array_equal(dv2.view('u4'), dv.view('u4')) and np.array_equal(df2, df)


def test_chained_call():
    """a result fed back in: the second call's input is the first one's output, on the device and in the restatement"""
    name = 'icosphere3_x0.70_n1'
    rv, rf, info, _ = C.reference(name)
    L = 1.3 * C.CASES[name][1]['L']
    rv2, rf2, info2 = remesh_device_ref(rv, rf, 2, L)
    dv, df = R.remesh_device(*C.inputs(name), n=1, target_edge_length=C.CASES[name][1]['L'])
    dv2, df2, st2 = R.remesh_device(dv, df, 2, L, return_stats=True)
    _same(dv2, df2, st2, rv2, rf2, info2)


def test_retry_with_more_room_on_a_dyadic_input(monkeypatch):
    """NW_REMESH_ROOM=0.05: an attempt has room for 8192 faces at least, so running out takes a call that uses more face slots than that -- a
    cube's lattice of 768 faces at a target that calls for some 15 000 slots: five attempts run out before one fits, and the result is the
    restatement's all the same.  (The restatement needs 3 s for this input without its own checks, which the other inputs have had: this is
    the module's one slow test.)"""
    v, f = C.lattice(C.cube, 3)
    rv, rf, info = remesh_device_ref(v, f, 1, 6.0, check=False)
    assert f.shape[0] + 2 * info['n_split'] > 4 * 8192 // 3
    monkeypatch.setenv('NW_REMESH_ROOM', '0.05')
    dv, df, st = R.remesh_device(v, f, 1, 6.0, return_stats=True)
    print(st, {k: info[k] for k in info if k != 'log'})
    _same(dv, df, st, rv, rf, info)
    monkeypatch.delenv('NW_REMESH_ROOM')
    dv2, df2 = R.remesh_device(v, f, 1, 6.0)
    assert np.array_equal(dv2.view('u4'), dv.view('u4')) and np.array_equal(df2, df)
