"""
CPU tests of tests/remesh_device_ref.py, the plain restatement of nw_remesh_device that tests/test_hip_remesh_edges.py compares the
kernels with: on the restatement alone, every input of tests/remesh_edge_cases.py reaches the branches it is there for (info['log']), the
result is an oriented mesh of the input's Euler characteristic with the input's boundary, the restatement's own checks held (disjoint
footprints, writes inside them, twin / vhe / val after every round: they are assertions inside it), and no run takes more than 2 s.  On
the one-operation inputs (one split, one collapse, one flip; a collapse turned away for the long edge it would make, by the link condition on a
3-cycle that is no face, by the fold test's sign and by its cosine, a flip turned away for its dihedral angle and for a triangle of no area) the serial host remesher
(csrc/remesh.cpp, whose admission tests the device claims) gives the same triangles.
"""
import numpy as np
import pytest

import remesh_edge_cases as C
from ch_shrinkwrap_amd import remesh as R
from remesh_device_ref import remesh_device_ref, Refused, key_of


def _topology(v, f):
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    assert np.unique(d, axis=0).shape[0] == d.shape[0], 'a directed edge twice: not oriented'
    ue, cnt = np.unique(np.sort(d, 1), axis=0, return_counts=True)
    assert cnt.max() <= 2
    return np.unique(f).size - ue.shape[0] + f.shape[0], int((cnt == 1).sum())


@pytest.mark.parametrize('name', list(C.CASES))
def test_restatement_reaches_its_branches_and_gives_a_valid_mesh(name):
    v, f = C.inputs(name)
    rv, rf, info, dt = C.reference(name)
    print(name, dt, {k: info[k] for k in info if k != 'log'}, info['log'])
    for k, n in C.EXPECT[name].items():
        if k in info:
            assert info[k] == n, (k, info[k])
        else:
            assert info['log'].get(k, 0) >= n > 0 or info['log'].get(k, 0) == n == 0, (k, info['log'])
    assert rf.min() == 0 and rf.max() == rv.shape[0] - 1 and np.isfinite(rv).all()
    assert _topology(rv, rf) == _topology(v, f)
    assert info['n_split'] - info['n_collapse'] == rv.shape[0] - np.unique(f).size
    assert rf.shape[0] <= 8200 and f.shape[0] <= 1300
    assert dt <= 2.0


def test_what_the_cases_are_named_for():
    log = lambda name: C.reference(name)[2]['log']
    info = lambda name: C.reference(name)[2]
    # thresholds on a lattice edge (squared length 512): the float32 targets on either side fall on either side
    ops = [sum(info('oct_high_threshold_%d' % k)[x] for x in ('n_split', 'n_collapse', 'n_flip')) for k in range(3)]
    assert ops[0] > 0 and ops[2] == 0                     # a smaller L: 512 > high2; a larger one: nothing is too long
    ops = [info('oct_low_threshold_%d' % k)['n_collapse'] for k in range(3)]
    assert ops[0] == 0 and ops[2] > 0
    # frozen inputs come back as they are (renumbered)
    for name in ('strip', 'interior_edge_between_boundary_vertices'):
        v, f = C.inputs(name)
        rv, rf, i, _ = C.reference(name)
        assert i['n_split'] + i['n_collapse'] + i['n_flip'] == 0 and i['frozen'] == v.shape[0] and np.array_equal(rv[rf], v[f])
    # a degree-65 apex is frozen (the ring walk's limit is 64), a degree-64 apex is not
    for shape in ('bipyramid', 'crown'):
        assert info(shape + '_65')['frozen'] == 2 and info(shape + '_65')['max_valence'] >= 65 and info(shape + '_64')['frozen'] == 0
    # ... and passes 64 where the rim splits: from then on the walk round it does not close.  No collapse or flip gets as far as that walk
    # (60 is the largest max_valence there is, and the degree tests come first); the relaxation walks it, and leaves the apex where it was
    assert info('crown_64')['peak_valence'] > 64 and info('crown_64_relax')['max_valence'] > 64
    assert not any(k in log(name) for name in C.CASES for k in ('collapse:ring_of_a', 'collapse:ring_of_b', 'flip:ring_of_c'))
    v, _ = C.inputs('crown_64_relax')
    rv = C.reference('crown_64_relax')[0]
    assert all((rv == v[k]).all(1).any() for k in (64, 65)), 'an apex of degree above 64 was moved'
    # 60 is the largest max_valence there is: where the apex is at it (the flat rim never splits: nothing comes near)
    for shape in ('bipyramid', 'crown'):
        a, b = C.reference(shape + '_60_max_60'), C.reference(shape + '_60_max_100')
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert info('crown_60_max_100')['peak_valence'] > 60
    assert info('bow_tie')['frozen'] == 1 and info('tetrahedron_far_above')['n_collapse'] == 0
    # unreferenced slots are dropped, and what is far away does not stretch the result
    assert np.abs(C.reference('spare_slots')[0]).max() < 60.0
    # the admission branches that some input reaches; UNREACHED lists the others, each with what keeps the inputs from it
    seen = set()
    for name in C.CASES:
        seen |= set(log(name))
    want = {'split:bid', 'split:short_enough_now', 'collapse:frozen', 'collapse:degree_cd_at_most_3', 'collapse:degree_sum_above_max',
            'collapse:long_edge', 'collapse:link_3', 'collapse:fold_sign', 'collapse:fold_cosine', 'collapse:bid_h', 'collapse:bid_twin', 'collapse:long_enough_now',
            'flip:frozen', 'flip:degree_ab_at_most_3', 'flip:max_valence', 'flip:no_gain_now', 'flip:dihedral', 'flip:orientation_0', 'flip:orientation_1', 'flip:skew',
            'flip:area', 'flip:bid', 'flip:bid_at_max_valence', 'flip:already_joined', 'flip:no_area'}
    print(sorted(seen))
    assert want <= seen, want - seen
    assert seen - want <= {'collapse:link_%d' % k for k in range(70)} and not (seen & set(UNREACHED)), seen - want
    # inputs that are not dyadic stay clear of rounding: no comparison closer to equality than 1e-9 unless it is exactly there (a midpoint
    # on the line it was taken from gives cross products of exactly 0: those ties are counted apart, in `margin`).  On the lattices every
    # operand is exact, however close.
    for name in C.CASES:
        m = info(name)['margin_nonzero']
        print(name, info(name)['margin'], m, info(name)['margin_rounded'])
        assert m > 1e-9 or name.startswith('oct_') or name.startswith('cube_'), (name, m)


# what the restatement can log and no input can reach: every one is a test that an earlier test has answered
UNREACHED = {
    'split:both_frozen': 'the candidate scan has turned such an edge away, and nothing freezes a vertex later',
    'collapse:c_is_d': 'the candidate scan has turned such an edge away; a collapse that passed the link condition makes none',
    'collapse:degree_ab_below_3': 'a vertex of degree 2 whose fan closes has c == d on both its edges, which is tested before',
    'collapse:degree_sum_below_3': 'val a = val b = 3 on a closed fan is the tetrahedron, whose c and d have degree 3, which is tested before',
    'collapse:ring_of_a': 'a fan that does not close is frozen; past 64 the degree sum is above max_valence (at most 60), which is tested before',
    'collapse:ring_of_b': 'as ring_of_a',
    'collapse:open_twin': 'an open edge freezes both its ends, which is tested first',
    'flip:c_is_d': 'the candidate scan has turned such an edge away',
    'flip:ring_of_c': 'val c + 1 <= max_valence <= 60 has been tested before, and a fan that does not close is frozen',
}


def test_keys_and_refusals():
    assert key_of(0, 0) == 0 and key_of(65, 7) >> 32 < 65536 and (key_of(65, 7) & 0xffffffff) == 7
    v, f = C.inputs('octahedron_far_below')
    g = f.copy(); g[0, 1] = g[0, 0]
    bad = v.copy(); bad[0, 0] = np.inf
    far = v.copy(); far[0] *= 1e7
    for vv, ff in ((v, g), (bad, f), (far, f), (v, np.where(f == 5, 6, f))):
        with pytest.raises(Refused, match='bad argument'):
            remesh_device_ref(vv, ff, 1, 2.5)
    with pytest.raises(Refused, match='non-manifold'):
        remesh_device_ref(v, np.vstack([f, f[:1]]), 1, 2.5)


@pytest.mark.parametrize('name', C.ONE_OPERATION)
def test_one_operation_is_the_serial_host_remeshers(name):
    """the tie to csrc/remesh.cpp: one edge too long or too short, or one flip that gains -- or nothing but refusals; one iteration; the same set of
    triangles over the same positions (tests/remesh_edge_cases.py says what each input is, and EXPECT, checked above, that it is the operation or the
    refusals it is named for)"""
    v, f = C.inputs(name)
    rv, rf, info, _ = C.reference(name)
    print(info)
    # no order to differ in: one bidder per round, or nothing but refusals (a list of candidates that are all turned away takes one round)
    assert max(info['rounds']) <= 2 and max(info['passes']) <= 1
    assert max(info['n_split'], info['n_collapse'], info['n_flip']) <= 1
    hv, hf = R.remesh(v, f, 1, C.kwargs(name)['L'], 0.5, 0, serial=True)
    tri = lambda x, y: sorted(tuple(map(tuple, np.roll(t, -int(np.lexsort(t.T[::-1])[0]), 0).tolist())) for t in x[y])
    assert tri(rv, rf) == tri(hv, hf)
