"""
CPU test: the NumPy restatement of the self-intersection check (tests/mesh_intersections_ref.py) against ground truth -- closed forms,
hand-made touching cases, counts that follow from the geometry -- so that the device, which is asked for the restatement's answer bit
for bit (tests/test_hip_intersections.py), is tied to something other than itself.  At the end, three one-line mistakes in the
restatement that each turn one of these assertions red.
"""
import numpy as np
import pytest

import mesh_intersections_ref as R
from ch_shrinkwrap_amd.trimesh import icosphere


def n_pairs(v, f, mutate=None):
    return R.self_intersections(v, f, mutate)['n_pairs']


def check_cube_and_plane(mutate=None):
    v, f = R.cube_and_plane()
    r = R.self_intersections(v, f, mutate)
    assert r['n_pairs'] == 8 and r['n_crossed_faces'] == 9
    assert (r['count'][:4] == 0).all() and (r['count'][4:12] == 1).all() and r['count'][12] == 8          # z = 0 and z = 1 are not crossed
    assert np.array_equal(r['pairs'], np.stack([np.arange(4, 12), np.full(8, 12)], axis=1))


def check_two_triangles(mutate=None):
    for name, (B, expected) in R.TWO_TRIANGLES.items():
        for tris in ((R.A_TRI, B), (B, R.A_TRI)):
            assert n_pairs(*R.soup(*tris), mutate=mutate) == expected, name


def check_shared_corner(mutate=None):
    for ra in range(3):
        for rb in range(3):
            assert n_pairs(*R.shared_corner(True, ra, rb), mutate=mutate) == 1
            assert n_pairs(*R.shared_corner(False, ra, rb), mutate=mutate) == 0


# A's edge 0 -> 1 has corner 3 of the second face as its exact midpoint (float32), and the second face rises from there to one side of
# A's plane: they touch.  A's plane rejection says so from the signs of three dot products; without it A's edge is tested against a face
# with a corner on the edge's own line, and two of the three triple products are rounding noise.
TOUCHING_AT_AN_EDGE_MIDPOINT = np.array([
    [0.6150052547454834, 0.3103475570678711, -0.3494671583175659], [1.0062557458877563, -0.6114755868911743, 0.28693363070487976],
    [0.42215538024902344, 1.4788070917129517, -0.5054413676261902], [0.8106305003166199, -0.1505640149116516, -0.03126676380634308],
    [0.5135536789894104, 0.3572530448436737, 1.108161449432373], [-0.24615611135959625, -0.7976542115211487, -0.5400946736335754]], np.float32)


def check_touching_at_an_edge_midpoint(mutate=None):
    v = TOUCHING_AT_AN_EDGE_MIDPOINT
    d = v.astype(np.float64)
    assert np.array_equal(2 * d[3], d[0] + d[1])                                          # the midpoint, exactly
    n = np.cross(d[1] - d[0], d[2] - d[0])
    assert ((d[4:] - d[0]) @ n > 0.1).all() or ((d[4:] - d[0]) @ n < -0.1).all()           # the other two corners: one side, far from rounding
    assert n_pairs(v, np.array([[0, 1, 2], [3, 4, 5]], np.int32), mutate) == 0


def test_cube_cut_by_a_plane():
    check_cube_and_plane()


def test_two_triangles_crossing_and_touching():
    check_two_triangles()
    check_touching_at_an_edge_midpoint()


def test_shared_corner_under_every_corner_order():
    check_shared_corner()
    # touching: the far edge of the second face ends on A's interior
    v = np.concatenate([R.A_TRI, np.array([[1, 1, 0], [1, 2, 1]], np.float32)])
    assert n_pairs(v, np.array([[0, 1, 2], [0, 3, 4]], np.int32)) == 0


def test_shared_edge_is_not_examined():
    v = np.concatenate([R.A_TRI, np.array([[1, 1, -1], [1, 1, 1]], np.float32)])
    assert n_pairs(v, np.array([[0, 1, 2], [1, 0, 3]], np.int32)) == 0                     # a fold: the remesher's business
    assert n_pairs(v, np.array([[0, 1, 2], [3, 4, 1]], np.int32)) == 1                     # one shared corner: the far edge pierces A


def test_spheres_are_embedded():
    assert n_pairs(*icosphere(2)) == 0
    assert n_pairs(*R.noisy_sphere(0.05)) == 0


def test_crumpled_sphere():
    v, f = R.noisy_sphere(0.3)
    r = R.self_intersections(v, f)
    s = R.shared_corners(f, r['pairs'])
    assert r['n_pairs'] == 700 and (s == 0).sum() == 562 and (s == 1).sum() == 138 and (s >= 2).sum() == 0
    assert r['count'].sum() == 1400 and r['n_crossed_faces'] == (r['count'] > 0).sum()


@pytest.mark.parametrize('radius,centre', [(1.0, 0.0), (100.0, 1e6)])
def test_two_overlapping_spheres(radius, centre):
    v, f, n1 = R.two_spheres(radius, centre)
    r = R.self_intersections(v, f)
    p = r['pairs']
    assert r['n_pairs'] == 78 and ((p[:, 0] < n1) & (p[:, 1] >= n1)).all()               # every pair joins the two spheres
    # the faces in the pairs: those with corners on both sides of the other sphere
    d = v.astype(np.float64)
    c = [centre + radius * np.zeros(3), centre + radius * np.array([1.1, 0.13, 0.07])]
    expected = []
    for k, faces in enumerate((f[:n1], f[n1:])):
        inside = np.linalg.norm(d[faces] - c[1 - k], axis=2) < radius
        expected.append(np.flatnonzero(inside.any(1) & ~inside.all(1)) + k * n1)
    assert len(expected[0]) == 39 and len(expected[1]) == 39
    assert np.array_equal(np.unique(p), np.concatenate(expected)) and np.array_equal(np.flatnonzero(r['count']), np.unique(p))


def test_common_centroid_cushion():
    v, f = R.cushion()
    r = R.self_intersections(v, f)
    assert r['n_pairs'] == 190 and (r['count'] == 19).all() and r['n_crossed_faces'] == 20


def test_flat_faces_are_never_in_a_pair():
    v, f, flat = R.with_flat_faces()
    r = R.self_intersections(v, f)
    assert r['n_pairs'] == 78 and (r['count'][flat] == 0).all() and not np.isin(r['pairs'], flat).any()


def test_pairs_do_not_depend_on_the_face_order():
    for v, f in (R.noisy_sphere(0.3), R.cube_and_plane(), R.shared_corner(True)):
        nf = len(f)
        fwd, rev = R.self_intersections(v, f), R.self_intersections(v, f[::-1])
        back = np.sort(nf - 1 - rev['pairs'], axis=1)
        assert np.array_equal(back[np.lexsort((back[:, 1], back[:, 0]))], fwd['pairs'])
        assert np.array_equal(rev['count'][::-1], fwd['count'])


def test_one_and_two_faces():
    r = R.self_intersections(R.A_TRI, [[0, 1, 2]])
    assert r['n_pairs'] == 0 and r['n_crossed_faces'] == 0 and r['count'].tolist() == [0] and r['pairs'].shape == (0, 2)
    r = R.self_intersections(*R.soup(R.A_TRI, R.TWO_TRIANGLES['pierced'][0]))
    assert r['pairs'].tolist() == [[0, 1]] and r['count'].tolist() == [1, 1]


def test_strips_in_closed_form():
    for m in (1, 2, 65):
        v, f, expected = R.strip(m)
        r = R.self_intersections(v, f)
        assert np.array_equal(r['pairs'], expected) and (r['count'] == 1).all()


# ---- three one-line mistakes, each caught ---------------------------------------------------------------------------------------------------
def test_mutation_ge_for_gt_is_caught():
    with pytest.raises(AssertionError, match='edge_through_edge'):
        check_two_triangles('ge')


def test_mutation_wrong_opposite_edge_is_caught():
    with pytest.raises(AssertionError):
        check_shared_corner('wrong_edge')
    v, f = R.noisy_sphere(0.3)
    assert n_pairs(v, f, 'wrong_edge') != 700


def test_mutation_plane_rejection_dropped_on_one_side_is_caught():
    with pytest.raises(AssertionError):
        check_touching_at_an_edge_midpoint('one_plane')
    check_cube_and_plane('one_plane')                                                      # (what it costs is only seen where faces touch)
