"""
The NumPy restatement of the mesh-to-mesh distance (tests/mesh_proximity_ref.py) against ground truth that does not come from it:
closed forms, dense sampling of both triangles, integer-lattice cubes whose gap is exact, the self-intersection restatement's crossing
pairs, exact translations, and the cap of a sphere within a distance of another sphere.  Then three one-line mutations, each of which
turns one of these assertions red.  No GPU, no compiled code.
"""
import numpy as np
import pytest

import mesh_intersections_ref as X
import mesh_proximity_ref as P


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(P.CLOSED_FORMS))
def test_closed_forms_are_met_exactly(name):
    ta, tb, want, kinds = P.CLOSED_FORMS[name]
    d2, kind, ca, cb = P.tri_tri(ta, tb)
    assert d2 == want and not np.signbit(d2) and kind in kinds
    e = ca - cb
    assert (e * e).sum() == want                                          # the two closest points are that far apart
    if name.startswith('crossed_edges'):
        assert sorted(map(tuple, (ca, cb))) == [(0.0, 0.0, 0.0), (0.0, 0.0, 2.0)]
        import mesh_distance_ref as D
        ids = np.arange(3).reshape(1, 3)
        assert D.point_triangles(np.asarray(ta, float), np.asarray(tb, np.float32), ids)[0].min() == 8.0      # what A's corners alone would say


# ---- dense sampling ---------------------------------------------------------------------------------------------------------------------
def barycentric(n=61):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    keep = i + j <= n - 1
    u, v = i[keep] / (n - 1.0), j[keep] / (n - 1.0)
    return np.stack([1.0 - u - v, u, v], 1)                               # (n (n + 1) / 2, 3)


def sampled_distance(ta, tb, w):
    """the distance of the nearest pair among the samples of the two triangles: the pair is found through a matrix product, its
    distance is then taken directly"""
    pa, pb = w @ np.asarray(ta, np.float64), w @ np.asarray(tb, np.float64)
    g = (pa * pa).sum(1)[:, None] + (pb * pb).sum(1)[None, :] - 2.0 * (pa @ pb.T)
    i, j = np.unravel_index(np.argmin(g), g.shape)
    return float(np.sqrt(((pa[i] - pb[j]) ** 2).sum()))


def longest_edge(*tris):
    t = np.concatenate([np.asarray(x, np.float64).reshape(-1, 3, 3) for x in tris])
    return float(np.sqrt(((t - np.roll(t, 1, axis=1)) ** 2).sum(2)).max())


def check_against_samples(ta, tb, d2, w, pitch):
    """Every sample is a point of its triangle up to the rounding of a barycentric sum, so the exact distance is never above the
    sampled one (but for that rounding: 1e-12 of the size of the coordinates); and it is below it by at most the pitch times the
    longest edge."""
    worst = 0.0
    for a, b, x in zip(ta, tb, d2):
        s = sampled_distance(a, b, w)
        size = float(max(np.abs(a).max(), np.abs(b).max(), 1.0))
        assert np.sqrt(x) <= s + 1e-12 * size
        assert s - np.sqrt(x) <= pitch * longest_edge(a, b)
        worst = max(worst, s - np.sqrt(x))
    return worst


def test_random_pairs_against_61_by_61_samples_of_both_triangles():
    rng = np.random.default_rng(7)
    t = (rng.normal(size=(400, 2, 3, 3)) + rng.normal(size=(400, 2, 1, 3)) * rng.uniform(0, 2, (400, 1, 1, 1))).astype(np.float32)
    d2, kind, ca, cb = P.pairwise(t[:, 0], t[:, 1])
    assert sorted(set(kind.tolist())) == list(range(16))                                     # every kind is reached
    assert (d2[kind == 0] == 0).all() and not np.signbit(d2).any()
    e = ca - cb
    assert np.array_equal(X.dot(e, e), d2)                                                  # d2 is the distance of the two closest points
    worst = check_against_samples(t[:, 0], t[:, 1], d2, barycentric(61), 1.0 / 60)
    print('largest gap to the sampled distance: %.4f' % worst)


def test_needles_flat_faces_and_near_parallel_edges_against_samples():
    import mesh_distance_ref as D
    v, f = D.needles()
    t = v[f]
    w = barycentric(61)
    d2 = P.pairwise(t[:20], t[20:])[0]
    check_against_samples(t[:20], t[20:], d2, w, 1.0 / 60)
    flat = np.array([[[0, 0, 0], [0, 0, 0], [1, 0, 0]], [[0, 0, 0], [1, 1, 1], [2, 2, 2]], [[1, 2, 3], [1, 2, 3], [1, 2, 3]]], np.float32)
    other = np.array([[[0.5, 1, -1], [0.5, 3, -1], [0.5, 2, 2]], [[5, 2, 2], [2, 5, 2], [2, 2, 5.5]], [[1, 2, 5], [3, 2, 5], [1, 4, 6]]], np.float32)
    for ta, tb in ((flat, other), (other, flat), (flat, flat[::-1])):
        d2, kind, _, _ = P.pairwise(ta, tb)
        assert (kind > 0).all()                                                              # a flat face pierces nothing and is not pierced
        check_against_samples(ta, tb, d2, w, 1.0 / 60)
    assert P.tri_tri(flat[2], other[2])[0] == 4.0                                            # a point 2 below a face's corner
    # what the definition leaves out, on purpose: a flat face is skipped by the piercing tests, so one that passes through the other
    # face's interior is as far away as its corners and edges are
    assert P.tri_tri(flat[0], [[0.5, -1, -1], [0.5, 1, -1], [0.5, 0, 2]])[:2] == (0.25, 1)
    ta, tb = P.near_parallel_edges()
    for a, b in ((ta, tb), (tb, ta)):
        d2 = P.pairwise(a, b)[0]
        check_against_samples(a, b, d2, w, 1.0 / 60)
        assert np.abs(np.sqrt(d2) - 1.0).max() < 1e-8                                        # the edges are 1 apart, but for the 1e-9


def test_a_pair_a_million_from_the_origin_is_the_pair_at_the_origin():
    """integer corners moved by 10^6, which is exact in float32: the pair is the same pair, so the kind is the same and the distance
    differs by the rounding of closest points that are now computed at the size of 10^6 -- 2^-53 x 10^6 = 1.1e-10 an operation, a few
    operations each: within 1e-8"""
    rng = np.random.default_rng(3)
    t = rng.integers(-8, 9, size=(300, 2, 3, 3)).astype(np.float32)
    near = P.pairwise(t[:, 0], t[:, 1])
    far = P.pairwise(t[:, 0] + np.float32(1e6), t[:, 1] + np.float32(1e6))
    assert np.array_equal(near[1], far[1]) and len(set(near[1].tolist())) > 8
    assert np.array_equal(P.bits(near[0][near[1] == 0]), P.bits(far[0][near[1] == 0])) and (near[1] == 0).sum() > 10       # pierced: +0.0
    assert np.abs(np.sqrt(near[0]) - np.sqrt(far[0])).max() < 1e-8
    e = far[2] - far[3]
    assert np.array_equal(X.dot(e, e), far[0])


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------
def test_two_lattice_cubes_a_gap_of_three_apart():
    va, fa, vb, fb, side_a, side_b = P.two_cubes(3.0)
    assert len(side_a) == len(side_b) == 8
    for band in (np.inf, 3.0):
        r = P.mesh_distance(va, fa, vb, fb, band)
        assert (r['distance'][side_a] == 3.0).all() and np.isin(r['partner'][side_a], side_b).all()
    # in the band at 3.0: the facing side and the sixteen faces of the four sides around it that reach its plane with an edge or a corner
    touching = (va[fa][:, :, 0] == 4).any(1)
    assert touching.sum() == 24 and np.array_equal(r['in_band'], touching) and (r['distance'][touching] == 3.0).all()
    assert r['n_in_band'] == 24 and (r['partner'] == -1).sum() == len(fa) - 24
    below = P.mesh_distance(va, fa, vb, fb, np.nextafter(3.0, 0.0))
    assert below['n_in_band'] == 0 and np.isinf(below['distance']).all() and (below['kind'] == -1).all() and np.isnan(below['closest_a']).all()
    back = P.mesh_distance(vb, fb, va, fa, 3.0)
    assert (back['distance'][side_b] == 3.0).all() and back['n_in_band'] == 24


def test_crossing_spheres_are_at_zero_where_the_intersection_restatement_finds_crossings():
    va, fa, vb, fb = P.crossing_spheres()
    r = P.mesh_distance(va, fa, vb, fb)
    merged = X.self_intersections(np.concatenate([va, vb]), np.concatenate([fa, fb + len(va)]))
    cross = merged['pairs'][(merged['pairs'][:, 0] < len(fa)) & (merged['pairs'][:, 1] >= len(fa))]
    assert len(cross) > 40 and merged['n_pairs'] == len(cross)                               # (neither sphere crosses itself)
    assert np.array_equal(np.flatnonzero((r['d2'] == 0) & (r['kind'] == 0)), np.unique(cross[:, 0]))
    assert not ((r['d2'] == 0) & (r['kind'] != 0)).any()
    back = P.mesh_distance(vb, fb, va, fa)
    assert np.array_equal(np.flatnonzero(back['kind'] == 0), np.unique(cross[:, 1]) - len(fa))
    # the smallest partner of a crossed face is the smallest face it crosses
    first = {int(f): int(cross[cross[:, 0] == f, 1].min()) - len(fa) for f in np.unique(cross[:, 0])}
    assert all(r['partner'][f] == g for f, g in first.items())


def sagitta(v, f, centre):
    """the most a face lies inside the sphere its corners lie on: the largest corner radius minus the smallest plane distance"""
    t = np.asarray(v, np.float64)[f] - centre
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    h = np.abs((n * t[:, 0]).sum(1)) / np.sqrt((n * n).sum(1))
    return float(np.sqrt((t * t).sum(2)).max() - h.min())


def test_contact_area_of_two_spheres_lies_in_the_bracket_of_two_caps():
    """Spheres S_A, S_B of radius R, centres L apart; the meshes are inscribed: every point of mesh A lies within [R - s, R] of c_A (s its
    sagitta), the same for B, and the radial projection pi of a mesh onto its sphere is onto and moves no point by more than s.
    For a point x outside S_B write g(x) = |x - c_B| - R, its distance from S_B.  A point of S_A at angle theta from the axis has
    |x - c_B|^2 = R^2 + L^2 - 2 R L cos theta, so g(x) <= D' on the cap (R + D')^2 >= R^2 + L^2 - 2 R L cos theta, of area
    cap(D') = 2 pi R^2 (1 - cos theta(D')).
      Distances.  For y on mesh A: g(y) <= dist(y, mesh B) <= g(y) + s_B (mesh B lies inside S_B, and the point of S_B nearest to y is
      the projection of a point of mesh B at most s_B away), and |g(y) - g(pi y)| <= s_A.
      Above.  A face f in contact has a point y with dist(y, mesh B) <= D, so g(y) <= D; every point z of f is within the longest
      edge e of y, so g(pi z) <= g(z) + s_A <= D + e + s_A: pi(f) lies in cap(D + e + s_A).  Projecting a planar face outwards onto the
      sphere never shrinks its area, and the projections of distinct faces do not overlap, so area_a <= cap(D + e + s_A).
      With delta = s_A + s_B >= s_A that is inside the upper side asked for, cap(D + e + delta).
      Below.  A point x of S_A with g(x) <= D - s_A - s_B is pi(y) for a y of some face f with dist(y, mesh B) <= g(x) + s_A + s_B <= D,
      so f is in contact: cap(D - delta) is covered by the projections of the in-contact faces.  The bracket asked for is
      cap(D - delta) <= area_a <= cap(D + e + delta), and it is asserted as it stands.  Its lower side compares a planar area with a
      spherical one, so by itself the covering does not prove it: an element of a face at plane distance h and radius r from c_A has
      dA_plane = dA_sphere r^3 / (R^2 h) >= (h / R)^2 dA_sphere (the projection scales lengths by R / r, and the tilt enlarges the
      planar element).  What the covering proves is area_a >= ((R - s_A) / R)^2 cap(D - delta), which is asserted as well; the plain
      lower side holds because the in-contact faces are whole faces that reach past the cap."""
    R, L, D = 50.0, 110.0, 30.0
    va, fa, vb, fb = P.two_spheres(R, L)
    c_b = np.asarray(vb, np.float64).mean(0)
    s_a, s_b = sagitta(va, fa, np.zeros(3)), sagitta(vb, fb, c_b)
    assert 0 < s_a < 0.06 * R and abs(s_a - s_b) < 1e-3
    e = longest_edge(np.asarray(va)[fa])

    def cap(dist):
        cos_t = (R * R + L * L - (R + dist) ** 2) / (2.0 * R * L)
        return 2.0 * np.pi * R * R * (1.0 - min(max(cos_t, -1.0), 1.0))
    side = P.contact_side(va, fa, vb, fb, D)
    delta = s_a + s_b
    lower, upper = cap(D - delta), cap(D + e + delta)
    print('area_a %.1f in [%.1f, %.1f]; the sphere\'s own cap %.1f' % (side['area'], lower, upper, cap(D)))
    assert lower <= side['area'] <= upper
    assert ((R - s_a) / R) ** 2 * lower <= side['area'] <= cap(D + e + s_a)                 # what the derivation proves by itself
    assert len(side['patch_area']) == 1 and side['patch_faces'][0] == side['faces'].sum() and side['n_crossing'] == 0
    assert side['patch_area'][0] == pytest.approx(side['area'], rel=1e-12)
    assert (L - 2 * R) <= side['patch_min_distance'][0] <= (L - 2 * R) + s_a + s_b           # the gap on the axis, within the sagittas


# ---- mutations --------------------------------------------------------------------------------------------------------------------------
def test_each_mutation_turns_an_assertion_red():
    ta, tb, want, kinds = P.CLOSED_FORMS['crossed_edges']
    assert P.tri_tri(ta, tb, 'no_edge_edge')[0] == 8.0 != want                               # the corner answer
    ta, tb, want, kinds = P.CLOSED_FORMS['parallel_3_apart']
    d2, kind, _, _ = P.tri_tri(ta, tb, 'ge')
    assert d2 == want and kind not in kinds                                                  # the last of the equal candidates
    ta, tb, want, kinds = P.CLOSED_FORMS['pierced']
    d2, kind, _, _ = P.tri_tri(ta, tb, 'no_pierce')
    assert d2 > 0 and kind != 0
    va, fa, vb, fb = P.crossing_spheres()
    assert P.mesh_distance(va, fa, vb, fb, mutate='no_pierce')['n_zero'] == 0 < P.mesh_distance(va, fa, vb, fb)['n_zero']
    assert set(P.MUTATIONS) == {'no_edge_edge', 'ge', 'no_pierce'}
