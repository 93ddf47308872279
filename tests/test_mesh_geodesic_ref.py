"""
CPU test: the NumPy restatement of the geodesic graph distance (tests/mesh_geodesic_ref.py) against ground truth -- closed forms on a
strip and on flat tilings, the chord and the arc on a sphere, scipy's Dijkstra on the same arcs -- and against three one-line mutations
of the definition.  The GPU tests then ask the device for this restatement's bits.
"""
import numpy as np

import mesh_geodesic_ref as R
from ch_shrinkwrap_amd.trimesh import geodesic_sphere

bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)

# The method's stated overestimate: D / (R angle) from vertex 0 of geodesic_sphere(12, 100.0), as the restatement gives it on a CPU.
# The values are deterministic (IEEE float64, correctly rounded sqrt); the margin of the test allows for nothing in particular.
SPHERE = dict(n=12, R=100.0, max_diag=1.0415, mean_diag=1.0148, max_edges=1.2167, mean_edges=1.0824)


def test_strip_of_unit_squares():
    """along the strip D is the exact sum of the edge lengths; across one square D is sqrt(2) with diagonals and 2 without, where the
    mesh's own diagonal runs the other way"""
    V, F = R.grid_mesh(9, 2)                                  # own diagonals (i, 0) -> (i+1, 1)
    r = R.geodesic(V, F, [0])
    assert (r['distance'][:9] == np.arange(9.0)).all()
    assert r['distance'][9 + 1] == np.sqrt(2.0)               # (1, 1): the mesh's own diagonal
    for diag, want in ((True, np.sqrt(2.0)), (False, 2.0)):
        r = R.geodesic(V, F, [1], diagonals=diag)             # (1, 0) -> (0, 1): against the mesh's own diagonal
        assert abs(r['distance'][9] - want) <= 4 * np.spacing(want)          # (the unfolding rounds: a few ulps, not the bits of sqrt(2))
        assert (r['source'] == 0).all()
    V, F = R.grid_mesh(9, 2, flip=True)
    assert R.geodesic(V, F, [0], diagonals=False)['distance'][9 + 1] == 2.0
    assert abs(R.geodesic(V, F, [0], diagonals=True)['distance'][9 + 1] - np.sqrt(2.0)) <= 4 * np.spacing(np.sqrt(2.0))


def test_flat_tilings_against_the_euclidean_distance():
    V, F = R.grid_mesh(12, 9, dx=1.0, dy=0.75)
    for diag in (True, False):
        r = R.geodesic(V, F, [40], diagonals=diag, want_labels=False)
        eu = np.linalg.norm(V.astype(np.float64) - V[40].astype(np.float64), axis=1)
        assert (r['distance'] >= eu * (1 - 1e-12)).all()                  # (sums and roots round: a few ulps either way)
    V, F = R.equilateral_mesh(14, 11)
    src = 5 * 14 + 6
    eu = np.linalg.norm(V.astype(np.float64) - V[src].astype(np.float64), axis=1)
    r = R.geodesic(V, F, [src], diagonals=False, want_labels=False)
    far = eu > 0
    assert (r['distance'][far] >= eu[far] * (1 - 1e-6)).all()                 # (float32 positions: the tiling's sides are 1 to 2^-24)
    assert (r['distance'][far] / eu[far]).max() <= 2.0 / np.sqrt(3.0) * (1 + 1e-6)
    assert (r['distance'][far] / eu[far]).max() > 1.15                        # ... and the bound is reached
    rd = R.geodesic(V, F, [src], diagonals=True, want_labels=False)
    assert (rd['distance'] <= r['distance']).all() and (rd['distance'][far] >= eu[far] * (1 - 1e-6)).all()


def _sphere_ratios(diag):
    V, F = geodesic_sphere(SPHERE['n'], SPHERE['R'])
    r = R.geodesic(V, F, [0], diagonals=diag, want_labels=False)
    P = V.astype(np.float64)
    chord = np.linalg.norm(P - P[0], axis=1)
    Rm = np.linalg.norm(P, axis=1)
    angle = np.arccos(np.clip((P @ P[0]) / (Rm * Rm[0]), -1.0, 1.0))
    far = np.arange(V.shape[0]) != 0
    assert (r['distance'] >= chord).all()
    ratio = r['distance'][far] / (SPHERE['R'] * angle[far])
    return float(ratio.max()), float(ratio.mean())


def test_sphere_overestimate_is_the_stated_one():
    """Measured on this restatement: D / (R angle) from one vertex of geodesic_sphere(12, 100) is at most 1.0415 (mean 1.0148) with
    diagonals and at most 1.2167 (mean 1.0824) on the edges alone.  These are the numbers the README and geodesic.py state."""
    mx_d, mean_d = _sphere_ratios(True)
    mx_e, mean_e = _sphere_ratios(False)
    print('sphere: diagonals max %.4f mean %.4f; edges max %.4f mean %.4f' % (mx_d, mean_d, mx_e, mean_e))
    assert mx_d < mx_e and mean_d < mean_e
    assert mx_d <= SPHERE['max_diag'] + 0.01 and mean_d <= SPHERE['mean_diag'] + 0.01
    assert mx_e <= SPHERE['max_edges'] + 0.01 and mean_e <= SPHERE['mean_edges'] + 0.01
    assert mx_d >= SPHERE['max_diag'] - 0.01 and mean_d >= SPHERE['mean_diag'] - 0.01       # the statement is not stale
    import re
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in ('README.md', os.path.join('ch_shrinkwrap_amd', 'geodesic.py')):
        txt = re.sub(r'\s+', ' ', open(os.path.join(root, path)).read())
        for key in ('max_diag', 'mean_diag', 'max_edges', 'mean_edges'):
            assert '%.4f' % SPHERE[key] in txt, (path, key)


def test_scipy_dijkstra_on_the_same_arcs():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    V, F = geodesic_sphere(5, 30.0)
    rng = np.random.default_rng(3)
    V = (V + rng.normal(scale=0.4, size=V.shape)).astype(np.float32)
    ids = np.array([7, 100, 33])
    r = R.geodesic(V, F, ids, want_labels=False)
    tail, head, w = r['arcs']
    # (coo sums duplicates: keep one arc per (tail, head); they carry one weight)
    key, first = np.unique(tail * V.shape[0] + head, return_index=True)
    G = coo_matrix((w[first], (tail[first], head[first])), shape=(V.shape[0],) * 2).tocsr()
    want = dijkstra(G, directed=True, indices=ids).min(0)
    assert np.allclose(r['distance'], want, rtol=1e-12, atol=0)


def _perturbed_sphere(seed=1):
    V, F = geodesic_sphere(4, 20.0)
    rng = np.random.default_rng(seed)
    return (V + rng.normal(scale=0.5, size=V.shape)).astype(np.float32), F


def test_face_order_and_corner_rotation_change_no_bit():
    V, F = _perturbed_sphere()
    ids, d0 = np.array([3, 90, 41, 3]), np.array([0.0, 2.5, 1.0, 0.5])
    a = R.geodesic(V, F, ids, d0)
    rng = np.random.default_rng(5)
    G = F[rng.permutation(F.shape[0])]
    G = np.stack([np.roll(f, k) for f, k in zip(G, rng.integers(0, 3, G.shape[0]))])
    b = R.geodesic(V, G, ids, d0)
    assert (bits(a['distance']) == bits(b['distance'])).all() and (a['source'] == b['source']).all()


def test_vertex_renumbering():
    V, F = _perturbed_sphere(2)
    perm = np.random.default_rng(6).permutation(V.shape[0])          # new id of old vertex i
    V2 = np.empty_like(V)
    V2[perm] = V
    F2 = perm[F].astype(np.int32)
    for diag in (False, True):
        a = R.geodesic(V, F, [11], diagonals=diag, want_labels=False)['distance']
        b = R.geodesic(V2, F2, [perm[11]], diagonals=diag, want_labels=False)['distance'][perm]
        if diag:                                                     # the canonical end of an edge is the smaller id: it may change
            assert np.allclose(a, b, rtol=1e-12, atol=0)
        else:
            assert (bits(a) == bits(b)).all()


def test_a_cap_changes_no_value_at_or_below_it():
    V, F = _perturbed_sphere(3)
    full = R.geodesic(V, F, [0, 50])
    d = np.sort(full['distance'])
    for cap in (d[40], np.nextafter(d[40], 0.0), d[-1], 1e-300):
        r = R.geodesic(V, F, [0, 50], max_distance=cap)
        keep = full['distance'] <= cap
        assert (bits(r['distance'][keep]) == bits(full['distance'][keep])).all() and np.isinf(r['distance'][~keep]).all()
        assert (r['source'][keep] == full['source'][keep]).all() and (r['source'][~keep] == -1).all()


def test_a_dominated_source_takes_the_other_label():
    V, F = R.grid_mesh(6, 2)
    r = R.geodesic(V, F, [0, 3], [0.0, 10.0])                 # vertex 3 is 3 from vertex 0: its own start value never counts
    assert r['distance'][3] == 3.0 and (r['source'] == 0).all()
    r = R.geodesic(V, F, [0, 3], [0.0, 3.0])                  # a tie: both are tight at vertex 3, the smaller index wins
    assert r['source'][3] == 0
    r = R.geodesic(V, F, [3, 0], [3.0, 0.0])
    assert r['source'][3] == 0 and r['source'][0] == 1 and r['source'][5] == 0
    r = R.geodesic(V, F, [0, 3], [0.0, 2.0])
    assert r['source'][3] == 1 and r['source'][4] == 1 and r['source'][0] == 0


def _hinge(xc, yc, xd, yd, L=1.0):
    """two faces about the edge a = 0 -> b = 1 along x: c above, d below, in one plane"""
    V = np.array([[0, 0, 0], [L, 0, 0], [xc, yc, 0], [xd, -yd, 0]], np.float32)
    F = np.array([[0, 1, 2], [1, 0, 3]], np.int32)
    return V, F


def test_mutations_are_caught():
    # (1) <= in the crossing test: the segment c -> d runs exactly through the end a of the edge
    V, F = _hinge(-0.5, 0.5, 0.5, 0.5)
    assert R.diagonals(V, F, R.twins(F))[2].size == 0
    assert R.diagonals(V, F, R.twins(F), crossing_inclusive=True)[2].size == 1
    # (2) a flat face keeps its diagonal: c on the edge's line, between its ends
    V, F = _hinge(0.5, 0.0, 0.25, 0.5)
    assert R.diagonals(V, F, R.twins(F))[2].size == 0
    assert R.diagonals(V, F, R.twins(F), keep_flat=True)[2].size == 1
    # (3) the label along an arc that is not tight: source 1 starts late, its label must not leave its vertex's neighbourhood
    V, F = R.grid_mesh(6, 2)
    good = R.geodesic(V, F, [3, 0], [2.0, 0.0])
    bad = R.geodesic(V, F, [3, 0], [2.0, 0.0], any_arc=True)
    assert good['source'][0] == 1 and good['source'][3] == 0
    assert (bad['source'] == 0).all() and (good['source'] != bad['source']).any()
