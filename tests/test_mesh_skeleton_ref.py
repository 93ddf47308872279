"""
CPU test of the restatement itself (tests/mesh_skeleton_ref.py): before the device is asked for its bytes, the definition is tied to
results that are known without it -- a tube is a path whose nodes sit on the axis with the ring's perimeter, a torus has one loop down
to a band width of a tenth of an edge and LOSES it where the band is wider than the hole, two joined tori have two, a sphere is a path
-- to the invariants of the construction, to renumbering, to ties and dead corners, and to one-line mutations that must turn an
assertion red.  The tempting definition on the vertices' bands alone is shown to break a tube apart.
"""
import functools

import numpy as np
import pytest

import mesh_skeleton_ref as R
from ch_shrinkwrap_amd.trimesh import icosphere


@functools.lru_cache(maxsize=None)
def torus():
    V, F = R.torus_mesh()
    D = V[:, 0].astype(np.float64) * np.cos(0.3) + V[:, 1] * np.sin(0.3)          # a rotated x coordinate
    return V, F, D - D.min() + 0.0123


@functools.lru_cache(maxsize=None)
def tube(capped=False):
    V, F = R.tube_mesh(capped=capped)
    return V, F, V[:, 2].astype(np.float64) + 0.011


@functools.lru_cache(maxsize=None)
def double_torus():
    V, F = R.double_torus()
    far = int(np.argmax(R.edge_dijkstra(V, F, 0)))
    return V, F, R.edge_dijkstra(V, F, far), R.mean_edge(V, F)


def is_path(r):
    N, A, C, loops = R.graph_numbers(r)
    deg = np.bincount(R.degrees(r), minlength=3)
    return C == 1 and loops == 0 and A == N - 1 and (N == 1 or (deg[1] == 2 and deg[2] == N - 2 and deg[3:].sum() == 0))


def invariants(r, closed):
    P = r['piece_node'].size
    assert r['piece_start'][-1] == P and r['piece_start'][0] == 0 and (np.diff(r['piece_start']) >= 0).all()
    N = r['node_band'].size
    # every piece lies in one node, every node has a piece, nodes are numbered by their smallest piece
    assert P == 0 or (r['piece_node'].min() == 0 and r['piece_node'].max() == N - 1)
    first = np.full(N, P)
    np.minimum.at(first, r['piece_node'], np.arange(P))
    assert (np.diff(first) > 0).all()
    # a node's pieces share one band
    assert (r['node_band'][r['piece_node']] == r['piece_band']).all()
    # arcs join bands k and k + 1 only, (smaller, larger), sorted, distinct
    a = r['arcs'].astype(np.int64)
    assert (np.abs(r['node_band'][a[:, 0]] - r['node_band'][a[:, 1]]) == 1).all() and (a[:, 0] < a[:, 1]).all()
    key = a[:, 0] * (N + 1) + a[:, 1]
    assert (np.diff(key) > 0).all()
    assert (r['node_sums'][:, R.S_PIECES].astype(np.int64) == np.bincount(r['piece_node'], minlength=N)).all()
    # vertex_node: the node of a piece of the vertex's own band, -1 exactly for the vertices without a live face
    vn = r['vertex_node']
    assert ((vn >= 0) <= (r['band'] >= 0)).all() and (r['node_band'][vn[vn >= 0]] == r['band'][vn >= 0]).all()
    if closed:
        # contours close: every crossing point (an edge and a band) is used by exactly two segments, and both compute the same bits
        cr = np.flatnonzero(r['crossed'])
        keys = np.concatenate([np.concatenate([r['edge_keys'][cr, e], r['piece_band'][cr, None]], 1) for e in (0, 1)])
        pts = np.concatenate([r['points'][cr, 0], r['points'][cr, 1]])
        uniq, inv, count = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
        assert (count == 2).all()
        order = np.argsort(inv.reshape(-1), kind='stable')
        assert pts[order[0::2]].tobytes() == pts[order[1::2]].tobytes()
        # and the two segments at a crossing point belong to one node
        node = np.concatenate([r['piece_node'][cr], r['piece_node'][cr]])
        assert (node[order[0::2]] == node[order[1::2]]).all()


def test_a_tube_is_a_path_on_its_axis_with_the_rings_perimeter():
    V, F, D = tube()
    ring = V[:12].astype(np.float64)
    polygon = float(np.sqrt(((ring - np.roll(ring, -1, 0)) ** 2).sum(1)).sum())   # the float32 ring's own perimeter
    assert abs(polygon - 2 * 12 * np.sin(np.pi / 12)) < 2e-7                       # 2 * 12 sin(pi / 12), to float32 rounding of the corners
    for w in (1.3, 0.5, 0.07):
        r = R.level_sets(V, F, D, w)
        invariants(r, closed=False)
        assert is_path(r), w
        per, cen = R.float_contours(r)
        has = per > 0
        assert has.sum() >= r['node_band'].size - 1
        # in float64, before quantisation: the perimeter to 4e-15, the axis to 1e-16
        assert np.abs(per[has] - polygon).max() <= 4e-15 and np.abs(cen[has][:, :2]).max() <= 1e-16, w
        # and what the integer sums give: within the header's bounds (q / 2 per axis; n (sqrt(3) + 2^-11) q for a perimeter of n segments)
        n = R.nodes(r)
        q = r['q']
        assert np.abs(n['position'][has] - cen[has]).max() <= 0.5 * q
        assert (np.abs(n['perimeter'][has] - per[has]) <= n['n_segments'][has] * (np.sqrt(3) + 2.0 ** -11) * q).all()
        assert np.abs(n['radius'][has] - 1.0).max() < 1e-5 + 0.05                   # (a 12-gon's perimeter is 1.1 % short of the circle's)
        assert q == 2.0 ** -17 and (n['n_segments'][has] == 24).all()
    assert R.level_sets(V, F, D, 0.07)['node_band'].size == 65


def test_a_capped_tubes_end_band_has_no_contour_and_falls_back_to_the_centroids():
    V, F, D = tube(capped=True)
    w = 0.5
    # the bottom cap lies at z = 0, D = 0.011: band 0's level 0.25 is crossed by the wall; shift so that the cap's band holds no level
    D = V[:, 2].astype(np.float64) + 0.3                          # cap at 0.3 (band 0, level 0.25 below it), first wall ring at 0.8
    r = R.level_sets(V, F, D, w)
    invariants(r, closed=True)
    assert is_path(r)
    n = R.nodes(r)
    node0 = np.flatnonzero(r['node_band'] == 0)
    assert node0.size == 1 and n['n_segments'][node0[0]] == 0 and n['perimeter'][node0[0]] == 0.0
    pieces = np.flatnonzero(r['piece_node'] == node0[0])
    cent = V.astype(np.float64)[F[r['piece_face'][pieces]]].mean(1).mean(0)        # the mean of its faces' centroids
    assert np.abs(n['position'][node0[0]] - cent).max() <= 0.5 * r['q'] and np.isfinite(n['position']).all()
    assert n['n_segments'][r['node_band'] == 3][0] == 24


def test_a_torus_has_one_loop_down_to_a_tenth_of_an_edge():
    V, F, D = torus()
    for w in (2.0, 0.7, 0.25, 0.05):
        r = R.level_sets(V, F, D, w)
        invariants(r, closed=True)
        N, A, C, loops = R.graph_numbers(r)
        assert (C, loops) == (1, 1) and A - N + C == 1, w
    assert 0.05 < 0.11 * R.mean_edge(V, F)                        # a tenth of an edge


def test_a_band_wider_than_the_hole_loses_the_loop():
    """the documented limit as a tested fact: a graph-distance field from one vertex, one loop at 0.3, 1 and 2 mean edge lengths, NONE at 4"""
    V, F, _ = torus()
    D, me = R.edge_dijkstra(V, F, 0), R.mean_edge(V, F)
    for m, loops in ((0.3, 1), (1.0, 1), (2.0, 1), (4.0, 0)):
        r = R.level_sets(V, F, D, m * me)
        invariants(r, closed=True)
        assert R.graph_numbers(r)[2:] == (1, loops), m


def test_two_joined_tori_have_two_loops():
    V, F, D, me = double_torus()
    assert V.shape[0] == 1040 and F.shape[0] == 2084
    edges = np.unique(np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), 1), axis=0).shape[0]
    assert V.shape[0] - edges + F.shape[0] == -2                  # genus 2
    for m, loops in ((0.3, 2), (1.0, 2), (2.0, 2), (4.0, 2), (8.0, 1)):
        r = R.level_sets(V, F, D, m * me)
        if m in (0.3, 2.0):
            invariants(r, closed=True)
        assert R.graph_numbers(r)[2:] == (1, loops), m


def test_a_sphere_is_a_path():
    V, F = icosphere(2, 1.0)
    for w in (0.3, 0.05):
        r = R.level_sets(V, F, V[:, 2].astype(np.float64) + 1.0, w)
        invariants(r, closed=True)
        assert is_path(r)


def _canonical(r, V):
    """what does not depend on the numbering: per node (band, sums), sorted, and the arcs as pairs of such rows"""
    rows = [tuple([int(b)] + [int(x) for x in s]) for b, s in zip(r['node_band'], r['node_sums'])]
    arcs = sorted(tuple(sorted((rows[a], rows[b]))) for a, b in r['arcs'].tolist())
    return sorted(rows), arcs


def test_renumbering_faces_corners_and_vertices_changes_nothing():
    V, F, D = torus()
    rng = np.random.default_rng(3)
    base = _canonical(R.level_sets(V, F, D, 0.25), V)
    assert len(set(base[0])) > len(base[0]) // 2                  # the rows tell most nodes apart: the comparison means something
    F2 = F[rng.permutation(F.shape[0])]
    F2 = np.stack([np.roll(f, int(s)) for f, s in zip(F2, rng.integers(0, 3, F2.shape[0]))]).astype(np.int32)
    assert _canonical(R.level_sets(V, F2, D, 0.25), V) == base
    perm = rng.permutation(V.shape[0])                            # vertex i becomes perm[i]
    V3, D3 = np.empty_like(V), np.empty_like(D)
    V3[perm], D3[perm] = V, D
    r3 = R.level_sets(V3, perm[F2].astype(np.int32), D3, 0.25)
    assert _canonical(r3, V3) == base
    invariants(r3, closed=True)


def test_ties_and_dead_corners():
    V, F = R.tube_mesh()
    z = V[:, 2].astype(np.float64)
    r = R.level_sets(V, F, z, 0.5)                                # D exactly on k w on every ring, D = 0 on the first
    invariants(r, closed=False)
    assert is_path(r) and r['band'].tolist() == np.repeat(np.arange(10), 12).tolist()
    assert r['node_band'].size == 10                              # band 9 is the top ring alone: D = 4.5 belongs to band 9, not 8
    assert R.bands(np.array([0.0, -0.0, 0.5, np.nextafter(0.5, 0), np.inf, -1e-300, -np.inf]), 0.5).tolist() == [0, 0, 1, 0, -1, -1, -1]
    for bad in (np.array([np.nan]), np.array([2.0 ** 31])):
        with pytest.raises(ValueError):
            R.bands(bad, 1.0)
    with pytest.raises(ValueError, match='2\\^28'):
        R.level_sets(V, F, z, 2e-7)
    D = z.copy()
    D[z > 3.7] = np.inf
    D[:3] = -1.0
    r = R.level_sets(V, F, D, 0.3)
    invariants(r, closed=False)
    dead_faces = ~np.isfinite(D[F]).all(1) | (D[F] < 0).any(1)
    assert (r['live'] == ~dead_faces).all() and (np.diff(r['piece_start'])[dead_faces] == 0).all()
    assert (r['vertex_node'][:3] == -1).all() and (r['vertex_node'][D == np.inf] == -1).all() and (r['vertex_node'][(D >= 0) & (D < 3.0)] >= 0).all()
    # two components, one of them dead: its faces have no piece and its vertices no node; alive, it is a second path
    V2, F2 = np.concatenate([V, V + np.float32(10.0)]), np.concatenate([F, F + V.shape[0]])
    r = R.level_sets(V2, F2, np.concatenate([z + 0.011, np.full(z.size, np.inf)]), 0.5)
    invariants(r, closed=False)
    assert is_path(r) and (r['vertex_node'][z.size:] == -1).all() and r['piece_start'][-1] == r['piece_start'][F.shape[0]]
    r = R.level_sets(V2, F2, np.concatenate([z + 0.011, z[::-1] * 0.7]), 0.5)
    assert R.graph_numbers(r)[2:] == (2, 0)
    r = R.level_sets(V2, F2, np.full(2 * z.size, np.inf), 0.5)
    assert r['piece_start'][-1] == 0 and r['node_band'].size == 0 and r['arcs'].shape == (0, 2) and (r['vertex_node'] == -1).all()
    with pytest.raises(ValueError, match='non-manifold'):
        R.level_sets(V, np.concatenate([F, F[:1]]), z, 0.5)


def test_the_vertex_bands_alone_break_the_tube():
    """most bands hold no vertex at w = 0.07: the tempting definition gives ten islands and no arc, the right one a path of 65 nodes"""
    V, F, D = tube()
    assert R.vertex_band_graph(F, D, 1.3)[2:] == (1, 0) and R.vertex_band_graph(F, D, 0.5)[2:] == (1, 0)       # at wide bands both agree
    N, A, C, loops = R.vertex_band_graph(F, D, 0.07)
    assert (N, A, C) == (10, 0, 10)
    assert is_path(R.level_sets(V, F, D, 0.07))


def test_three_mutations_turn_an_assertion_red():
    V, F, D = torus()
    # the crossing point taken from the above end: the two faces of an edge still agree with each other (both are wrong in the same
    # way), but not with the definition's bits
    good = R.level_sets(V, F, D, 0.25)
    bad = R.level_sets(V, F, D, 0.25, from_above=True)
    assert good['points'][good['crossed']].tobytes() != bad['points'][bad['crossed']].tobytes()
    cr = np.flatnonzero(good['crossed'])
    t_good = np.abs(good['points'][cr] - bad['points'][cr]).max()
    assert 0 < t_good < 1e-12                                     # a rounding apart, no more: only a bit comparison of the points sees it
    # (the quantum is 2^-16 here, so the integer sums absorb it unless a coordinate sits on a rounding boundary)
    # a half-open band closed on the wrong side: a ring exactly on k w moves to the band below
    Vt, Ft = R.tube_mesh()
    z = Vt[:, 2].astype(np.float64)
    assert R.level_sets(Vt, Ft, z, 0.5)['node_band'].size == 10
    with pytest.raises((AssertionError, ValueError, IndexError)):
        r = R.level_sets(Vt, Ft, z, 0.5, band_closed_above=True)  # D = 0 lands in band -1: dead by mistake
        assert r['node_band'].size == 10 and r['live'].all()
    # an edge's band range taken exclusive: pieces that touch across an edge are not joined, and the tube falls apart
    r = R.level_sets(Vt, Ft, Vt[:, 2].astype(np.float64) + 0.011, 0.07, edge_range_exclusive=True)
    with pytest.raises(AssertionError):
        assert is_path(r)
    assert R.graph_numbers(r)[0] > 65
