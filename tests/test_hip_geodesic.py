"""The geodesic graph distance on the device (csrc/nw_geodesic.hip) against the NumPy restatement (tests/mesh_geodesic_ref.py), bit for bit in
`distance` and `source`: on one and two triangles, on strips whose vertex and half-edge counts lie around the wave and the workgroup, on a
strip 2 048 arcs long (many times a batch of rounds), on an integer lattice full of ties, on duplicate positions and flat faces, on a half
sphere and on two spheres of which one has no source, with one source, every vertex, duplicates and a dominated source, with the cap at a
vertex's distance and one ulp below, on a non-manifold face array, from a device pointer, through one context across meshes, twice, and
from contact_sites to the field end to end.  The info words that depend on scheduling are compared with nothing."""
import functools

import numpy as np
import pytest

import mesh_geodesic_ref as R
from ch_shrinkwrap_amd import geodesic as G
from ch_shrinkwrap_amd.trimesh import geodesic_sphere, TriMesh

pytestmark = pytest.mark.gpu

bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
# vertices of a strip: half-edges = 3 (V - 2), so 23 -> 63, 24 -> 66, 87 -> 255, 88 -> 258
STRIPS = [3, 4, 23, 24, 63, 64, 65, 87, 88, 255, 256, 257, 4097]


@pytest.fixture(scope='module')
def ctx():
    c = G.GeodesicContext()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def strip(n):
    """a zig-zag strip of n vertices and n - 2 faces, consistently oriented, jittered out of its plane"""
    i = np.arange(n)
    rng = np.random.default_rng(n)
    V = np.stack([0.5 * i, 0.8 * (i % 2), np.zeros(n)], 1) + rng.normal(scale=0.1, size=(n, 3))
    k = np.arange(n - 2)
    F = np.where((k % 2 == 0)[:, None], np.stack([k, k + 1, k + 2], 1), np.stack([k + 1, k, k + 2], 1))
    return V.astype(np.float32), F.astype(np.int32)


@functools.lru_cache(maxsize=None)
def sphere(seed=1, n=4, radius=20.0):
    V, F = geodesic_sphere(n, radius)
    return (V + np.random.default_rng(seed).normal(scale=0.5, size=V.shape)).astype(np.float32), F


def same(got, ref, V, F, diagonals, cap=np.inf):
    assert got['distance'].dtype == np.float64 and got['distance'].shape == (V.shape[0],)
    assert (bits(got['distance']) == bits(ref['distance'])).all()
    if got['source'] is not None:
        assert got['source'].dtype == np.int32 and (got['source'] == ref['source']).all()
    info = got['info']
    assert info['halfedges'] == 3 * F.shape[0]
    assert info['diagonals'] == (R.diagonals(V, F, R.twins(F))[2].size if diagonals else 0)
    assert info['reached'] == int(np.isfinite(ref['D']).sum()) and info['in_band'] == int(np.isfinite(ref['distance']).sum())
    assert 1 <= info['rounds'] <= V.shape[0] + info['batch'] and info['label_rounds'] <= V.shape[0] + info['batch'] and info['batch'] == G.BATCH


def check(V, F, sources, d0=None, cap=np.inf, diagonals=True, labels=True, context=None):
    ref = R.geodesic(V, F, sources, d0, max_distance=cap, diagonals=diagonals)
    got = G.geodesic_distance((V, F), sources, d0=d0, max_distance=cap, diagonals=diagonals, labels=labels, context=context)
    same(got, ref, V, F, diagonals, cap)
    return got, ref


def test_one_and_two_triangles(ctx):
    V = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0]], np.float32)
    got, _ = check(V, np.array([[0, 1, 2]], np.int32), [0], context=ctx)
    assert got['distance'].tolist() == [0.0, 2.0, 1.0] and got['info']['diagonals'] == 0
    # two triangles about the edge 0 -> 1: the corners 2 and 3 see each other across it, or do not (the segment misses the edge)
    F = np.array([[0, 1, 2], [1, 0, 3]], np.int32)
    for d, n_diag in (([0.5, -1, 0.5], 1), ([3.0, -1, 0.0], 0)):
        V = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], d], np.float32)
        got, ref = check(V, F, [2], context=ctx)
        assert got['info']['diagonals'] == n_diag
        edges_only, _ = check(V, F, [2], diagonals=False, context=ctx)
        assert (got['distance'][3] < edges_only['distance'][3]) == bool(n_diag)


@pytest.mark.parametrize('n', STRIPS)
def test_sizes_around_the_wave_and_the_workgroup(ctx, n):
    V, F = strip(n)
    check(V, F, [0, n - 1, n // 2], [0.0, 0.5, 0.25], context=ctx)
    check(V, F, [n // 3], diagonals=False, labels=(n % 2 == 0), context=ctx)


def test_a_strip_many_batches_long(ctx):
    V, F = R.grid_mesh(2049, 2)
    got, ref = check(V, F, [0], context=ctx)
    assert ref['bf_rounds'] >= 2048                           # the shortest walks have about 2 048 arcs
    assert got['distance'][2048] == 2048.0 and got['info']['rounds'] <= V.shape[0] + G.BATCH
    assert got['info']['rounds'] > G.BATCH                    # more than one read of the changed words


def test_an_integer_lattice_of_ties(ctx):
    V, F = R.grid_mesh(17, 17)
    ids = [0, 16, 17 * 16, 17 * 17 - 1, 17 * 8 + 8]
    got, ref = check(V, F, ids, diagonals=False, context=ctx)
    each = np.stack([R.geodesic(V, F, [s], diagonals=False, want_labels=False)['D'] for s in ids])
    tied = int(((each == each.min(0)).sum(0) > 1).sum())
    print('vertices with more than one nearest source:', tied)
    assert tied >= 10                                         # many vertices have several nearest sources: the smallest index wins
    check(V, F, ids, context=ctx)
    check(V, F, ids[::-1], context=ctx)


def test_duplicate_positions_and_flat_faces(ctx):
    V, F = (a.copy() for a in sphere(3))
    V[F[::7, 1]] = V[F[::7, 0]]
    check(V, F, [0, 33], context=ctx)
    V, F = R.grid_mesh(9, 9)
    V[:, 1] = 0.0
    check(V, F, [4], context=ctx)
    V[:] = V[0]
    got, _ = check(V, F, [3, 1], context=ctx)
    assert (got['distance'] == 0).all() and (got['source'] == 0).all()


def test_a_half_sphere_has_border_edges(ctx):
    V, F = sphere(4)
    half = F[V[F].mean(1)[:, 2] > 0]
    assert (R.twins(half) < 0).sum() > 10
    got, ref = check(V, half, [int(half[0, 0])], context=ctx)
    assert np.isinf(got['distance']).any()                    # the vertices of the other half are in no face


def test_two_spheres_and_sources_on_one(ctx):
    V, F = sphere(5)
    V2 = np.concatenate([V, V + np.float32(100.0)])
    F2 = np.concatenate([F, F + V.shape[0]]).astype(np.int32)
    got, _ = check(V2, F2, [3, 40], context=ctx)
    n = V.shape[0]
    assert np.isfinite(got['distance'][:n]).all() and np.isinf(got['distance'][n:]).all() and (got['source'][n:] == -1).all()
    assert got['info']['reached'] == n


def test_sources(ctx):
    V, F = sphere(6)
    n = V.shape[0]
    check(V, F, [17], context=ctx)
    got, _ = check(V, F, np.arange(n), context=ctx)
    assert (got['distance'] == 0).all() and (got['source'] == np.arange(n)).all()
    mask = np.zeros(n, bool)
    mask[[4, 9, 100]] = True
    got, _ = check(V, F, mask, context=ctx)
    assert set(got['source'].tolist()) == {0, 1, 2}
    got, _ = check(V, F, [5, 5, 80, 5], [3.0, 1.0, 0.0, 2.0], context=ctx)      # duplicates with different start values
    assert got['distance'][5] == 1.0 and got['source'][5] == 1
    row = F[(F == 5).any(1)][0]
    near = int(row[row != 5][0])                               # a neighbour of vertex 5 that starts too late: dominated
    got, ref = check(V, F, [5, near], [0.0, 1.0e3], context=ctx)
    assert (got['source'] == 0).all() and got['distance'][near] < 1.0e3
    got, _ = check(V, F, [5], [-0.0], context=ctx)
    assert bits(got['distance'][5:6])[0] == 0


def test_the_cap_at_a_distance_and_one_ulp_below(ctx):
    V, F = sphere(7)
    full = R.geodesic(V, F, [0, 50])
    d = np.sort(full['distance'])[60]
    got, _ = check(V, F, [0, 50], cap=d, context=ctx)
    assert (got['distance'] == d).any()
    below, _ = check(V, F, [0, 50], cap=np.nextafter(d, 0.0), context=ctx)
    assert not (below['distance'] == d).any() and below['info']['in_band'] < got['info']['in_band']
    keep = full['distance'] <= d
    assert (bits(got['distance'][keep]) == bits(full['distance'][keep])).all() and np.isinf(got['distance'][~keep]).all()


def test_a_non_manifold_edge(ctx):
    V = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0], [0.5, 0, 1]], np.float32)
    F = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)          # three faces on the edge 0 - 1
    check(V, F, [2], diagonals=False, context=ctx)
    with pytest.raises((RuntimeError, ValueError)):
        G.geodesic_distance((V, F), [2], diagonals=True, context=ctx)
    with pytest.raises(RuntimeError):                                   # a twin table that is not mutual is refused by the library too
        ctx.set_mesh(V, F, np.array([3, -1, -1, 0, -1, -1, 3, -1, -1], np.int32))
    with pytest.raises(RuntimeError):                                   # ... and it left no mesh behind
        ctx.distances([0])


def test_positions_by_device_pointer(ctx):
    import torch
    V, F = sphere(8)
    dev = torch.from_numpy(V).to('cuda')
    torch.cuda.synchronize()
    ref = R.geodesic(V, F, [1, 2])
    got = ctx.set_mesh((dev.data_ptr(), V.shape[0]), F, R.twins(F)).distances([1, 2], labels=True)
    same(got, ref, V, F, True)
    bad = V.copy()
    bad[7, 1] = np.nan
    dev = torch.from_numpy(bad).to('cuda')
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='non-finite'):
        ctx.set_mesh((dev.data_ptr(), V.shape[0]), F, None)
    with pytest.raises(RuntimeError, match='non-finite'):
        ctx.set_mesh(bad, F, None)


def test_one_context_across_meshes_and_twice_the_same_bytes(ctx):
    big, small = sphere(9, n=6), strip(24)
    for V, F in (big, small, big):
        a = G.geodesic_distance((V, F), [0, 5], [0.0, 0.5], labels=True, context=ctx)
        b = ctx.distances([0, 5], [0.0, 0.5], labels=True)
        same(a, R.geodesic(V, F, [0, 5], [0.0, 0.5]), V, F, True)
        assert a['distance'].tobytes() == b['distance'].tobytes() and a['source'].tobytes() == b['source'].tobytes()
        for k in set(a['info']) - set(G.NOT_DETERMINISTIC):
            assert a['info'][k] == b['info'][k]
    c = ctx.distances([3], max_distance=4.0)                           # the mesh and its weights stay for other sources and caps
    assert (bits(c['distance']) == bits(R.geodesic(big[0], big[1], [3], max_distance=4.0)['distance'])).all() and c['source'] is None


def test_trimesh_method_and_face_order(ctx):
    V, F = sphere(10)
    ref = R.geodesic(V, F, [2, 30])
    got = TriMesh(V, F).geodesic_distance([2, 30], labels=True)
    same(got, ref, V, F, True)
    rng = np.random.default_rng(0)
    P = F[rng.permutation(F.shape[0])]
    P = np.stack([np.roll(f, k) for f, k in zip(P, rng.integers(0, 3, P.shape[0]))]).astype(np.int32)
    other = G.geodesic_distance((V, P), [2, 30], labels=True, context=ctx)
    assert other['distance'].tobytes() == got['distance'].tobytes() and other['source'].tobytes() == got['source'].tobytes()


def test_from_contact_sites_to_the_field():
    from ch_shrinkwrap_amd.proximity import contact_sites
    Va, F = geodesic_sphere(4, 20.0)
    Vb = (Va + np.array([43.0, 0.0, 0.0], np.float32)).astype(np.float32)      # a gap of 3 between the two spheres
    sites = contact_sites((Va, F), (Vb, F), distance=6.0)
    assert sites['faces_a'].any() and not sites['faces_a'].all()
    ids, patch = G.sources_from_faces(F, sites['patches_a'])
    ids_mask, _ = G.sources_from_faces(F, sites['faces_a'])
    assert np.array_equal(ids, ids_mask) and np.array_equal(ids, np.unique(F[sites['faces_a']])) and (patch == 0).all()
    got = G.geodesic_distance((Va, F), ids, labels=True)
    same(got, R.geodesic(Va, F, ids), Va, F, True)
    assert (got['distance'][F[sites['faces_a']]] == 0).all()                   # every in-band face's vertices are sources
    far = int(np.argmin(Va[:, 0]))
    # along the sphere, not through it: over an angle of about pi - 0.5 the arc is 1.36 chords (mesh edges are chords themselves: a per cent less)
    assert got['distance'][far] > 1.2 * np.linalg.norm(Va[far].astype(np.float64) - Va[ids], axis=1).min()
    out = G.GeodesicDistance(max_distance=30.0).execute({'membrane': TriMesh(Va, F), 'contacts': sites})
    assert sorted(k for k in out if k != 'metadata') == ['geodesic_distance', 'nearest_source', 'x', 'y', 'z']
    cap = R.geodesic(Va, F, ids, max_distance=30.0)
    assert (bits(out['geodesic_distance']) == bits(cap['distance'])).all()
    assert np.array_equal(out['nearest_source'], np.where(cap['source'] >= 0, ids[np.maximum(cap['source'], 0)], -1))
    r_mid, mean, area, n = G.surface_profile(got['distance'], np.ones(Va.shape[0]), np.ones(Va.shape[0]), np.linspace(0.0, 70.0, 8))
    assert n.sum() == Va.shape[0] and np.allclose(mean[n > 0], 1.0) and np.array_equal(area, n)
