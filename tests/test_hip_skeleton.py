"""The level-set skeleton on the device (csrc/nw_skeleton.hip) against the NumPy restatement (tests/mesh_skeleton_ref.py), byte for byte in
piece_start, piece_node, vertex_node, node_band, node_sums and arcs: on strips whose piece counts lie around the wave and the workgroup,
on a strip of 2 048 faces in one band whose hooks form one long chain, on one face spanning 1 000 bands beside faces of span 1, on the
torus at a band width of a tenth of an edge and at two units, on the double torus, on ties, dead corners, two components and border
edges, from a field handed over as a device pointer, twice through one context, with a smaller mesh after a larger one, and end to end
from the default field to the loop count.  The info words that depend on scheduling are compared with nothing."""
import functools

import numpy as np
import pytest

import mesh_skeleton_ref as R
from ch_shrinkwrap_amd import skeleton as S
from ch_shrinkwrap_amd import geodesic as G
from ch_shrinkwrap_amd.trimesh import TriMesh

pytestmark = pytest.mark.gpu

KEYS = ('piece_start', 'piece_node', 'vertex_node', 'node_band', 'node_sums', 'arcs')


@pytest.fixture(scope='module')
def ctx():
    c = S.SkeletonContext()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def torus():
    V, F = R.torus_mesh()
    D = V[:, 0].astype(np.float64) * np.cos(0.3) + V[:, 1] * np.sin(0.3)
    return V, F, D - D.min() + 0.0123


@functools.lru_cache(maxsize=None)
def double_torus():
    V, F = R.double_torus()
    far = int(np.argmax(R.edge_dijkstra(V, F, 0)))
    return V, F, R.edge_dijkstra(V, F, far), R.mean_edge(V, F)


def same(got, ref):
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert got[k].tobytes() == ref[k].tobytes(), k
    assert got['low'].tobytes() == np.asarray(ref['low'], np.float64).tobytes() and got['q'] == ref['q']
    info = got['info']
    assert info['pieces'] == ref['piece_node'].size and info['nodes'] == ref['node_band'].size and info['arcs'] == ref['arcs'].shape[0]
    assert info['live_faces'] == int(ref['live'].sum()) and info['live_vertices'] == int((ref['band'] >= 0).sum())
    assert info['segments'] == int(ref['crossed'].sum()) and info['max_band'] == int(ref['band'].max())
    assert info['arc_keys'] == info['pieces'] - info['live_faces']
    # (hook_retries, atomics and the *_us words depend on scheduling: compared with nothing)


def check(ctx, V, F, D, w, set_mesh=True):
    ref = R.level_sets(V, F, D, w)
    if set_mesh:
        ctx.set_mesh(V, F, R.twins(F))
    got = ctx.level_sets(D, w)
    same(got, ref)
    return got, ref


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_strips_around_the_wave_and_the_workgroup(ctx, n):
    V, F = R.strip_mesh(n)
    got, _ = check(ctx, V, F, np.full(V.shape[0], 0.5), 1.0)      # one band: as many pieces as faces, one node
    assert got['info']['pieces'] == n and got['info']['nodes'] == 1 and got['info']['arcs'] == 0
    got, _ = check(ctx, V, F, V[:, 0].astype(np.float64) * 0.37 + V[:, 1] * 0.11, 0.25, set_mesh=False)
    assert got['info']['pieces'] > n or n < 3


def test_strips_with_exactly_these_piece_counts(ctx):
    """the same counts with more than one band: every face but the last lies in band 0, the last spans what is missing"""
    for P in (63, 64, 65, 255, 256, 257, 1025):
        V, F = R.strip_mesh(40)
        D = np.full(V.shape[0], 0.5)
        D[-1] = (P - 40) + 0.5                                    # the last face spans P - 39 bands
        got, _ = check(ctx, V, F, D, 1.0)
        assert got['info']['pieces'] == P


def test_a_long_chain_of_hooks(ctx):
    V, F = R.strip_mesh(2048)
    got, ref = check(ctx, V, F, np.full(V.shape[0], 3.25), 1.0)
    assert got['info']['nodes'] == 1 and (got['piece_node'] == 0).all() and (got['vertex_node'] == 0).all() and got['node_band'][0] == 3
    assert got['info']['atomics'] >= 2047                         # every union but none is free; how many more is scheduling
    F2 = F[np.random.default_rng(5).permutation(F.shape[0])]     # the same strip with its faces in a random order
    check(ctx, V, F2, np.full(V.shape[0], 3.25), 1.0)
    check(ctx, V, F[::-1].copy(), V[:, 0].astype(np.float64), 100.0)


def test_one_face_spanning_a_thousand_bands(ctx):
    V, F = R.strip_mesh(9)
    D = np.arange(V.shape[0], dtype=np.float64) * 0.5
    D[4] = 1000.3
    got, ref = check(ctx, V, F, D, 1.0)
    span = np.diff(got['piece_start'])
    assert span.max() >= 1000 and span.min() <= 2 and R.graph_numbers(got)[2:] == (1, 0)


@pytest.mark.parametrize('w', [0.05, 2.0])
def test_the_torus(ctx, w):
    V, F, D = torus()
    got, _ = check(ctx, V, F, D, w)
    assert R.graph_numbers(got)[2:] == (1, 1)


def test_the_double_torus(ctx):
    V, F, D, me = double_torus()
    for m, loops in ((0.3, 2), (2.0, 2), (8.0, 1)):
        got, _ = check(ctx, V, F, D, m * me, set_mesh=m == 0.3)
        assert R.graph_numbers(got)[2:] == (1, loops)


def test_ties_dead_corners_two_components_and_borders(ctx):
    V, F = R.tube_mesh(capped=False)                              # border edges at both ends
    z = V[:, 2].astype(np.float64)
    check(ctx, V, F, z, 0.5)                                      # every ring exactly on k w, D = 0 on the first
    check(ctx, V, F, z * 2.0, 1.0, set_mesh=False)
    D = z.copy()
    D[z > 3.7] = np.inf                                           # the top dead
    D[:3] = -1.0                                                  # three corners of the bottom ring below zero
    got, ref = check(ctx, V, F, D, 0.3, set_mesh=False)
    assert (got['vertex_node'][:3] == -1).all() and (got['vertex_node'][D == np.inf] == -1).all() and 0 < ref['live'].sum() < F.shape[0]
    # two components, one of them dead altogether
    V2 = np.concatenate([V, V + np.float32(10.0)])
    F2 = np.concatenate([F, F + V.shape[0]])
    D2 = np.concatenate([z + 0.011, np.full(V.shape[0], np.inf)])
    got, _ = check(ctx, V2, F2, D2, 0.5)
    assert (got['vertex_node'][V.shape[0]:] == -1).all() and (np.diff(got['piece_start'])[F.shape[0]:] == 0).all()
    D2[V.shape[0]:] = z[::-1] * 0.7                               # both alive: two paths
    got, _ = check(ctx, V2, F2, D2, 0.5, set_mesh=False)
    assert R.graph_numbers(got)[2:] == (2, 0)
    got, _ = check(ctx, V2, F2, np.full(V2.shape[0], np.inf), 0.5, set_mesh=False)     # nothing alive: empty tables
    assert got['info']['pieces'] == 0 and got['info']['nodes'] == 0 and got['arcs'].shape == (0, 2)


def test_refusals_with_a_context(ctx):
    V, F, D = torus()
    ctx.set_mesh(V, F, R.twins(F))
    bad = D.copy()
    bad[5] = np.nan
    for field, w, text in ((bad, 1.0, 'nan'), (D * 2.0 ** 31, 1.0, 'band beyond'), (D, 0.0, 'positive'), (D, np.inf, 'positive'), (D, 1.0e-6, '2\\^28')):
        with pytest.raises(RuntimeError, match=text):
            ctx.level_sets(field, w)
    with pytest.raises(RuntimeError, match='band width'):
        ctx.level_sets(D, 1.0e-6)                         # too many pieces: the text names the band width
    with pytest.raises(ValueError):
        ctx.level_sets(D[:-1], 1.0)
    Fbad = np.concatenate([F, F[:1]])                             # a face twice: a non-manifold edge
    with pytest.raises(Exception):
        S.level_set_skeleton((V, Fbad), field=np.concatenate([D]), band_width=1.0)
    tw = R.twins(F).copy()
    tw[4] = -1
    with pytest.raises(RuntimeError, match='mutual'):
        ctx.set_mesh(V, F, tw)
    with pytest.raises(RuntimeError, match='no mesh'):
        ctx.level_sets(D, 1.0)                                    # a failed set_mesh leaves no mesh
    check(ctx, V, F, D, 0.7)                                      # and the context is as good as new


def test_a_field_by_device_pointer_from_the_geodesic_unit(ctx):
    """the field comes from GeodesicContext and is handed over as a device pointer (the geodesic unit returns host arrays and is not
    changed for this: the array is put on the device by torch)"""
    import torch
    V, F, _, me = double_torus()
    g = G.GeodesicContext()
    try:
        D = g.set_mesh(V, F, R.twins(F)).distances([3])['distance']
    finally:
        g.close()
    dev = torch.from_numpy(D).to('cuda')
    posdev = torch.from_numpy(V).to('cuda')
    torch.cuda.synchronize()
    ref = R.level_sets(V, F, D, 1.5 * me)
    got = ctx.set_mesh((posdev.data_ptr(), V.shape[0]), F, R.twins(F)).level_sets((dev.data_ptr(), V.shape[0]), 1.5 * me)
    same(got, ref)
    bad = D.copy()
    bad[11] = np.nan
    dev = torch.from_numpy(bad).to('cuda')
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='nan'):
        ctx.level_sets((dev.data_ptr(), V.shape[0]), 1.5 * me)


def test_twice_on_one_context_and_a_smaller_mesh_after_a_larger(ctx):
    V, F, D, me = double_torus()
    a, _ = check(ctx, V, F, D, 0.5 * me)
    b = ctx.level_sets(D, 0.5 * me, timing=True)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert all(b['info'][n] >= 0 for n in S.NOT_DETERMINISTIC) and b['info']['hook_us'] > 0
    Vs, Fs = R.tube_mesh(5, 3)
    check(ctx, Vs, Fs, Vs[:, 2].astype(np.float64) + 0.011, 0.3)  # a smaller mesh after a larger one
    check(ctx, V, F, D, 3.0 * me)                                 # and back


def test_end_to_end_on_the_double_torus():
    V, F, _, me = double_torus()
    mesh = TriMesh(V, F)
    r = mesh.skeleton()
    assert abs(r['band_width'] - 2.0 * me) < 1e-5 * me            # the default: twice the mean edge length
    same(dict(r, node_band=r['raw']['node_band'], node_sums=r['raw']['node_sums'], low=r['raw']['low'], q=r['raw']['q']),
         R.level_sets(V, F, r['field'], r['band_width']))
    g = S.skeleton_graph(r)
    genus = mesh.genus() if callable(mesh.genus) else mesh.genus
    assert g['n_loops'] == 2 and g['n_components'] == 1 and int(genus) == 2
    assert g['n_loops'] == R.graph_numbers(dict(node_band=r['raw']['node_band'], arcs=r['arcs']))[3]
    n = R.nodes(dict(node_sums=r['raw']['node_sums'], low=r['raw']['low'], q=r['raw']['q']))
    assert np.array_equal(n['position'], r['nodes']['position']) and np.array_equal(n['perimeter'], r['nodes']['perimeter'])
    has = r['nodes']['perimeter'] > 0
    assert 2 * has.sum() >= r['nodes']['band'].size and 0.5 < np.median(r['nodes']['radius'][has]) < 1.5     # tubes of radius 1
    b = S.branch_of_vertex(r, g)
    assert b.shape == (V.shape[0],) and 0 <= b.max() < g['n_branches'] and len(g['junctions']) >= 2
    nodes, branches = S.SkeletonizeMembrane(prune=0.5).execute({'membrane': mesh})
    assert nodes['metadata']['n_loops'] == 2 and branches['length'].size == len(branches['start']) > 0
