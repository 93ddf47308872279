"""
GPU test: the self-intersection check on the device (include/nw_intersections.h, csrc/nw_intersections.hip) against the brute-force
NumPy restatement (tests/mesh_intersections_ref.py, itself tied to closed forms by tests/test_mesh_intersections_ref.py): per-face
counts, the two totals and the sorted pair list, exactly.  The restatement looks at all pairs of faces with no grid and no centroid
filter, so the device's walk is checked as well as its arithmetic.  No input has more than about 700 faces but the longest strip (1 026).
"""
import ctypes

import numpy as np
import pytest

import mesh_intersections_ref as R
from ch_shrinkwrap_amd import intersections as X
from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = X.IntersectionContext()
    yield c
    c.close()


def device(ctx, v, f, **kw):
    r = ctx.set_mesh(v, f).find(**kw)
    return dict(n_pairs=r['n_pairs'], n_crossed_faces=r['n_faces'], count=r['count'], pairs=r['pairs'])


def check(ctx, v, f):
    """with the list and without it, against the restatement; returns the restatement's answer"""
    ref = R.self_intersections(v, f)
    R.same_as_restatement(device(ctx, v, f), ref)
    without = device(ctx, v, f, return_pairs=False)
    assert without['pairs'] is None
    R.same_as_restatement(without, ref)
    return ref


def test_hand_made_cases(ctx):
    assert check(ctx, *R.cube_and_plane())['n_pairs'] == 8
    for name, (B, expected) in R.TWO_TRIANGLES.items():
        for tris in ((R.A_TRI, B), (B, R.A_TRI)):
            assert check(ctx, *R.soup(*tris))['n_pairs'] == expected, name
    for crossing in (True, False):
        for ra in range(3):
            for rb in range(3):
                assert check(ctx, *R.shared_corner(crossing, ra, rb))['n_pairs'] == int(crossing)
    from test_mesh_intersections_ref import TOUCHING_AT_AN_EDGE_MIDPOINT
    assert check(ctx, TOUCHING_AT_AN_EDGE_MIDPOINT, [[0, 1, 2], [3, 4, 5]])['n_pairs'] == 0


def test_spheres(ctx):
    assert check(ctx, *icosphere(2))['n_pairs'] == 0
    assert check(ctx, *R.noisy_sphere(0.05))['n_pairs'] == 0


def test_crumpled_sphere(ctx):
    v, f = R.noisy_sphere(0.3)
    assert check(ctx, v, f)['n_pairs'] == 700
    # reversed face order: the same set of pairs
    nf = len(f)
    rev = device(ctx, v, f[::-1])
    back = np.sort(nf - 1 - rev['pairs'], axis=1)
    assert np.array_equal(back[np.lexsort((back[:, 1], back[:, 0]))], R.self_intersections(v, f)['pairs'])


@pytest.mark.parametrize('radius,centre', [(1.0, 0.0), (100.0, 1e6)])
def test_two_overlapping_spheres(ctx, radius, centre):
    v, f, _ = R.two_spheres(radius, centre)
    assert check(ctx, v, f)['n_pairs'] == 78


def test_flat_faces(ctx):
    v, f, flat = R.with_flat_faces()
    ref = check(ctx, v, f)
    assert ref['n_pairs'] == 78 and (ref['count'][flat] == 0).all()


@pytest.mark.parametrize('m', [1, 2, 63, 64, 65, 255, 256, 257, 513])
def test_strips_around_the_wave_and_the_block(ctx, m):
    v, f, expected = R.strip(m)
    r = device(ctx, v, f)
    assert np.array_equal(r['pairs'], expected) and (r['count'] == 1).all() and r['n_pairs'] == m and r['n_crossed_faces'] == 2 * m
    check(ctx, v, f)


def test_one_oversize_face_makes_every_lane_walk_the_whole_grid(ctx):
    v, f = R.sphere_and_oversize_face()
    d = np.asarray(v, np.float64)
    assert np.ptp(d[f[-1]], axis=0).max() >= 3 * np.ptp(d[:-3], axis=0).max()
    ref = check(ctx, v, f)
    assert ref['n_pairs'] > 0 and ref['count'][-1] == ref['n_pairs']
    # every lane's box is the whole grid: each reads every other centroid
    r = ctx.set_mesh(v, f).find(stats=True)
    assert r['candidates'] == len(f) * (len(f) - 1) and 0 < r['tested'] < r['candidates']
    R.same_as_restatement(dict(n_pairs=r['n_pairs'], n_crossed_faces=r['n_faces'], count=r['count'], pairs=r['pairs']), ref)


def test_common_centroid_cushion(ctx):
    ref = check(ctx, *R.cushion())                                                        # a grid of almost no extent
    assert ref['n_pairs'] == 190 and (ref['count'] == 19).all()


def test_one_and_two_faces(ctx):
    assert check(ctx, R.A_TRI, [[0, 1, 2]])['n_pairs'] == 0
    assert check(ctx, *R.soup(R.A_TRI, R.TWO_TRIANGLES['pierced'][0]))['pairs'].tolist() == [[0, 1]]


def test_one_context_across_meshes_of_different_sizes(ctx):
    big, small, mid = R.noisy_sphere(0.3), R.soup(R.A_TRI, R.TWO_TRIANGLES['pierced'][0]), R.cube_and_plane()
    own = X.IntersectionContext()
    try:
        for v, f in (small, big, mid, small, big):
            R.same_as_restatement(device(own, v, f), R.self_intersections(v, f))
        # a failed set_mesh leaves the context without a mesh
        bad = np.array(big[0], np.float32)
        bad[5, 1] = np.nan
        with pytest.raises(RuntimeError):
            own.set_mesh(bad, big[1])
        n = ctypes.c_int64()
        assert own.L.nwx_find(own.h, 0, None, ctypes.byref(n), ctypes.byref(n)) == X.NWX_ERR_NOMESH
    finally:
        own.close()


def test_a_second_run_gives_identical_arrays(ctx):
    v, f = R.noisy_sphere(0.3)
    a, b = device(ctx, v, f), device(ctx, v, f)
    assert a['n_pairs'] == b['n_pairs'] == 700 and np.array_equal(a['count'], b['count']) and np.array_equal(a['pairs'], b['pairs'])


def test_get_pairs_refuses_a_short_buffer_and_writes_nothing(ctx):
    v, f, _ = R.two_spheres()
    r = ctx.set_mesh(v, f).find()
    assert r['n_pairs'] == 78
    out = np.full((78, 2), -7, np.int32)
    p = out.ctypes.data_as(ctypes.c_void_p)
    assert ctx.L.nwx_get_pairs(ctx.h, p, 77) == X.NWX_ERR_BADARG and (out == -7).all()
    assert ctx.L.nwx_get_pairs(ctx.h, p, 78) == X.NWX_OK and np.array_equal(out, r['pairs'])
    # no list without NWX_PAIRS
    ctx.find(return_pairs=False)
    out[:] = -7
    assert ctx.L.nwx_get_pairs(ctx.h, p, 78) == X.NWX_ERR_NOPAIRS and (out == -7).all()


# ---- through Python ---------------------------------------------------------------------------------------------------------------------------
def torus(n=24, m=12, R0=3.0, r0=1.0):
    u, w = np.meshgrid(2 * np.pi * np.arange(n) / n, 2 * np.pi * np.arange(m) / m, indexing='ij')
    v = np.stack([(R0 + r0 * np.cos(w)) * np.cos(u), (R0 + r0 * np.cos(w)) * np.sin(u), r0 * np.sin(w)], axis=-1).reshape(-1, 3)
    idx = lambda i, j: (i % n) * m + (j % m)
    f = [t for i in range(n) for j in range(m) for t in ([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])]
    return v.astype(np.float32), np.array(f, np.int32)


def test_trimesh_method_and_mesh_properties():
    from ch_shrinkwrap_amd import evaluation
    v, f, _ = R.two_spheres()
    ref = R.self_intersections(v, f)
    r = TriMesh(v, f).self_intersections()
    R.same_as_restatement(dict(n_pairs=r['n_pairs'], n_crossed_faces=r['n_faces'], count=r['count'], pairs=r['pairs']), ref)
    q = evaluation.mesh_properties(TriMesh(v, f), self_intersections=True)
    assert q['self_intersections'] == 78 and q['self_intersecting_faces'] == 78 and q['manifold'] and q['genus'] == 0 and q['components'] == 2
    plain = evaluation.mesh_properties(TriMesh(v, f))
    assert sorted(plain) == ['area', 'components', 'euler', 'genus', 'manifold', 'volume']
    assert all(q[k] == plain[k] for k in plain)
    v, f = torus()
    q = evaluation.mesh_properties(TriMesh(v, f), self_intersections=True)
    assert q['self_intersections'] == 0 and q['self_intersecting_faces'] == 0 and q['manifold'] and q['genus'] == 1
    assert R.self_intersections(v, f)['n_pairs'] == 0


def test_mesh_properties_module_columns():
    from ch_shrinkwrap_amd import evaluation
    v, f, _ = R.two_spheres()
    ns = {'membrane': TriMesh(v, f)}
    assert list(evaluation.MeshProperties().execute(ns)) == ['euler', 'genus', 'manifold', 'components', 'area', 'volume']
    t = evaluation.MeshProperties(self_intersections=True).execute(ns)
    assert list(t) == ['euler', 'genus', 'manifold', 'components', 'area', 'volume', 'self_intersections', 'self_intersecting_faces']
    assert t['self_intersections'].tolist() == [78] and t['self_intersecting_faces'].tolist() == [78]


def test_the_check_only_observes_a_fit():
    from ch_shrinkwrap_amd import membrane_mesh as mm, synth
    v, f = icosphere(3, 120.0)
    pts = synth.sphere_cloud(2000, 100.0, 10.0, seed=5)
    sigma = np.full(pts.shape, 10.0, 'f4')
    fits = []
    for check_ in (None, 'device'):
        m = mm.MembraneMesh(v, f, kc=1.0, step_size=20.0, max_iter=10, remesh_frequency=5, delaunay_remesh_frequency=0, remesher='device',
                            intersection_check=check_)
        m.shrink_wrap(pts, sigma, minimum_edge_length=25.0)         # (edges grow from 19 to 25 nm: the fitted mesh stays small enough for the restatement)
        fits.append(m)
    plain, watched = fits
    assert len(plain.block_log) == 2 and len(watched.block_log) == 2                       # two remeshed blocks
    assert np.array_equal(np.asarray(plain.faces), np.asarray(watched.faces))
    assert np.array_equal(np.asarray(plain.vertices).view(np.uint32), np.asarray(watched.vertices).view(np.uint32))
    assert plain.intersection_log == []
    assert [e['iteration'] for e in watched.intersection_log] == [5, 10, 10]               # one entry per boundary plus the end
    assert all(sorted(e) == ['iteration', 'n_faces', 'n_pairs'] for e in watched.intersection_log)
    last = watched.intersection_log[-1]
    assert 100 < len(watched.faces) <= 1500 and not np.array_equal(np.asarray(watched.faces), f)
    ref = R.self_intersections(np.asarray(watched.vertices), np.asarray(watched.faces))
    assert last['n_pairs'] == ref['n_pairs'] and last['n_faces'] == ref['n_crossed_faces']
    with pytest.raises(ValueError):
        mm.MembraneMesh(v, f, intersection_check='host')
    with pytest.raises(ValueError):
        mm.ShrinkwrapMembrane(intersection_check='host')
    assert mm.ShrinkwrapMembrane(intersection_check='device').intersection_check == 'device'
