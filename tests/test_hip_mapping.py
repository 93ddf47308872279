"""Localizations mapped onto a mesh on the device (csrc/nw_mapping.hip) against the NumPy restatement (tests/surface_mapping_ref.py): the
per-localization record -- face, weights, distance, closest point -- bit for bit and the integer accumulators exactly, the equalities
the compiled core owes it in tests/test_mapping_core_cpu.py: on cloud sizes around the wave and the block, under contention on one
vertex, edge and face, at the band's edge, with 0, 1 and 8 value columns, from host arrays and device pointers, through one context
across meshes and calls, in chunks and shuffled; then against distance_to_mesh, which knows nothing of it, and through surface_density
and SurfaceDensity on a sphere with one hemisphere four times as dense."""
import functools

import numpy as np
import pytest

import mesh_distance_ref as D
import surface_mapping_ref as M
from ch_shrinkwrap_amd import build
from ch_shrinkwrap_amd import mapping as C
from ch_shrinkwrap_amd.distance import distance_to_mesh
from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere

pytestmark = pytest.mark.gpu

W = M.W_ONE


@pytest.fixture(scope='module')
def ctx():
    c = C.MappingContext()
    yield c
    c.close()


def columns(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-900.0, 5000.0, n), rng.integers(0, 2, n).astype(np.float64), np.zeros(n)], 1), np.array([8192.0, 1.0, 1.0])


@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices, faces, cloud, band, values or None, scales or None) by name"""
    if name == 'sphere':                                          # 80 faces; about a third of the cloud in band
        v, f = icosphere(1, 10.0)
        pts = M.sphere_points(1025, 10.0, 7, jitter=1.5)
        return (v, f, pts, 1.0) + columns(len(pts), 4)
    if name == 'vertex':                                          # 5000 localizations beyond corner 7 of the cube: one row of mass
        v, f = D.cube()
        pts = 1.0 + np.random.default_rng(1).uniform(0.0, 0.25, (5000, 3))
        return v, f, pts, 1.0, np.random.default_rng(2).uniform(-3.0, 3.0, (5000, 1)), np.array([4.0])
    if name == 'edge':                                            # 600 over the edge from (-1, 1, 1) to (1, 1, 1)
        v, f = D.cube()
        rng = np.random.default_rng(3)
        pts = np.stack([rng.uniform(-0.9, 0.9, 600), 1.0 + rng.uniform(0.01, 0.3, 600), 1.0 + rng.uniform(0.01, 0.3, 600)], 1)
        return v, f, pts, 1.0, rng.uniform(-3.0, 3.0, (600, 1)), np.array([4.0])
    if name == 'face':                                            # 600 over one face of the top
        v, f = D.cube()
        rng = np.random.default_rng(4)
        xy = rng.uniform(-0.9, 0.9, (600, 2))
        xy = np.where((xy[:, :1] > xy[:, 1:]), xy, xy[:, ::-1])   # x >= y: one of the two triangles of the quad
        return v, f, np.column_stack([xy, 1.0 + rng.uniform(0.01, 0.3, 600)]), 1.0, rng.uniform(-3.0, 3.0, (600, 1)), np.array([4.0])
    if name == 'degenerate':
        v, f = D.degenerate_faces()
        pts = M.cloud_around(v, 300, 8)
        return (v, f, pts, 0.8) + columns(len(pts), 5)
    if name == 'large':                                           # 1280 faces
        v, f = icosphere(3, 100.0)
        pts = M.sphere_points(600, 100.0, 11, jitter=20.0)
        return (v, f, pts, 15.0) + columns(len(pts), 6)
    if name == 'eight':                                           # eight columns: +scale, -scale, zeros, and five of everything
        v, f = icosphere(1, 10.0)
        pts = M.sphere_points(500, 10.0, 12, jitter=1.0)
        rng = np.random.default_rng(13)
        n = len(pts)
        vals = np.stack([np.full(n, 64.0), np.full(n, -64.0), np.zeros(n), rng.normal(size=n), rng.uniform(0, 1e6, n), -rng.uniform(0, 1e-3, n),
                         rng.integers(-5, 6, n).astype(np.float64), np.arange(n, dtype=np.float64)], 1)
        return v, f, pts, 1.0, vals, np.array([64.0, 64.0, 1.0] + [C.column_scale(vals[:, c]) for c in range(3, 8)])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, n=None, band=None):
    v, f, pts, b, vals, scales = case(name)
    n = len(pts) if n is None else n
    return M.map_cloud(pts[:n], v, f, b if band is None else band, None if vals is None else vals[:n], scales)


def check(ctx, name, n=None, band=None, set_mesh=True):
    v, f, pts, b, vals, scales = case(name)
    n = len(pts) if n is None else n
    ref = reference(name, n, band)
    if set_mesh:
        ctx.set_mesh(v, f)
    dev = ctx.map(pts[:n], band=b if band is None else band, values=None if vals is None else vals[:n], scales=scales)
    M.same_as_restatement(dev, ref)
    assert dev['n_in_band'] == ref['n_in_band'] and dev['info']['rings'] >= n and dev['info']['cells'] >= 1 and dev['info']['cell_size'] > 0
    return dev, ref


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 1025])
def test_cloud_sizes_around_the_wave_and_the_block(ctx, n):
    dev, ref = check(ctx, 'sphere', n)
    if n >= 63:
        assert 0 < ref['n_in_band'] < n
    assert int(dev['mass'].sum()) == dev['n_in_band'] * W and int(dev['count'].sum()) == dev['n_in_band']
    assert np.array_equal(ctx.areas(), M.vertex_areas(*case('sphere')[:2]))


def test_five_thousand_on_one_vertex_six_hundred_on_an_edge_and_on_a_face(ctx):
    dev, ref = check(ctx, 'vertex')
    assert ref['n_in_band'] == 5000 and dev['mass'][7] == 5000 * W and np.count_nonzero(dev['mass']) == 1 and dev['count'].max() == 5000
    dev, ref = check(ctx, 'edge', set_mesh=False)
    assert ref['n_in_band'] == 600 and np.flatnonzero(dev['mass']).tolist() == [6, 7] and int(dev['mass'].sum()) == 600 * W
    dev, ref = check(ctx, 'face', set_mesh=False)
    assert ref['n_in_band'] == 600 and np.count_nonzero(dev['count']) == 1 and np.count_nonzero(dev['mass']) == 3


def test_the_band(ctx):
    v, f, pts, b, vals, scales = case('sphere')
    dev, ref = check(ctx, 'sphere', band=1e-4)                    # every localization out of band
    assert dev['n_in_band'] == 0 and (dev['face'] == -1).all() and np.isinf(dev['distance']).all()
    for k in ('mass', 'count', 'sum_hi', 'sum_lo'):
        assert not dev[k].any()
    gap = float(reference('sphere', band=30.0)['distance'].min())
    assert gap > 1e-4
    dev, ref = check(ctx, 'sphere', band=gap, set_mesh=False)     # a band equal to the gap: the nearest localization alone
    assert dev['n_in_band'] == 1 and int(dev['mass'].sum()) == W
    dev, ref = check(ctx, 'sphere', band=float(np.nextafter(gap, 0.0)), set_mesh=False)
    assert dev['n_in_band'] == 0 and not dev['mass'].any()


def test_no_column_one_column_and_eight(ctx):
    v, f, pts, b, vals, scales = case('eight')
    ref = reference('eight')
    ctx.set_mesh(v, f)
    dev = ctx.map(pts, band=b)                                    # C = 0
    assert dev['sum_hi'].shape == (len(v), 0)
    M.same_as_restatement(dev, M.map_cloud(pts, v, f, b))
    dev = ctx.map(pts, band=b, values=vals[:, 3:4], scales=scales[3:4])
    assert np.array_equal(dev['sum_hi'][:, 0], ref['sum_hi'][:, 3]) and np.array_equal(dev['sum_lo'][:, 0], ref['sum_lo'][:, 3])
    dev, ref = check(ctx, 'eight', set_mesh=False)
    total, expect = C.column_sums(dev['sum_hi'], dev['sum_lo']), dev['mass'].astype(object) * C.Q_ONE
    assert (total[:, 0] == expect).all() and (total[:, 1] == -expect).all() and not total[:, 2].any() and expect.any()
    auto = ctx.map(pts, band=b, values=vals)                      # the binding's own scales
    assert auto['scales'].tolist() == [64.0, 64.0, 1.0] + scales[3:].tolist()
    M.same_accumulators(auto, ref)


def test_a_value_beyond_its_scale_is_refused_in_band_only(ctx):
    v, f, pts, b, vals, scales = case('sphere')
    ref = reference('sphere')
    far, near = int(np.flatnonzero(~ref['in_band'])[0]), int(np.flatnonzero(ref['in_band'])[0])
    ctx.set_mesh(v, f)
    bad = vals.copy()
    bad[far, 0] = 1.5 * scales[0]
    bad[far, 1] = np.nan
    M.same_accumulators(ctx.map(pts, band=b, values=bad, scales=scales), ref)
    bad[near, 0] = 1.5 * scales[0]
    with pytest.raises(C.MappingError) as e:
        ctx.map(pts, band=b, values=bad, scales=scales)
    assert e.value.code == C.NWL_ERR_RANGE
    with pytest.raises(C.MappingError) as e:                      # nothing is left to add onto
        ctx.map(pts, band=b, values=vals, scales=scales, accumulate=True)
    assert e.value.code == C.NWL_ERR_BADARG
    bad[near, 0] = np.inf
    with pytest.raises(C.MappingError) as e:
        ctx.map(pts, band=b, values=bad, scales=scales)
    assert e.value.code == C.NWL_ERR_NONFINITE
    with pytest.raises(C.MappingError) as e:                      # a scale that is no power of two
        ctx.map(pts, band=b, values=vals, scales=[8192.0, 3.0, 1.0])
    assert e.value.code == C.NWL_ERR_BADARG
    M.same_accumulators(ctx.map(pts, band=b, values=vals, scales=scales), ref)      # and the context is as good as new


def test_device_pointers_give_what_host_arrays_give(ctx):
    import torch
    v, f, pts, b, vals, scales = case('sphere')
    ctx.set_mesh(v, f)
    host = ctx.map(pts, band=b, values=vals, scales=scales)
    tp, tv = torch.from_numpy(pts).to('cuda'), torch.from_numpy(np.ascontiguousarray(vals)).to('cuda')
    torch.cuda.synchronize()
    dev = ctx.map((tp.data_ptr(), len(pts)), band=b, values=(tv.data_ptr(), vals.shape[1]), scales=scales)
    M.same_as_restatement(dev, reference('sphere'))
    M.same_accumulators(dev, host)
    bad = pts.copy()
    bad[100, 1] = np.nan
    tb = torch.from_numpy(bad).to('cuda')
    torch.cuda.synchronize()
    with pytest.raises(C.MappingError) as e:
        ctx.map((tb.data_ptr(), len(bad)), band=b)
    assert e.value.code == C.NWL_ERR_NONFINITE
    with pytest.raises(C.MappingError) as e:
        ctx.map(bad, band=b)
    assert e.value.code == C.NWL_ERR_NONFINITE


def test_one_context_across_meshes_and_calls_chunks_and_a_shuffled_cloud():
    c = C.MappingContext()
    try:
        check(c, 'large')
        dev, ref = check(c, 'sphere')                             # a small mesh after a large one: nothing of the large one shows
        check(c, 'degenerate')
        v, f, pts, b, vals, scales = case('sphere')
        c.set_mesh(v, f)
        M.same_accumulators(c.map(pts, band=b, values=vals, scales=scales), ref)
        M.same_accumulators(c.map(pts, band=b, values=vals, scales=scales), ref)    # zeroed between calls
        twice = c.map(pts, band=b, values=vals, scales=scales, accumulate=True)
        assert np.array_equal(twice['mass'], 2 * ref['mass']) and np.array_equal(twice['count'], 2 * ref['count'])
        assert (C.column_sums(twice['sum_hi'], twice['sum_lo']) == 2 * M.column_sums(ref['sum_hi'], ref['sum_lo'])).all()
        acc = None
        for i, (s, e) in enumerate(((0, 1), (1, 300), (300, len(pts)))):
            acc = c.map(pts[s:e], band=b, values=vals[s:e], scales=scales, accumulate=i > 0)
        M.same_accumulators(acc, ref)
        old = C.CHUNK
        C.CHUNK = 256                                             # the binding's own chunking, five calls
        try:
            chunked = c.map(pts, band=b, values=vals, scales=scales)
        finally:
            C.CHUNK = old
        M.same_as_restatement(chunked, ref)
        assert chunked['n_in_band'] == ref['n_in_band']
        perm = np.random.default_rng(9).permutation(len(pts))
        M.same_accumulators(c.map(pts[perm], band=b, values=vals[perm], scales=scales), ref)
        walk = c.map(pts, band=b, walk_only=True)                 # the walk alone: the record, and no accumulator in sight
        assert 'mass' not in walk and np.array_equal(walk['face'], ref['face']) and walk['n_in_band'] == ref['n_in_band']
        with pytest.raises(C.MappingError) as e:
            c.map(pts, band=b, accumulate=True)                   # another number of columns than the accumulators at hand
        assert e.value.code == C.NWL_ERR_BADARG
        for band in (0.0, -1.0, np.inf, np.nan, 2.0 ** 41):
            with pytest.raises(C.MappingError) as e:
                c.map(pts, band=band)
            assert e.value.code == C.NWL_ERR_BADARG
    finally:
        c.close()
    c = C.MappingContext()
    try:
        with pytest.raises(C.MappingError) as e:
            c.map(np.zeros((3, 3)))
        assert e.value.code == C.NWL_ERR_NOMESH
        with pytest.raises(C.MappingError) as e:
            c.set_mesh(np.array([[0, 0, 0], [2.0 ** 21, 0, 0], [0, 2.0 ** 20, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
        assert e.value.code == C.NWL_ERR_BADARG                   # a face of area 2^40
    finally:
        c.close()


def test_face_distance_and_closest_point_are_distance_to_meshs(ctx):
    for name in ('sphere', 'degenerate', 'large'):
        v, f, pts, b, vals, scales = case(name)
        dist, closest, face = distance_to_mesh(pts, (v, f), signed=False, return_closest=True, return_face=True)
        dev = ctx.set_mesh(v, f).map(pts, band=b, accumulators=False)
        near = dev['face'] >= 0
        assert 0 < near.sum() < len(pts) and np.array_equal(near, dist <= b)
        assert np.array_equal(dev['face'][near], face[near]) and np.array_equal(D.bits(dev['distance'][near]), D.bits(dist[near]))
        assert np.array_equal(D.bits(dev['closest'][near]), D.bits(closest[near]))


def test_surface_density_and_the_recipe_on_a_sphere_with_one_hemisphere_four_times_as_dense():
    """The bracket is tests/test_surface_mapping_ref.py's: the caps |z| > 0.2 R hold about 6400 and 1600 localizations, the ratio's
    relative standard deviation is sqrt(1/6400 + 1/1600) = 0.028; five of them plus 1 % for the faces astride a cap's edge."""
    R = 100.0
    v, f = icosphere(2, R)
    mesh = TriMesh(v, f)
    pts = M.two_density_points(8000, R, 31, jitter=2.0)
    photons = np.where(pts[:, 2] > 0, 1000.0, 3000.0)
    ref = M.map_cloud(pts, v, f, 30.0, photons[:, None], [4096.0])
    r = mesh.surface_density(pts, band=30.0, values={'photons': photons})
    assert r['n_in_band'] == r['n_total'] == len(pts)
    M.same_accumulators(r['raw'], ref)
    n, area, density, means = M.densities(ref['mass'], M.vertex_areas(v, f), ref['sum_hi'], ref['sum_lo'], [4096.0])
    assert np.array_equal(r['density'], density) and np.array_equal(r['n'], n) and np.array_equal(r['area'], area)
    assert np.array_equal(r['means']['photons'], means[:, 0], equal_nan=True) and np.array_equal(r['count'], ref['count'])
    up, low = v[:, 2] > 0.2 * R, v[:, 2] < -0.2 * R
    ratio = (r['n'][up].sum() / r['area'][up].sum()) / (r['n'][low].sum() / r['area'][low].sum())
    assert 4 * 0.85 < ratio < 4 * 1.15
    assert np.allclose(r['means']['photons'][up], 1000.0) and np.allclose(r['means']['photons'][low], 3000.0)
    sm = mesh.surface_density(pts, band=30.0, smooth=2)
    assert np.isfinite(sm['density']).all() and sm['density'].std() < r['density'].std()
    # (a smoothed density is a ratio of sums over a patch: weighted by the vertices' own areas it still adds up to about the cloud)
    assert abs((sm['density'] * r['area']).sum() / len(pts) - 1) < 0.2 and sm['area'].min() > 10 * r['area'].min()
    ns = {'membrane': mesh, 'filtered_localizations': {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2], 'photons': photons}}
    table = C.SurfaceDensity(columns=['photons']).execute(ns)
    assert ns['membrane_density'] is table and sorted(table) == sorted(['x', 'y', 'z', 'density', 'n_localizations', 'area', 'mean_photons', 'metadata'])
    assert np.array_equal(table['density'], r['density']) and np.array_equal(table['x'], v[:, 0])
    mapped = ns['mapped_localizations']
    assert np.array_equal(mapped['surface_face'], ref['face']) and np.array_equal(D.bits(mapped['surface_distance']), D.bits(ref['distance']))
    assert mapped['photons'] is photons
    with pytest.raises(AttributeError):
        C.SurfaceDensity(colums=[])


def test_the_kernel_budgets_hold_with_the_new_rows():
    """(reads the object files the build leaves in csrc/, as tests/test_mapping_device_abi.py does without a GPU)"""
    res = build.check_kernel_budgets()
    for k in ('k_lm_face_setup', 'k_bq_face_setup', 'k_bq_rho_reduce', 'k_lm_map', 'k_lm_totals'):
        assert k in build.KERNEL_BUDGETS and res[k]['scratch'] == 0
    assert build.KERNEL_BUDGETS['k_lm_map'][0] == build.KERNEL_BUDGETS['k_vx_nodes'][0] == 128
