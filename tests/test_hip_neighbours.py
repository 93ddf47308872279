"""The k-th-neighbour distance on the device (csrc/nw_neighbours.hip) against its brute-force restatement (tests/neighbours_ref.py): r_k and
the node field bit for bit, from host arrays and from device pointers, at the sizes and inputs where the walk, the list and the cap can
go wrong (tests/test_neighbours.py checks on the restatement that each input reaches its branch); nwi_set_field against surface_nets;
knn_isosurface against the restatement's chain; and the recipe DensitySurface(method='knn') -> ShrinkwrapMembrane on a sparse sphere."""
import ctypes

import numpy as np
import pytest

import isosurface_ref as IR
import neighbours_ref as R
from ch_shrinkwrap_amd import isosurface as I
from ch_shrinkwrap_amd import neighbours as N

pytestmark = pytest.mark.gpu

KS = [1, 2, 20, 31, 32]


@pytest.fixture(scope='module')
def ctx():
    """One context for the whole module: every test after the first reuses it across clouds of different size and different k."""
    c = N.NeighbourContext()
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check(ctx, pts, q, k, r_cap=np.inf, set_cloud=True):
    if set_cloud:
        ctx.set_cloud(pts)
    r = ctx.kth_distance(q, k, r_cap)
    ref = R.kth_distance(pts, q, k, r_cap)
    assert same_bits(r, ref), (k, r_cap, int((r != ref).sum()), float(np.abs(r - ref)[np.isfinite(ref)].max(initial=0.0)))
    return r


CLOUD = R.random_cloud(4097, 21)
QUERIES = R.queries_around(CLOUD, 513, 22)


@pytest.mark.parametrize('k', KS)
def test_kth_distance_from_host_arrays_and_device_pointers(ctx, k):
    import torch
    r = check(ctx, CLOUD, QUERIES, k)
    assert (r[:128] == 0).all() == (k == 1)                     # the first queries are cloud points: they count themselves
    capped = check(ctx, CLOUD, QUERIES, k, 60.0, set_cloud=False)
    assert (capped == 60.0).any() and (capped < 60.0).any()
    dp, dq = torch.from_numpy(CLOUD).cuda(), torch.from_numpy(QUERIES).cuda()
    torch.cuda.synchronize()
    ctx.set_cloud((dp.data_ptr(), CLOUD.shape[0]))
    assert same_bits(ctx.kth_distance((dq.data_ptr(), QUERIES.shape[0]), k), r)
    assert same_bits(ctx.kth_distance((dq.data_ptr(), QUERIES.shape[0]), k, 60.0), capped)
    assert same_bits(ctx.kth_distance(QUERIES, k, 60.0), capped)                       # a device cloud, host queries


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 4097])
def test_cloud_sizes_and_query_counts(ctx, n):
    """Blocks are 128 lanes: 127, 128, 129 and 513 queries end in a partial block, a full one, one lane of a second and of a fifth.
    k > n gives the cap (inf without one)."""
    pts = CLOUD[:n]
    ctx.set_cloud(pts)
    for nq in (1, 127, 128, 129, 513):
        for k, cap in ((1, np.inf), (2, np.inf), (20, np.inf), (20, 35.0), (32, 250.0)):
            r = check(ctx, pts, QUERIES[:nq], k, cap, set_cloud=False)
            if k > n:
                assert (r == cap).all()


def test_k_out_of_range_is_refused_on_a_live_context(ctx):
    ctx.set_cloud(CLOUD[:100])
    out = np.empty(4)
    q = np.ascontiguousarray(QUERIES[:4])
    for k in (0, 33, -1):
        assert ctx.L.nwk_kth_distance(ctx.h, q.ctypes.data, 4, 0, k, float('inf'), out.ctypes.data) == N.NWK_ERR_BADARG
        with pytest.raises(RuntimeError, match='bad argument'):
            ctx.kth_distance(q, k)
        with pytest.raises(RuntimeError, match='bad argument'):
            ctx.node_field(np.zeros(3, np.float32), 1.0, [4, 4, 4], k, 5.0)
    for cap in (0.0, -2.0, float('nan')):
        with pytest.raises(RuntimeError, match='bad argument'):
            ctx.kth_distance(q, 3, cap)
    with pytest.raises(RuntimeError, match='bad argument'):
        ctx.node_field(np.zeros(3, np.float32), 1.0, [4, 4, 4], 3, np.inf)
    check(ctx, CLOUD[:100], q, 32, set_cloud=False)                                    # the context is as it was
    bad = q.copy()
    bad[2, 1] = np.nan
    with pytest.raises(RuntimeError, match='non-finite'):
        ctx.kth_distance(bad, 3)
    fresh = N.NeighbourContext()
    try:
        with pytest.raises(RuntimeError, match='no cloud'):
            fresh.kth_distance(q, 3)
        with pytest.raises(RuntimeError, match='no cloud'):
            fresh.node_field(np.zeros(3, np.float32), 1.0, [4, 4, 4], 3, 5.0)
        assert fresh.field_pointer() == 0
    finally:
        fresh.close()


def test_non_finite_on_the_device_is_reported(ctx):
    import torch
    bad = QUERIES[:200].copy()
    bad[150, 2] = np.inf
    ctx.set_cloud(CLOUD[:100])
    d = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='non-finite'):
        ctx.kth_distance((d.data_ptr(), 200), 3)
    with pytest.raises(RuntimeError, match='non-finite'):
        ctx.set_cloud((d.data_ptr(), 200))
    with pytest.raises(RuntimeError, match='no cloud'):                                # a failed set_cloud leaves none
        ctx.kth_distance(QUERIES[:4], 3)


@pytest.mark.parametrize('k', KS)
def test_lattice_with_ties(ctx, k):
    pts, q = R.lattice_case()
    r = check(ctx, pts, q, k)
    check(ctx, pts[::-1], q, k)                                                        # the order of the cloud does not show
    assert same_bits(check(ctx, pts, q, k, 1.5), np.minimum(r, 1.5))                   # nor does the cell size a cap brings


def test_copies_of_one_point(ctx):
    pts, q = R.copies_case()
    for k in KS:
        r = check(ctx, pts, q, k)
        assert r[0] == 0.0 and r[1] == 1.0
    assert (check(ctx, pts[:20], q, 21) == np.inf).all()


@pytest.mark.parametrize('kind', ['plane', 'axis', 'diagonal'])
def test_grids_one_cell_thick(ctx, kind):
    pts, q = R.flat_case(kind)
    for k, cap in ((1, np.inf), (20, np.inf), (20, 12.0), (32, 3.0)):
        check(ctx, pts, q, k, cap)


def test_queries_far_outside_the_box(ctx):
    pts, q, diag = R.far_case()
    for k, cap in ((1, np.inf), (20, np.inf), (32, np.inf), (20, 11.0 * diag), (20, 5.0 * diag)):
        r = check(ctx, pts, q, k, cap)
        assert (r > 10 * diag).all() if cap > 10 * diag else (r == cap).all()


@pytest.mark.parametrize('where', ['below', 'at', 'above'])
def test_twentieth_neighbour_at_the_cap(ctx, where):
    pts, q, k, r_cap = R.cap_case(where)
    r = check(ctx, pts, q, k, r_cap)
    assert r[0] == (40.0 if where != 'above' else r_cap)
    check(ctx, pts, q, k, np.inf, set_cloud=False)
    check(ctx, pts, q, k + 1, r_cap, set_cloud=False)
    check(ctx, pts, q, k - 1, r_cap, set_cloud=False)


@pytest.mark.parametrize('name', sorted(R.NODE_GRIDS))
def test_node_field_is_bit_identical(ctx, name):
    import torch
    pts, lo, h, dims = R.node_case(name)
    for k, cap in ((3, 4.0), (20, 8.0), (1, 2.0 ** 40)):
        ref = R.node_field(pts, lo, h, dims, k, cap)
        ctx.set_cloud(pts)
        f = ctx.node_field(lo, h, dims, k, cap, return_field=True)
        assert f.dtype == np.uint64 and np.array_equal(f, ref), (name, k, cap, int((f != ref).sum()))
        assert ctx.field_pointer() != 0
        dp = torch.from_numpy(pts).cuda()
        torch.cuda.synchronize()
        ctx.set_cloud((dp.data_ptr(), pts.shape[0]))
        assert np.array_equal(ctx.node_field(lo, h, dims, k, cap, return_field=True), ref)


def test_node_that_is_a_cloud_point(ctx):
    pts, lo, h, dims, index = R.coincident_node_case()
    ctx.set_cloud(pts)
    for k in (1, 2):
        f = ctx.node_field(lo, h, dims, k, 6.0, return_field=True)
        assert np.array_equal(f, R.node_field(pts, lo, h, dims, k, 6.0))
    assert ctx.node_field(lo, h, dims, 1, 6.0, return_field=True)[index[2], index[1], index[0]] == 6 << 20      # r_1 = 0 there


def test_one_context_across_clouds_and_k(ctx):
    """Large, small, large again; k and the cap (and with it the cell size) changing between calls on one cloud."""
    small, sq = R.copies_case()
    first = check(ctx, CLOUD, QUERIES, 20)
    check(ctx, small, sq, 2)
    check(ctx, CLOUD[:65], QUERIES[:129], 32, 80.0)
    assert same_bits(check(ctx, CLOUD, QUERIES, 20), first)
    for k, cap in ((1, 5.0), (32, np.inf), (20, 500.0), (2, 0.25), (20, np.inf)):
        r = check(ctx, CLOUD, QUERIES, k, cap, set_cloud=False)
    assert same_bits(r, first)
    dens = N.local_density(CLOUD, 20, context=ctx)
    assert same_bits(dens, R.local_density(CLOUD, 20))
    assert same_bits(N.kth_distance(CLOUD[:300], k=3), R.kth_distance(CLOUD[:300], CLOUD[:300], 3))             # a context of its own
    with pytest.raises(ValueError):
        N.local_density(CLOUD[:20], 20)


def test_set_field_extracts_surface_nets_arrays():
    pts, lo, h, dims, counts = IR.noise_case(0)
    field = IR.smooth(counts, 0)
    rv, rf, rk = IR.surface_nets(field, 1, lo, h)
    c = I.IsosurfaceContext()
    try:
        with pytest.raises(RuntimeError, match='call out of order'):
            c.extract(1)
        c.set_field(field, lo, h, dims)
        v, f, k = c.extract(1, return_keys=True)
        IR.compare_mesh('set_field noise', v, f, k, rv, rf, rk)
        thr = ctypes.c_uint64()
        assert c.L.nwi_threshold_auto(c.h, 0.3, None, ctypes.byref(thr), None, None) == I.NWI_ERR_STATE            # there are no counts
        with pytest.raises(RuntimeError, match='call out of order'):
            c.threshold_auto(0.3)
        v, f, k = c.extract(1, return_keys=True)                                                                    # ... and the field is still there
        IR.compare_mesh('set_field noise again', v, f, k, rv, rf, rk)
        with pytest.raises(ValueError):
            c.set_field(field[:-1], lo, h, dims)
        # a later nwi_density works as before
        dfield, dcounts = c.density(pts, lo, h, dims, 1, return_field=True, return_counts=True)
        ref_field, ref_counts = IR.density(pts, lo, h, dims, 1)
        assert np.array_equal(dfield, ref_field) and np.array_equal(dcounts, ref_counts)
        t = c.threshold_auto(0.3)
        assert (t['thr'], t['median'], t['n_occupied']) == IR.threshold_auto(ref_field, ref_counts, 0.3)
        # ... and a field adopted after a density takes the counts away again
        c.set_field(field, lo, h, dims)
        with pytest.raises(RuntimeError, match='call out of order'):
            c.threshold_auto(0.3)
    finally:
        c.close()


def test_knn_isosurface_equals_the_restatement():
    pts = R.topology_cloud('sphere', 1000)
    rv, rf, rk, rinfo = R.topology_reference('sphere', 1000)
    v, f, info = I.knn_isosurface(pts, R.TOPOLOGY_H['sphere'], 20)
    for key in ('R_thr', 'r_cap', 'threshold_density', 'median_density', 'thr', 'pad', 'h'):
        assert info[key] == rinfo[key], key
    assert np.array_equal(info['lo'], rinfo['lo']) and np.array_equal(info['dims'], rinfo['dims'])
    # keys: through a context of its own on the same field
    nctx, c = N.NeighbourContext(), I.IsosurfaceContext()
    try:
        nctx.set_cloud(pts)
        field = nctx.node_field(info['lo'], info['h'], info['dims'], 20, info['r_cap'], return_field=True)
        assert np.array_equal(field, rinfo['field'])
        c.set_field(nctx.field_pointer(), info['lo'], info['h'], info['dims'])
        v2, f2, k2 = c.extract(info['thr'], return_keys=True)
    finally:
        nctx.close()
        c.close()
    IR.compare_mesh('knn sphere 1000', v2, f2, k2, rv, rf, rk)
    assert np.array_equal(v, v2) and np.array_equal(f, f2)
    # a given threshold_density: upstream's parameter, the bandwidth from (threshold_density, n_points_min)
    v3, f3, info3 = I.knn_isosurface(pts, R.TOPOLOGY_H['sphere'], 20, threshold_density=rinfo['threshold_density'])
    assert info3['median_density'] is None and info3['R_thr'] == rinfo['R_thr'] and np.array_equal(f3, f) and np.array_equal(v3, v)


def test_recipe_from_a_sparse_cloud():
    """DensitySurface(method='knn') then ShrinkwrapMembrane (the module's defaults) on the 1 000-point sphere (R = 100 nm, sigma = 10 nm),
    in the reference's metric against the true sphere.  The fit must be better than the start surface it was given; the figures are
    printed before they are asserted."""
    from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane
    from ch_shrinkwrap_amd.evaluation import fit_quality, mesh_topology
    from ch_shrinkwrap_amd.trimesh import TriMesh
    pts = R.topology_cloud('sphere', 1000)
    truth = R.sphere_cloud(20000, 99, sigma=0.0).astype(np.float64)
    sig = np.full(pts.shape[0], 10.0, np.float32)
    ns = {'filtered_localizations': {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2], 'error_x': sig, 'error_y': sig, 'error_z': sig}}
    surf = I.DensitySurface(method='knn', voxel_size=R.TOPOLOGY_H['sphere']).execute(ns)
    assert ns['surf'] is surf and surf.info['method'] == 'knn' and surf.info['n_points_min'] == 20
    mesh = ShrinkwrapMembrane().execute(ns)

    def stats(v, f):
        t = mesh_topology(f, len(v))
        return t['euler'], bool(t['manifold']), t['border_loops'], len(IR.components(np.asarray(v), np.asarray(f)))
    s0 = stats(surf.vertices, surf.faces)
    s1 = stats(np.asarray(mesh.vertices), np.asarray(mesh.faces))
    q0 = fit_quality(TriMesh(surf.vertices, surf.faces), truth)
    q1 = fit_quality(mesh, truth)
    print('start surface: R_thr %.1f nm, %d faces, removed %s, (euler, manifold, border loops, components) %s, mse_rms %.3f nm' %
          (surf.info['R_thr'], surf.faces.shape[0], surf.info['removed'], s0, q0['mse_rms']))
    print('fit: %d faces, %s, mse_rms %.3f nm' % (len(mesh.faces), s1, q1['mse_rms']))
    assert s0 == (2, True, 0, 1) and s1 == (2, True, 0, 1)
    assert q1['mse_rms'] < q0['mse_rms']
