"""Pair counts on the device (csrc/nw_pairs.hip) against the NumPy restatement (tests/pair_counts_ref.py), bit for bit: hist, cumulative and
the per-query counts -- on cloud sizes around the wave and the workgroups of both variants, on bin counts on both sides of the variant
switch, on the lattice at exact edges and one ulp beside them, on duplicates and on 5 000 points in one cell, with a largest radius a
thousand times the extent and one below the smallest pair distance, on degenerate extents, with cross queries on the box's faces, far
outside it and at cloud points, from host arrays and device pointers through one context, twice, shuffled, with and without `local`;
then against the clustering unit, which knows nothing of this one, and through RipleysK and PairwiseDistanceHistogram."""
import functools

import numpy as np
import pytest

import pair_counts_ref as R
from ch_shrinkwrap_amd import pairs as C

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 257, 1025, 4097]
BINS = [1, 2, 15, 16, 17, 63, 64]


@pytest.fixture(scope='module')
def ctx():
    c = C.PairContext()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def cloud(n):
    return R.clustered(n, n + 1)


def radii(m, r_max=9.0, zero=False):
    r = np.linspace(0.0 if zero else r_max / m, r_max, m)
    return r


@functools.lru_cache(maxsize=None)
def reference(n, m):
    """the restatement once per size and bin count"""
    return R.pair_counts(cloud(n), radii(m))


def every_tenth(ref):
    """the restatement for every tenth edge of the 40 from the one for all 40: with nested edges a coarse bin is the union of its fine ones"""
    local = ref['local'].reshape(len(ref['local']), 4, 10).sum(2, dtype=np.uint32)
    hist = local.sum(0, dtype=np.uint64)
    return dict(ref, local=local, hist=hist, cumulative=np.cumsum(hist, dtype=np.uint64))


def run(ctx, P, r, queries=None, local=True, on_device=False):
    if on_device:
        import torch
        keep = [torch.from_numpy(np.ascontiguousarray(P, np.float32)).to('cuda')]
        cl = (keep[0].data_ptr(), len(P))
        if queries is not None:
            keep.append(torch.from_numpy(np.ascontiguousarray(queries, np.float32)).to('cuda'))
            queries = (keep[1].data_ptr(), len(keep[1]))
        torch.cuda.synchronize()
        ctx.set_cloud(cl)
    else:
        ctx.set_cloud(P)
    ctx.set_edges(r)
    return ctx.count(queries, local=local)


def check(ctx, P, r, queries=None, ref=None):
    """host arrays, device pointers, once more on the cloud at hand, and without local: the restatement's bytes every time"""
    if ref is None:
        ref = R.pair_counts(P, r) if queries is None else R.pair_counts(queries, r, other=P)
    host = run(ctx, P, r, queries)
    R.same_as_restatement(host, ref)
    dev = run(ctx, P, r, queries, on_device=True)
    R.same_as_restatement(dev, ref)
    again = ctx.count(None if queries is None else queries, local=True)
    R.same_as_restatement(again, ref)
    assert again['local'].tobytes() == host['local'].tobytes() and again['hist'].tobytes() == host['hist'].tobytes()
    bare = ctx.count(None if queries is None else queries, local=False)
    R.same_as_restatement(bare, ref, local=False)
    assert bare['local'] is None
    info = host['info']
    assert info['variant'] == ('wide' if len(r) > C.NARROW_BINS else 'narrow') and info['bins'] == len(r)
    assert info['tests'] >= int(ref['hist'].sum()) and info['cells_read'] >= 1 and info['n_cloud'] == len(P)
    assert again['info']['tests'] == info['tests'] == dev['info']['tests']               # what is tested depends on the grid alone
    return host, ref


@pytest.mark.parametrize('n', SIZES)
def test_sizes_around_the_wave_and_the_workgroups(ctx, n):
    ref = reference(n, 40)                                        # both variants at every size, on one pass of the restatement
    check(ctx, cloud(n), radii(40), ref=ref)
    check(ctx, cloud(n), radii(40)[9::10], ref=every_tenth(ref))


@pytest.mark.parametrize('m', BINS)
def test_bin_counts_on_both_sides_of_the_variant_switch(ctx, m):
    check(ctx, cloud(1025), radii(m), ref=reference(1025, m))
    check(ctx, cloud(257), radii(m, zero=True))


@pytest.mark.parametrize('edges', [[1.0, 1.5, 2.0], [float(np.nextafter(1.0, 0.0)), 1.5, 2.0], [float(np.nextafter(1.0, 2.0)), 1.5, 2.0],
                                   list(np.sqrt(np.arange(1.0, 18.0))), list(np.nextafter(np.sqrt(np.arange(1.0, 18.0)), 0.0))],
                         ids=['exact', 'below', 'above', 'wide_exact', 'wide_below'])
def test_the_lattice_at_exact_edges_and_one_ulp_beside_them(ctx, edges):
    host, ref = check(ctx, R.lattice(7), edges)
    if edges[:1] == [1.0] and len(edges) == 3:
        assert host['hist'].tolist() == [1764, 3024, 3198]
    if edges[0] < 1.0 and len(edges) == 3:
        assert host['hist'].tolist() == [0, 4788, 3198]


def test_duplicates_with_a_zero_edge(ctx):
    dup = np.tile(np.array([[3.0, -2.0, 7.5]], np.float32), (300, 1))
    host, _ = check(ctx, dup, [0.0, 0.5])
    assert host['hist'].tolist() == [300 * 299, 0]
    host, _ = check(ctx, dup, [0.0])
    assert host['hist'].tolist() == [300 * 299]
    mixed = np.concatenate([dup[:40], cloud(257), dup[:40]])
    check(ctx, mixed, list(np.linspace(0.0, 30.0, 20)))


def test_five_thousand_points_in_one_cell(ctx):
    P = np.random.default_rng(8).uniform(0.0, 0.5, (5000, 3)).astype(np.float32)
    ctx.set_cloud(P).set_edges([1.0])
    out = ctx.count(local=True)
    assert out['info']['cells'] == 1 and out['info']['tests'] == 5000 * 4999
    assert (out['local'][:, 0] == 4999).all() and out['hist'].tolist() == [5000 * 4999]
    wide = np.linspace(0.02, 1.0, 50)                             # the same crowd through the search: nothing is further than 0.87
    out = ctx.set_edges(wide).count(local=True)
    assert int(out['hist'].sum()) == 5000 * 4999 and (out['local'].sum(1) == 4999).all()
    assert np.array_equal(out['local'].sum(0, dtype=np.uint64), out['hist'])
    some = ctx.count(P[:600], local=True)                         # 600 of its points as cross queries, against the restatement
    R.same_as_restatement(some, R.pair_counts(P[:600], wide, other=P))
    assert np.array_equal(some['local'][:, 1:], out['local'][:600, 1:]) and np.array_equal(some['local'][:, 0], out['local'][:600, 0] + 1)


def test_extreme_radii(ctx):
    P = cloud(1025)
    ext = float((P.max(0) - P.min(0)).max())
    host, _ = check(ctx, P, [1000.0 * ext])                        # one cell, everything in one bin
    assert host['info']['cells'] == 1 and host['hist'].tolist() == [1025 * 1024]
    host, _ = check(ctx, P, [0.5 * ext, 1000.0 * ext] + [1001.0 * ext + k for k in range(20)])
    assert int(host['hist'][:2].sum()) == 1025 * 1024 and not host['hist'][2:].any()
    U = np.unique(P, axis=0)
    e = U.astype(np.float64)[None, :, :] - U.astype(np.float64)[:, None, :]
    d2 = (e ** 2).sum(-1)
    tiny = float(np.sqrt(d2[d2 > 0].min())) * 0.5                 # below the smallest pair distance: all zeros
    host, _ = check(ctx, U, [tiny / 2, tiny])
    assert not host['hist'].any() and not host['local'].any()
    host, _ = check(ctx, U, list(np.linspace(tiny / 30, tiny, 30)))
    assert not host['hist'].any()


@pytest.mark.parametrize('name', ['plane', 'axis', 'one_point', 'far'])
def test_degenerate_extents(ctx, name):
    if name == 'plane':
        P = cloud(1025).copy()
        P[:, 2] = 3.0
    elif name == 'axis':
        P = np.zeros((400, 3), np.float32)
        P[:, 1] = np.random.default_rng(9).uniform(0.0, 300.0, 400)
    elif name == 'one_point':
        P = np.array([[1.0, 2.0, 3.0]], np.float32)
    else:
        P = R.clustered(900, 10, offset=1.0e6)                    # float32 steps of 1/16 out there
    check(ctx, P, [2.0, 4.0, 6.5, 9.0])
    check(ctx, P, list(np.linspace(0.0, 12.0, 33)))
    if name == 'one_point':
        Q = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 4.0], [100.0, 2.0, 3.0]], np.float32)
        host, _ = check(ctx, P, [0.0, 1.0, 5.0], queries=Q)
        assert host['local'].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 0]]


@functools.lru_cache(maxsize=None)
def cross_queries(where):
    rng = np.random.default_rng(5)
    P = cloud(1025)
    lo, hi = P.min(0).astype(np.float64), P.max(0).astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    if where == 'faces':                                          # on the box's faces, edges and corners
        Q = rng.uniform(lo, hi, (200, 3))
        for k in range(len(Q)):
            for d in range(3):
                if (k >> d) & 1 or k % 3 == d:
                    Q[k, d] = lo[d] if (k >> (d + 3)) & 1 else hi[d]
    elif where == 'outside':                                      # up to ten diagonals away, in every direction
        u = rng.normal(size=(513, 3))
        Q = (lo + hi) / 2 + u / np.linalg.norm(u, axis=1)[:, None] * rng.uniform(0.3, 10.0, (513, 1)) * diag
    elif where == 'at_points':
        Q = P[rng.integers(0, len(P), 129)]
    else:
        Q = rng.uniform(lo - 5.0, hi + 5.0, (513, 3))
    return Q.astype(np.float32), diag


@pytest.mark.parametrize('where', ['faces', 'outside', 'at_points', 'around'])
def test_cross_queries(ctx, where):
    Q, diag = cross_queries(where)
    P = cloud(1025)
    check(ctx, P, [2.0, 4.0, 6.5, 9.0], queries=Q)
    check(ctx, P, list(np.linspace(0.0, 40.0, 41)), queries=Q)
    if where == 'outside':
        host, _ = check(ctx, P, [0.0, 12.0 * diag], queries=Q)    # every pair, from far outside the box
        assert host['hist'].tolist() == [0, 513 * 1025]


@pytest.mark.parametrize('nq', [1, 2, 63, 64, 65, 127, 128, 129, 513])
def test_cross_query_counts_around_the_wave_and_the_workgroups(ctx, nq):
    Q, _ = cross_queries('around')
    P = cloud(257)
    check(ctx, P, radii(5, 12.0), queries=Q[:nq])
    check(ctx, P, radii(24, 12.0), queries=Q[:nq])


def test_identities_on_the_device(ctx):
    P = cloud(1025)
    r = radii(7, 9.0, zero=True)
    auto = run(ctx, P, r)
    perm = np.random.default_rng(2).permutation(len(P))          # a shuffled cloud: hist is equal, local is permuted
    shuf = run(ctx, P[perm], r)
    assert np.array_equal(shuf['hist'], auto['hist']) and np.array_equal(shuf['local'], auto['local'][perm])
    cross = run(ctx, P, r, queries=P)                             # auto against cross: n more in bin 0
    assert np.array_equal(cross['local'][:, 1:], auto['local'][:, 1:]) and np.array_equal(cross['local'][:, 0], auto['local'][:, 0] + 1)
    assert int(cross['hist'][0]) == int(auto['hist'][0]) + len(P)
    one = C.pair_counts(P, r, local=True)                         # the one-call form, with a context of its own
    assert np.array_equal(one['hist'], auto['hist']) and np.array_equal(one['local'], auto['local'])
    two = C.pair_counts(P[:100], r, other=P, context=ctx)
    assert two['local'] is None and np.array_equal(two['hist'], cross['local'][:100].sum(0, dtype=np.uint64))


def test_edges_changed_on_a_kept_cloud_and_errors_leave_the_context_usable(ctx):
    P = cloud(1025)
    ctx.set_cloud(P)
    for m, r_max in ((3, 9.0), (40, 9.0), (5, 2.0), (64, 30.0), (3, 9.0)):
        out = ctx.set_edges(radii(m, r_max)).count(local=True)
        R.same_as_restatement(out, R.pair_counts(P, radii(m, r_max)) if (m, r_max) != (3, 9.0) else reference(1025, 3))
    with pytest.raises(RuntimeError):
        ctx.set_edges([2.0, 1.0])
    out = ctx.count(local=True)                                   # the edges it had
    R.same_as_restatement(out, reference(1025, 3))
    bad = P.copy()
    bad[7, 1] = np.nan
    with pytest.raises(RuntimeError):
        ctx.set_cloud(bad)
    with pytest.raises(RuntimeError):                             # a failed set_cloud leaves no cloud
        ctx.count()
    import torch
    t = torch.from_numpy(bad).to('cuda')
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):                             # the same from a device pointer: the bounding-box kernel notices
        ctx.set_cloud((t.data_ptr(), len(bad)))
    ctx.set_cloud(P)
    with pytest.raises(RuntimeError):                             # a device query that is not finite: the kernel notices
        ctx.count((t.data_ptr(), len(bad)))
    R.same_as_restatement(ctx.count(local=True), reference(1025, 3))
    fresh = C.PairContext()
    try:
        with pytest.raises(RuntimeError):
            fresh.set_cloud(P).count()                            # no edges yet
    finally:
        fresh.close()


def test_cumulative_counts_are_the_clustering_units(ctx):
    """cumulative_local[:, b] + 1 == dbscan(points, r_b, 1, count_cap=n)['count']: the same d2 <= r_b^2, itself included there"""
    from ch_shrinkwrap_amd.clustering import dbscan
    P = cloud(1025)
    r = radii(20, 9.0)
    out = run(ctx, P, r)
    cum = np.cumsum(out['local'], axis=1, dtype=np.int64)
    for b in (0, 7, 19):
        assert np.array_equal(cum[:, b] + 1, dbscan(P, float(r[b]), 1, count_cap=len(P))['count'])


def test_the_recipe_modules_on_a_two_cluster_table(ctx):
    rng = np.random.default_rng(21)
    P = np.concatenate([rng.normal((0, 0, 0), 4.0, (400, 3)), rng.normal((60, 10, 0), 4.0, (400, 3)), rng.uniform(-20, 80, (200, 3))]).astype(np.float32)
    table = {'x': P[:, 0], 'y': P[:, 1], 'z': P[:, 2], 'photons': np.arange(len(P), dtype=np.float32)}
    ns = {'filtered_localizations': table}
    h = C.PairwiseDistanceHistogram(r_max=50.0, n_bins=25).execute(ns)
    edges = np.linspace(0.0, 50.0, 26)
    ref = R.pair_counts(P, edges[1:])
    assert ns['pair_histogram'] is h and np.array_equal(h['count'], ref['hist'])
    assert np.array_equal(h['bin_left'], edges[:-1]) and np.array_equal(h['bin_right'], edges[1:])
    V = float(np.prod(P.max(0).astype(np.float64) - P.min(0).astype(np.float64)))
    N = len(P) * (len(P) - 1.0)
    assert np.allclose(h['g'], ref['hist'] * V / (N * 4.0 / 3.0 * np.pi * np.diff(edges ** 3)), rtol=1e-12)
    assert h['g'][:4].min() > 3.0 and h['metadata']['n_pairs'] == N                 # clustered at the clusters' scale
    k = C.RipleysK(r_max=50.0, n_steps=25, local_radius=10.0).execute(ns)
    K = V * ref['cumulative'].astype(np.float64) / N
    assert np.allclose(k['K'], K, rtol=1e-12) and np.allclose(k['L'], np.cbrt(3.0 * K / (4.0 * np.pi)), rtol=1e-12)
    assert np.allclose(k['H'], k['L'] - k['r'], rtol=0, atol=1e-12) and np.array_equal(k['r'], edges[1:]) and k['H'][4] > 5.0
    loc = ns['ripley_localizations']
    one = R.pair_counts(P, [10.0])
    want = np.cbrt(3.0 * (V * one['local'][:, 0].astype(np.float64) / (len(P) - 1.0)) / (4.0 * np.pi))
    assert np.allclose(loc['ripley_local_L'], want, rtol=1e-12) and np.array_equal(loc['photons'], table['photons'])
    assert loc['ripley_local_L'][:800].mean() > 2.0 * loc['ripley_local_L'][800:].mean()        # the clusters' points see more neighbours
    two = C.PairwiseDistanceHistogram(input2='second', r_max=30.0, n_bins=10)                 # two tables: A against B
    Q = P[800:]
    ns['second'] = {'x': Q[:, 0], 'y': Q[:, 1], 'z': Q[:, 2]}
    h2 = two.execute(ns)
    assert np.array_equal(h2['count'], R.pair_counts(P, np.linspace(0.0, 30.0, 11)[1:], other=Q)['hist'])
    r2 = C.ripley(P[:300], [5.0, 10.0], dim=2, volume=100.0 * 100.0, local=True, context=ctx)
    assert r2['L_local'].shape == (300, 2) and np.allclose(r2['L'], np.sqrt(r2['K'] / np.pi))
