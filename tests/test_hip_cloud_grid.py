"""The cloud grid the four cloud query units share (bq::CloudGrid of csrc/nw_bq.h: set_cloud, bin, and the one scatter whose sorted point
carries its index), through the four public contexts only: k-th-neighbour distances, DBSCAN, pair counts and the local shape of five
small clouds against the restatements of tests/ (neighbours_ref, dbscan_ref, pair_counts_ref, local_shape_ref), exactly; the same with the
cloud's rows reversed, which shows that a point's index travels in the fourth word; a grid kept, binned anew and kept again on one
context per unit, buffers reused by a smaller cloud, a device pointer against the host path; and what a refused cloud leaves behind,
which differs between the units and is pinned here as it is."""
import functools

import numpy as np
import pytest

import dbscan_ref
import local_shape_ref
import neighbours_ref
import pair_counts_ref
from ch_shrinkwrap_amd import clustering, neighbours, pairs, structure

pytestmark = pytest.mark.gpu

F32 = np.float32


# ---- the clouds ---------------------------------------------------------------------------------------------------------------------------
def _lattice16():
    a = np.arange(16, dtype=F32)
    z, y, x = np.meshgrid(a, a, a, indexing='ij')
    return np.ascontiguousarray(np.stack([x.ravel(), y.ravel(), z.ravel()], 1))


def _line257():
    P = np.zeros((257, 3), F32)
    P[:, 0] = np.arange(257, dtype=F32) * F32(0.5)
    P[:, 1], P[:, 2] = F32(-3.0), F32(7.25)
    return P


def _far_cube():
    P = (np.random.default_rng(11).random((1000, 3)) + 1e6).astype(F32)        # float spacing 1/16 at 10^6: 17 values an axis
    assert len(np.unique(P, axis=0)) < len(P)                                      # many coincident points
    return P


# name -> (cloud, scale): the radii of a cloud are the ones below times its scale
CLOUDS = {
    'one point': (np.array([[3.0, -2.0, 7.0]], F32), 1.0),
    'two identical points': (np.array([[3.0, -2.0, 7.0]] * 2, F32), 1.0),                   # zero extent: one cell of side 1
    'line of 257': (_line257(), 1.0),                                                        # two axes without extent; two blocks of the scatter
    'lattice 16^3': (_lattice16(), 1.0),                                                     # points on the box's upper faces, distance ties
    'far cube': (_far_cube(), 1.0 / 16.0),
}
NAMES = list(CLOUDS)
K, MIN_POINTS = 3, 3                                              # clouds 1 and 2 have fewer than k points and no core point
EPS = 1.5                                                         # the lattice's axis and face-diagonal neighbours (sqrt 2 < 1.5 < sqrt 3)
RADIUS = 1.5
EDGES_NARROW = np.array([0.0, 1.0, 1.5, 2.0, 3.0])                                           # the zero edge counts coincident points
EDGES_WIDE = np.concatenate([[0.0], np.linspace(0.5, 3.0, 19)])                              # 20 bins: the other kernel variant
R_CAP = 2.0


def cloud(name, reverse=False):
    P = CLOUDS[name][0]
    return np.ascontiguousarray(P[::-1]) if reverse else P


def queries(name):
    """the cloud's own points, and each of them moved off the cloud (partly out of its box)"""
    P, s = CLOUDS[name]
    return np.concatenate([P, (P.astype(np.float64) + np.array([0.75, -0.5, 2.25]) * s).astype(F32)])


# ---- one adapter per unit: its context, a result as a dict of arrays, the restatement, the exact comparison --------------------------------
class Neighbours:
    make = neighbours.NeighbourContext
    per_point = ()

    @staticmethod
    def run(ctx, name, scale=1.0):
        s = CLOUDS[name][1]
        q = queries(name)
        return dict(capped=ctx.kth_distance(q, K, R_CAP * s * scale), free=ctx.kth_distance(q, K, np.inf) if scale == 1.0 else None)

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def ref(name):
        P, s = CLOUDS[name]
        return dict(capped=neighbours_ref.kth_distance(P, queries(name), K, R_CAP * s), free=neighbours_ref.kth_distance(P, queries(name), K, np.inf))

    @staticmethod
    def same(mine, ref):
        for k in ('capped', 'free'):
            assert mine[k].dtype == np.float64 and mine[k].tobytes() == ref[k].tobytes(), k

    @staticmethod
    def grid(out):
        return None                                               # (this ABI has no info words)


class Clustering:
    make = clustering.ClusterContext
    per_point = ('count', 'core')

    @staticmethod
    def run(ctx, name, scale=1.0):
        out = ctx.dbscan(EPS * CLOUDS[name][1] * scale, MIN_POINTS)
        out.update(ctx.stats())
        return out

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def ref(name):
        return dbscan_ref.dbscan(CLOUDS[name][0], EPS * CLOUDS[name][1], MIN_POINTS)

    same = staticmethod(dbscan_ref.same_as_restatement)

    @staticmethod
    def grid(out):
        return out['info']['cell_size'], out['info']['cells']


class Pairs:
    make = pairs.PairContext
    per_point = ('local', 'local_wide')

    @staticmethod
    def run(ctx, name, scale=1.0):
        s = CLOUDS[name][1] * scale
        out = ctx.set_edges(EDGES_NARROW * s).count(local=True)
        wide = ctx.set_edges(EDGES_WIDE * s).count(local=True)
        assert out['info']['variant'] == 'narrow' and wide['info']['variant'] == 'wide'
        out.update(hist_wide=wide['hist'], cumulative_wide=wide['cumulative'], local_wide=wide['local'], info_wide=wide['info'])
        return out

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def ref(name):
        P, s = CLOUDS[name]
        return pair_counts_ref.pair_counts(P, EDGES_NARROW * s), pair_counts_ref.pair_counts(P, EDGES_WIDE * s)

    @staticmethod
    def same(mine, ref):
        pair_counts_ref.same_as_restatement(mine, ref[0])
        wide = dict(hist=mine['hist_wide'], cumulative=mine['cumulative_wide'], local=mine['local_wide'], n_queries=mine['n_queries'], n_cloud=mine['n_cloud'])
        pair_counts_ref.same_as_restatement(wide, ref[1])

    @staticmethod
    def grid(out):
        assert (out['info']['cell_size'], out['info']['cells']) == (out['info_wide']['cell_size'], out['info_wide']['cells'])     # r_max is the same
        return out['info']['cell_size'], out['info']['cells']


class Structure:
    make = structure.StructureContext
    per_point = ('moments', 'eigenvalues', 'vectors', 'flags')

    @staticmethod
    def run(ctx, name, scale=1.0):
        return ctx.query(RADIUS * CLOUDS[name][1] * scale)

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def ref(name):
        return local_shape_ref.local_shape(CLOUDS[name][0], RADIUS * CLOUDS[name][1])

    same = staticmethod(local_shape_ref.same_as_restatement)

    @staticmethod
    def grid(out):
        return out['info']['cell_size'], out['info']['cells']


UNITS = {'neighbours': Neighbours, 'clustering': Clustering, 'pairs': Pairs, 'structure': Structure}


@pytest.fixture(scope='module')
def contexts():
    made = {u: U.make() for u, U in UNITS.items()}
    yield made
    for c in made.values():
        c.close()


def as_bytes(out):
    """every array of a result and its plain numbers; the info words are left to grid(): some of them count the tests of walks that end
    early, which depend on the order within a cell, and the atomic cursors of the scatter decide that anew at every binning"""
    flat = {}
    for k, v in sorted(out.items()):
        if isinstance(v, np.ndarray):
            flat[k] = (v.dtype.str, v.shape, v.tobytes())
        elif v is not None and not isinstance(v, dict):
            flat[k] = v
    return flat


# ---- every cloud through every unit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('unit', list(UNITS))
def test_the_result_is_the_restatement_and_reversed_rows_give_reversed_results(contexts, unit, name):
    U, ctx = UNITS[unit], contexts[unit]
    ctx.set_cloud(cloud(name))
    out = U.run(ctx, name)
    U.same(out, U.ref(name))
    if unit == 'neighbours':
        few = len(cloud(name)) < K
        assert np.isinf(out['free']).all() == few and (out['capped'] == R_CAP * CLOUDS[name][1]).all() == few       # fewer than k: the cap, or infinity
        return
    ctx.set_cloud(cloud(name, reverse=True))
    rev = U.run(ctx, name)
    for k in U.per_point:
        assert rev[k].dtype == out[k].dtype and np.array_equal(rev[k][::-1], out[k]), k
    if unit == 'clustering':
        assert dbscan_ref.partition(rev['labels'][::-1]) == dbscan_ref.partition(out['labels'])
        assert np.array_equal(rev['labels'][::-1] < 0, out['labels'] < 0) and rev['n_clusters'] == out['n_clusters']
        assert np.array_equal(np.sort(rev['sizes']), np.sort(out['sizes']))
        if len(cloud(name)) < MIN_POINTS:
            assert (out['labels'] == -1).all() and not out['core'].any() and out['n_clusters'] == 0                 # no neighbour, no cluster
    if unit == 'pairs':
        assert np.array_equal(rev['hist'], out['hist']) and np.array_equal(rev['hist_wide'], out['hist_wide'])
        if name == 'two identical points':
            assert out['hist'][0] == 2                                                                              # the zero edge: (0, 1) and (1, 0)
    if unit == 'structure' and len(cloud(name)) < 3:
        assert out['info']['few'] == len(cloud(name))                                                               # fewer than three neighbours


def test_a_node_field_reads_the_same_sorted_points(contexts):
    """the neighbour unit's second kernel, on the lattice: it reads the coordinates of a sorted point and leaves the index alone"""
    ctx, P = contexts['neighbours'], cloud('lattice 16^3')
    ctx.set_cloud(P)
    lo, h, dims = np.array([-1.0, -1.0, -1.0], F32), 1.5, (12, 11, 13)
    assert np.array_equal(ctx.node_field(lo, h, dims, K, R_CAP, return_field=True), neighbours_ref.node_field(P, lo, h, dims, K, R_CAP))


# ---- one context per unit: kept, binned anew, kept again; a smaller cloud; a device pointer -----------------------------------------------
@pytest.mark.parametrize('unit', list(UNITS))
def test_the_grid_is_kept_for_the_same_radius_and_binned_anew_for_another(unit):
    import torch
    U = UNITS[unit]
    ctx = U.make()
    try:
        ctx.set_cloud(cloud('lattice 16^3'))
        first = U.run(ctx, 'lattice 16^3')
        again = U.run(ctx, 'lattice 16^3')
        # the grid was kept: the same cell size and number of cells.  (The neighbour ABI has no info words, and its run() asks at two
        # caps, so that unit bins at every call: for it the lines below compare the results only, across one binning after another.)
        assert U.grid(first) == U.grid(again)
        assert as_bytes(again) == as_bytes(first)
        wider = U.run(ctx, 'lattice 16^3', scale=8.0)
        if U.grid(first) is not None:
            assert U.grid(wider)[0] > U.grid(first)[0] and U.grid(wider)[1] < U.grid(first)[1]           # binned anew: larger and fewer cells
        back = U.run(ctx, 'lattice 16^3')
        assert U.grid(back) == U.grid(first) and as_bytes(back) == as_bytes(first)                       # byte for byte
        U.same(back, U.ref('lattice 16^3'))
        # a smaller cloud after a larger one: every buffer is larger than needed
        ctx.set_cloud(cloud('line of 257'))
        small = U.run(ctx, 'line of 257')
        fresh = U.make()
        try:
            fresh.set_cloud(cloud('line of 257'))
            assert as_bytes(small) == as_bytes(U.run(fresh, 'line of 257'))
            # the same cloud through a device pointer
            t = torch.from_numpy(cloud('lattice 16^3')).cuda()
            torch.cuda.synchronize()
            fresh.set_cloud((t.data_ptr(), len(cloud('lattice 16^3'))))
            assert as_bytes(U.run(fresh, 'lattice 16^3')) == as_bytes(first)
        finally:
            fresh.close()
        U.same(small, U.ref('line of 257'))
    finally:
        ctx.close()


# ---- a refused cloud ----------------------------------------------------------------------------------------------------------------------
def refused(ctx, points):
    """set_cloud(points) is refused as non-finite.  What is pinned below is what the C-ABI's context holds afterwards, not the binding's
    bookkeeping: the binding zeroes its n_points before the call, and clustering, pairs and structure size their outputs by it, so it is
    put back to the size of the cloud the library may still hold (all clouds here have the same size)."""
    n = ctx.n_points
    with pytest.raises(RuntimeError, match='non-finite'):
        ctx.set_cloud(points)
    ctx.n_points = n


@pytest.mark.parametrize('unit', list(UNITS))
def test_a_non_finite_cloud_on_the_device_leaves_no_cloud(unit):
    import torch
    U = UNITS[unit]
    ctx = U.make()
    try:
        ctx.set_cloud(cloud('line of 257'))
        U.run(ctx, 'line of 257')
        bad = cloud('line of 257').copy()
        bad[200, 1] = np.inf
        t = torch.from_numpy(bad).cuda()
        torch.cuda.synchronize()
        refused(ctx, (t.data_ptr(), len(bad)))
        with pytest.raises(RuntimeError, match='no cloud'):
            U.run(ctx, 'line of 257')
        ctx.set_cloud(cloud('line of 257'))                       # ... and the context is as good as new
        U.same(U.run(ctx, 'line of 257'), U.ref('line of 257'))
    finally:
        ctx.close()


@pytest.mark.parametrize('unit', list(UNITS))
def test_a_non_finite_host_cloud_after_a_good_one(unit):
    """What is there today, and part of each ABI: the pairs and structure units forget their cloud when a host array is refused (a
    failed call leaves no cloud, whichever check failed); the neighbour and clustering units refuse it before anything is reset and go
    on answering from the cloud they had."""
    U = UNITS[unit]
    ctx = U.make()
    try:
        ctx.set_cloud(cloud('line of 257'))
        before = U.run(ctx, 'line of 257')
        bad = cloud('line of 257').copy()
        bad[13, 2] = np.nan
        refused(ctx, bad)
        if unit in ('pairs', 'structure'):
            with pytest.raises(RuntimeError, match='no cloud'):
                U.run(ctx, 'line of 257')
        else:
            assert as_bytes(U.run(ctx, 'line of 257')) == as_bytes(before)
    finally:
        ctx.close()
