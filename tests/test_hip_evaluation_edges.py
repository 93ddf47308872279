"""The fit-quality kernels (csrc/nw_evaluation.hip) and the shared exclusive scan (csrc/nw_bq.hip) at their edges: reference clouds that
are flat, collinear, skewed by an outlier or a single point; exact ties between reference points of different cells and rings; query
counts around the wave and the block; scans around the tile (2048) and the chunk of tile sums (1024 tiles = 2^21 elements); meshes whose
node counts are mostly zero, or nearly all in one face.  Every case asserts on the host, from a restatement of the grid's sizing or from
the host sampler's node counts, that it reaches the branch it is named for, before it touches the device."""
import collections
import itertools

import numpy as np
import pytest

from ch_shrinkwrap_amd import evaluation as E
from ch_shrinkwrap_amd.trimesh import icosphere
from test_hip_evaluation import Duck, _bits, check_nearest, check_samples, cloud_pair
from test_evaluation_core_cpu import EDGE_MESHES, edge_mesh, edge_mesh_premise

pytestmark = pytest.mark.gpu

OFFSET = np.array([5000.0, -3000.0, 800.0])
TILE, CHUNK = 2048, 1 << 21          # elements a workgroup of the scan takes; elements after which k_bq_scan_bsums carries


@pytest.fixture(scope='module')
def ctx():
    c = E.EvaluationContext()
    yield c
    c.close()


# ---- make_grid of nw_evaluation.hip, restated -------------------------------------------------------------------------------------------
Grid = collections.namedtuple('Grid', 'lo hi ext emax h dims cap floored clamped widened')


def grid_of(ref):
    """The cell grid nwe_nearest lays over a reference cloud: floored = the axes that count as a thousandth of the widest, clamped =
    whether h is emax / 1024, widened = how often h grew by a tenth to fit the cap on the number of cells."""
    n = ref.shape[0]
    lo, hi = ref.min(0), ref.max(0)
    ext = hi - lo
    emax = float(ext.max())
    h, floored, clamped = 1.0, ext < 1e-3 * emax, False
    if emax > 0.0:
        e = np.maximum(ext, 1e-3 * emax)
        h = float(np.cbrt(e[0] * e[1] * e[2] / n))
        clamped = h < emax / 1024.0
        h = max(h, emax / 1024.0)
    cap = min(max(2 * n, 65536), 1 << 28)
    for widened in range(400):
        dims = np.minimum(1025.0, np.floor(ext / h) + 1.0).astype(np.int64)
        if dims.prod() <= cap:
            break
        h *= 1.1
    return Grid(lo, hi, ext, emax, h, tuple(int(d) for d in dims), cap, floored, clamped, widened)


def cells_of(g, pts):
    """the cell of every point, as k_ev_cell_count numbers them"""
    c = np.clip(np.floor((pts - g.lo) / g.h), 0, np.array(g.dims) - 1).astype(np.int64)
    return (c[:, 2] * g.dims[1] + c[:, 1]) * g.dims[0] + c[:, 0]


# ---- 1. degenerate and skewed reference clouds ------------------------------------------------------------------------------------------
def reference_cloud(name):
    rng = np.random.default_rng(101)
    if name == 'planar':
        return np.concatenate([rng.uniform(0.0, 1000.0, (120000, 2)), np.full((120000, 1), 37.5)], 1)
    if name == 'axis_line':
        return np.concatenate([rng.uniform(-300.0, 700.0, (5000, 1)), np.full((5000, 1), 12.25), np.full((5000, 1), -40.5)], 1)
    if name == 'diagonal_line':
        return np.array([10.0, -20.0, 5.0]) + rng.uniform(0.0, 600.0, (5000, 1)) * np.ones(3)
    if name == 'outlier':
        d = rng.normal(size=(5000, 3))
        ball = 100.0 * rng.uniform(0.0, 1.0, (5000, 1)) ** (1.0 / 3.0) * d / np.linalg.norm(d, axis=1)[:, None]
        return np.concatenate([ball, 1e6 * np.array([[0.6, 0.64, 0.48]])])
    if name == 'single':
        return rng.uniform(-50.0, 50.0, (1, 3))
    if name == 'pair':
        return rng.uniform(-50.0, 50.0, (2, 3))
    if name == 'coincident':
        return np.repeat(rng.uniform(-50.0, 50.0, (1, 3)), 300, 0)
    if name == 'slab':
        return rng.uniform(0.0, 1.0, (60000, 3)) * np.array([1000.0, 1000.0, 2.0])
    raise KeyError(name)


def assert_branch(name, ref, g):
    """the branch of make_grid (or the cell layout) the case is named for"""
    n = ref.shape[0]
    occupied = np.bincount(cells_of(g, ref), minlength=int(np.prod(g.dims)))
    print('%s: n %d, h %.6g, dims %s, cap %d, widened %d, clamped %s, floored %s, occupied cells %d of %d'
          % (name, n, g.h, g.dims, g.cap, g.widened, g.clamped, g.floored, (occupied > 0).sum(), occupied.size))
    if name == 'planar':
        assert g.dims[2] == 1 and g.floored[2] and g.widened >= 1
    elif name == 'axis_line':
        assert g.dims == (1025, 1, 1) and g.clamped and g.floored[1] and g.floored[2]
    elif name == 'diagonal_line':
        assert min(g.dims) > 1 and (occupied == 0).mean() > 0.99
    elif name == 'outlier':
        assert min(g.dims) > 1 and occupied.max() == n - 1
    elif name in ('single', 'coincident'):
        assert g.emax == 0.0 and g.h == 1.0 and g.dims == (1, 1, 1)
    elif name == 'pair':
        assert n == 2 and g.emax > 0.0
    elif name == 'slab':
        assert not g.floored.any() and g.dims[2] <= 3 and min(g.dims[:2]) > 100
    else:
        raise KeyError(name)


def queries_for(ref, rng):
    """about 5 000 queries -> (inside the box, outside it on every side, on its faces, edges and corners, copies of reference points)"""
    lo, hi = ref.min(0), ref.max(0)
    diag = float(np.linalg.norm(hi - lo)) or 1.0
    inside = rng.uniform(lo, hi, (1500, 3))
    # outside: each axis below the box, within it or above it, not all three within; the first 26 are every such combination
    side = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)])
    side = np.concatenate([side, side[rng.integers(0, 26, 1500 - 26)]])
    away = rng.uniform(0.0, 10.0, (1500, 1)) ** 2 / 10.0 * diag * rng.uniform(0.05, 1.0, (1500, 3))        # (near the box more often than far)
    outside = np.where(side < 0, lo - away, np.where(side > 0, hi + away, rng.uniform(lo, hi, (1500, 3))))
    # on the box: each axis at its minimum, within, or at its maximum, not all three within; the 8 corners first
    on = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)])
    more = rng.integers(-1, 2, (1000, 3))
    on = np.concatenate([on, more[(more != 0).any(1)]])
    border = np.where(on < 0, lo, np.where(on > 0, hi, rng.uniform(lo, hi, (on.shape[0], 3))))
    pick = rng.integers(0, ref.shape[0], 1000)
    return inside, outside, border, pick


NEAREST_CASES = ['planar', 'axis_line', 'diagonal_line', 'outlier', 'single', 'pair', 'coincident', 'slab']


@pytest.mark.parametrize('where', ['origin', 'offset'])
@pytest.mark.parametrize('name', NEAREST_CASES)
def test_nearest_on_degenerate_reference_clouds(ctx, name, where):
    ref = reference_cloud(name) + (OFFSET if where == 'offset' else 0.0)
    g = grid_of(ref)
    assert_branch(name, ref, g)
    # (the queries' seed is one at which no case has a near tie, which the cap in check_nearest requires of 5 000 queries: 10^4 point
    # spacings from a collinear cloud, two neighbours on the line are equally far to 1e-12 for about one query in 1 500)
    inside, outside, border, pick = queries_for(ref, np.random.default_rng(17))
    assert ((outside < g.lo) | (outside > g.hi)).any(1).all()
    assert ((border == g.lo) | (border == g.hi)).any(1).all()
    assert all((border == np.array(corner)).all(1).any() for corner in itertools.product(*zip(g.lo, g.hi)))
    q = np.concatenate([inside, outside, border, ref[pick]])
    dist, idx, _ = check_nearest(ctx, ref, q, duplicates=name == 'coincident')
    # a query that is a reference point finds it (the first copy of it) at distance 0
    first = 0 if name == 'coincident' else pick
    assert (dist[-pick.size:] == 0).all() and np.array_equal(idx[-pick.size:], np.broadcast_to(first, pick.shape))


# ---- 2. exact ties across cells and rings -----------------------------------------------------------------------------------------------
def brute_force(ref, q, chunk=500):
    """float64 argmin over all reference points; np.argmin names the first minimum, the smallest index -> (dist, idx, how many are as near)"""
    idx, d2, ties = np.empty(q.shape[0], np.int64), np.empty(q.shape[0], np.float64), np.empty(q.shape[0], np.int64)
    for s in range(0, q.shape[0], chunk):
        e = ref[None, :, :] - q[s:s + chunk, None, :]
        d = (e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]) + e[:, :, 2] * e[:, :, 2]
        idx[s:s + chunk] = d.argmin(1)
        d2[s:s + chunk] = d.min(1)
        ties[s:s + chunk] = (d == d2[s:s + chunk, None]).sum(1)
    return np.sqrt(d2), idx, ties


@pytest.mark.parametrize('scale,shift', [(1.0, (0.0, 0.0, 0.0)), (0.75, (4096.0, -2048.0, 512.0))])
def test_exact_ties_go_to_the_smallest_index(ctx, scale, shift):
    """An integer lattice {0..19}^3 in shuffled order, queried at the centres of its cells (8 equally near points), faces (4) and edges
    (2), half a step outside it too.  Every coordinate is dyadic, so every squared distance is exact in float64 in any order of
    summation: the index and the distance must equal a brute-force argmin's, with no allowance for near ties.
    (Without the `r.i < best_i` clause of ev_scan_cells this fails.  With `>=` for the `>` of the ring walk's end it still passes, and
    no input can tell the two apart: the ring's bound and out2 are both taken 1e-9 below their values, so a point of ring r is
    strictly farther than lbd^2 + out2, and with both zero the best distance is zero only for points of the query's own cell.)"""
    rng = np.random.default_rng(53)
    k = np.arange(20.0)
    lattice = np.stack(np.meshgrid(k, k, k, indexing='ij'), -1).reshape(-1, 3)
    lattice = lattice[rng.permutation(lattice.shape[0])]
    half = rng.integers(-1, 20, (6000, 3)) + 0.5               # -0.5 .. 19.5
    whole = rng.integers(0, 20, (6000, 3)).astype(np.float64)
    n_half = np.repeat([3, 2, 1], 2000)                        # cell centres, face centres, edge midpoints
    axes = np.argsort(rng.random((6000, 3)), 1)                # a random choice of which axes are the half-integer ones
    q = np.where(axes < n_half[:, None], half, whole)
    ref, q = scale * lattice + np.array(shift), scale * q + np.array(shift)
    # premises: the tied points lie in different cells (one point per occupied cell); exact arithmetic; ties of every order, some outside
    g = grid_of(ref)
    occupied = np.bincount(cells_of(g, ref))
    print('lattice x %g: h %.6g, dims %s, at most %d points a cell' % (scale, g.h, g.dims, occupied.max()))
    assert occupied.max() == 1 and abs(g.h / scale - 1.0) < 0.1
    assert np.array_equal((ref - np.array(shift)) / scale, lattice) and np.array_equal(ref * 8, np.round(ref * 8))
    dist, idx, ties = brute_force(ref, q)
    e2 = ((ref[None, :200] - q[:, None, :]) ** 2).sum(2)
    assert np.array_equal(e2 * 64, np.round(e2 * 64))          # (sixty-fourths: nothing was rounded)
    out = ((q < g.lo) | (q > g.hi)).any(1)
    print('ties: %s; %d queries outside the lattice' % (dict(zip(*np.unique(ties, return_counts=True))), out.sum()))
    assert all((ties == t).sum() > 1000 for t in (8, 4, 2)) and out.sum() > 500 and (ties[out] >= 2).sum() > 300
    got_dist, got_idx, _ = ctx.nearest(ref, q)
    assert np.array_equal(got_idx, idx)
    assert np.array_equal(_bits(got_dist), _bits(dist))


# ---- 3. launch geometry of the query kernel ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def full_pair(ctx):
    a, b = cloud_pair('off_origin')
    return a, b, ctx.nearest(a, b), ctx.nearest(b, a)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 511, 513])
def test_query_and_reference_counts_around_the_wave_and_the_block(ctx, full_pair, n):
    a, b, ab, ba = full_pair
    # the first n queries: what the full call gave them, the sum of their own squares, the same bits again
    for ref, q, full in ((a, b[:n], ab), (b, a[:n], ba)):
        dist, idx, s = ctx.nearest(ref, q)
        assert np.array_equal(_bits(dist), _bits(full[0][:n])) and np.array_equal(idx, full[1][:n])
        assert np.isclose(s, (dist ** 2).sum(), rtol=1e-12, atol=0)
        again = ctx.nearest(ref, q)
        assert np.array_equal(_bits(dist), _bits(again[0])) and np.array_equal(idx, again[1])
        assert np.float64(s).view(np.uint64) == np.float64(again[2]).view(np.uint64)
    # the roles swapped: n reference points
    for ref, q in ((b[:n], a[:5000]), (a[:n], b[:5000])):
        dist, idx, s = check_nearest(ctx, ref, q)
        again = ctx.nearest(ref, q)
        assert np.array_equal(_bits(dist), _bits(again[0])) and np.array_equal(idx, again[1])
        assert np.float64(s).view(np.uint64) == np.float64(again[2]).view(np.uint64)


# ---- 4. the shared scan at its edges, through the sampler -------------------------------------------------------------------------------
@pytest.mark.parametrize('nf', [1, 2047, 2048, 2049, 4096, 4097])
def test_sampler_with_face_counts_around_the_scan_tile(ctx, nf):
    v, f = icosphere(4, 100.0)
    f, dx = f[:nf], 1.5
    counts = E.node_counts(Duck(v, f), dx)
    print('%d faces: %d to %d nodes a face, %d nodes' % (nf, counts.min(), counts.max(), counts.sum()))
    assert counts.shape == (nf,) and counts.min() >= 20 and counts.max() < 100
    assert nf == 1 or counts.sum() > 4 * TILE                 # (the scan of the nodes' flags takes several tiles)
    dev, face = check_samples(ctx, v, f, dx)
    assert dev.shape[0] > 0.2 * counts.sum() and (nf == 1 or face.max() == nf - 1)


def test_sampler_with_more_nodes_than_one_chunk_of_tile_sums(ctx):
    v, f = icosphere(4, 100.0)
    dx = 0.36
    n_nodes = int(E.node_counts(Duck(v, f), dx).sum())
    print('%d nodes = 2^21 + %d' % (n_nodes, n_nodes - CHUNK))
    assert CHUNK + TILE < n_nodes < 1.1 * CHUNK                # more than 1025 tiles, and not much more
    dev, face = check_samples(ctx, v, f, dx)
    assert dev.shape[0] > 0.2 * n_nodes and face.max() == len(f) - 1


# ---- 5. meshes that stress the bisection of the node offsets and the counts --------------------------------------------------------------
@pytest.mark.parametrize('name', EDGE_MESHES)
def test_sampler_on_the_edge_meshes(ctx, name):
    runs = edge_mesh(name)
    counts = edge_mesh_premise(name, runs)
    total = 0
    for (v, f, dx), c in zip(runs, counts):
        dev, face = check_samples(ctx, v, f, dx)
        assert (c[face] > 0).all()
        total += dev.shape[0]
    print('%s: %s nodes, %d samples' % (name, [int(c.sum()) for c in counts], total))
    assert total > 100
