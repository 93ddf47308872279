"""
The pair-count query of include/nw_pairs.h restated in NumPy: brute force over all pairs in row blocks, no grid, np.searchsorted for the
bin.  tests/test_pair_counts_ref.py ties it to closed forms and to scipy's cKDTree.count_neighbors; the compiled core and the device
are asked for its arrays bit for bit.

    e2[b]     = r_b * r_b in float64
    d2(i, j)  = (ex*ex + ey*ey) + ez*ez in float64, e = (double)cloud_j - (double)query_i   (NumPy multiplies and adds separately: no fma)
    bin       = #{ b : e2[b] < d2 } = np.searchsorted(e2, d2, 'left'); a pair with bin m is not counted
    auto      : the queries are the cloud, (i, i) is left out by index; every unordered pair counts twice
    cross     : every (query, cloud point)
    local     = (n_queries, m) uint32 counts per query; hist = local.sum(0) as uint64; cumulative = hist.cumsum()

`mutate` breaks one rule on purpose (the tests show that they notice): 'closed_left' puts a pair at exactly an edge into the next bin
(<= for <), 'keep_self' counts (i, i), 'unordered' counts every unordered pair once (j > i).
"""
import numpy as np

BLOCK = 512
MAX_BINS = 64


def cloud32(points):
    return np.ascontiguousarray(points, np.float32).reshape(-1, 3)


def edges2(radii):
    """the squared edges, checked as nwq_edges checks them"""
    r = np.ascontiguousarray(radii, np.float64).reshape(-1)
    if not (1 <= len(r) <= MAX_BINS) or not np.isfinite(r).all() or (r < 0).any() or (r > 2.0 ** 40).any():
        raise ValueError('radii')
    e2 = r * r
    if (np.diff(e2) <= 0).any():
        raise ValueError('radii')
    return e2


def d2_rows(Q64, P64):
    """d2(i, j) for every query i and cloud point j: (len(Q64), len(P64)) float64"""
    e = P64[None, :, :] - Q64[:, None, :]
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def pair_counts(points, radii, other=None, mutate=None):
    """-> dict(hist (m,) uint64, cumulative (m,) uint64, local (n_queries, m) uint32, n_queries, n_cloud).  other = None: auto mode on
    `points`; else the queries `points` against the cloud `other`."""
    e2 = edges2(radii)
    m = len(e2)
    Q = cloud32(points).astype(np.float64)
    auto = other is None
    P = Q if auto else cloud32(other).astype(np.float64)
    nq, n = len(Q), len(P)
    local = np.zeros((nq, m), np.uint32)
    cols = np.arange(n)
    for s in range(0, nq, BLOCK):
        rows = np.arange(s, min(nq, s + BLOCK))
        d2 = d2_rows(Q[rows], P)
        bins = np.searchsorted(e2, d2.ravel(), 'right' if mutate == 'closed_left' else 'left').reshape(d2.shape)
        if auto and mutate != 'keep_self':
            bins[rows - s, rows] = m                              # (i, i) by index
        if auto and mutate == 'unordered':
            bins[cols[None, :] <= rows[:, None]] = m
        flat = (bins + (np.arange(len(rows)) * (m + 1))[:, None]).ravel()              # one bincount for the block: row k's bins at k (m + 1) + bin
        local[rows] = np.bincount(flat, minlength=len(rows) * (m + 1)).reshape(len(rows), m + 1)[:, :m]
    hist = local.sum(0, dtype=np.uint64)
    return dict(hist=hist, cumulative=np.cumsum(hist, dtype=np.uint64), local=local, n_queries=nq, n_cloud=n)


def min_edge_margin(points, radii, other=None):
    """min over all pairs and edges of |d2 - e2[b]| / e2[b] (edges at 0 aside): a comparison with a library that roots the distance
    needs a margin"""
    e2 = edges2(radii)
    e2 = e2[e2 > 0]
    Q = cloud32(points).astype(np.float64)
    P = Q if other is None else cloud32(other).astype(np.float64)
    best = np.inf
    for s in range(0, len(Q), BLOCK):
        d2 = d2_rows(Q[s:s + BLOCK], P)
        for e in e2:
            best = min(best, float(np.abs(d2 - e).min()) / e)
    return best


def lattice(k, step=1.0):
    """the k^3 integer lattice, scaled"""
    g = np.arange(k, dtype=np.float64) * step
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)


def clustered(n, seed, offset=0.0):
    """three blobs and a uniform background"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 3, n)[:, None] * np.array([[25.0, 8.0, -5.0]])
    P = c + rng.normal(0.0, 2.5, (n, 3))
    far = rng.random(n) < 0.2
    P[far] = rng.uniform(-20.0, 70.0, (int(far.sum()), 3))
    return (P + offset).astype(np.float32)


def same_as_restatement(mine, ref, local=True):
    assert mine['hist'].dtype == np.uint64 and np.array_equal(mine['hist'], ref['hist'])
    assert np.array_equal(mine['cumulative'], ref['cumulative'])
    assert mine['n_queries'] == ref['n_queries'] and mine['n_cloud'] == ref['n_cloud']
    if local:
        assert mine['local'].dtype == np.uint32 and mine['local'].shape == ref['local'].shape and np.array_equal(mine['local'], ref['local'])
        assert np.array_equal(mine['local'].sum(0, dtype=np.uint64), mine['hist'])
