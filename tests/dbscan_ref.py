"""
The DBSCAN query of include/nw_clustering.h restated in NumPy: brute force over all pairs in row blocks, no grid, no shortcut, a plain
sequential union.  tests/test_dbscan_ref.py ties it to scikit-learn and to closed forms; the compiled core and the device are asked for
its arrays bit for bit.

    d2(i, j)  = (ex*ex + ey*ey) + ez*ez in float64, e = (double)p_j - (double)p_i      (NumPy multiplies and adds separately: no fma)
    near      = d2 <= eps*eps          count = min(#near, count_cap)          core = #near >= min_points
    clusters  = components of the core points under near, numbered by their smallest index
    anchor    = itself for a core point; for another point the core point near it with the smallest (d2, index); else -1
    label     = the anchor's cluster, or -1

`mutate` breaks one rule on purpose (the tests show that they notice): 'strict' compares with < instead of <=, 'no_self' does not count
the point itself, 'border_index' gives a border point to the smallest-index core point near it instead of the nearest.
"""
import numpy as np

BLOCK = 512


def cloud32(points):
    return np.ascontiguousarray(points, np.float32).reshape(-1, 3)


def d2_rows(P64, rows):
    """d2(i, j) for i in rows, all j: (len(rows), n) float64"""
    e = P64[None, :, :] - P64[rows][:, None, :]
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def min_margin(points, eps):
    """min over all pairs of |d2 - eps2| / eps2: scikit-learn compares a rooted distance with eps, so a comparison with it needs a margin"""
    P = cloud32(points).astype(np.float64)
    eps2 = float(eps) * float(eps)
    m = np.inf
    for s in range(0, len(P), BLOCK):
        m = min(m, float(np.abs(d2_rows(P, np.arange(s, min(len(P), s + BLOCK))) - eps2).min()))
    return m / eps2


def dbscan(points, eps, min_points, count_cap=None, mutate=None):
    P32 = cloud32(points)
    P = P32.astype(np.float64)
    n = len(P)
    eps2 = float(eps) * float(eps)
    cap = int(min_points) if count_cap is None else int(count_cap)
    near_of = (lambda d2: d2 < eps2) if mutate == 'strict' else (lambda d2: d2 <= eps2)
    n_eps = np.zeros(n, np.int64)
    for s in range(0, n, BLOCK):
        rows = np.arange(s, min(n, s + BLOCK))
        n_eps[rows] = near_of(d2_rows(P, rows)).sum(1)
    if mutate == 'no_self':
        n_eps -= 1
    core = n_eps >= int(min_points)
    count = np.minimum(n_eps, cap).astype(np.int32)
    # the sequential union over the core points' edges, each from its larger end: comp[i] = the smallest index of i's component so far
    comp = np.arange(n)
    anchor = np.where(core, np.arange(n), -1).astype(np.int32)
    for s in range(0, n, BLOCK):
        rows = np.arange(s, min(n, s + BLOCK))
        d2 = d2_rows(P, rows)
        near = near_of(d2)
        for k, i in enumerate(rows):
            js = np.nonzero(near[k] & core)[0]
            if core[i]:
                ids = np.unique(comp[js[js <= i]])                # (i itself is among them)
                if len(ids) > 1:
                    comp[np.isin(comp, ids)] = ids[0]
            elif len(js):
                if mutate == 'border_index':
                    anchor[i] = js.min()
                else:
                    dj = d2[k, js]
                    anchor[i] = js[dj == dj.min()].min()
    root = np.where(core, comp, -1).astype(np.int64)
    roots = np.unique(root[root >= 0])                            # ascending: numbered by the smallest index
    rank = np.full(n + 1, -1, np.int64)
    rank[roots] = np.arange(len(roots))
    labels = np.where(anchor >= 0, rank[root[np.maximum(anchor, 0)]], -1).astype(np.int32)
    C = len(roots)
    sizes, n_core, first, bbox = np.zeros(C, np.int64), np.zeros(C, np.int64), np.zeros(C, np.int32), np.zeros((C, 6), np.float32)
    for c in range(C):
        m = labels == c
        sizes[c], n_core[c], first[c] = m.sum(), (m & core).sum(), np.nonzero(m & core)[0].min()
        bbox[c, :3], bbox[c, 3:] = P32[m].min(0), P32[m].max(0)
    return dict(labels=labels, anchor=anchor, count=count, core=core, n_eps=n_eps, n_clusters=C, sizes=sizes, n_core=n_core, first=first, bbox=bbox,
                info=dict(n_core=int(core.sum()), n_border=int((~core & (labels >= 0)).sum()), n_noise=int((labels < 0).sum()), n_clusters=C))


def same_as_restatement(mine, ref):
    """every output of `mine` (the compiled core's or the device's) is the restatement's, bit for bit"""
    for k in ('labels', 'anchor', 'count'):
        assert mine[k].dtype == np.int32 and np.array_equal(mine[k], ref[k]), k
    assert np.array_equal(np.asarray(mine['core'], bool), ref['core'])
    assert mine['n_clusters'] == ref['n_clusters']
    for k in ('sizes', 'n_core', 'first'):
        assert np.array_equal(mine[k], ref[k]), k
    assert mine['bbox'].dtype == np.float32 and mine['bbox'].tobytes() == ref['bbox'].tobytes()
    for k in ('n_core', 'n_border', 'n_noise', 'n_clusters'):
        assert mine['info'][k] == ref['info'][k], k


def partition(labels, mask=None):
    """the clusters as a set of frozensets of indices (over the points of `mask`)"""
    labels = np.asarray(labels)
    idx = np.arange(len(labels)) if mask is None else np.nonzero(mask)[0]
    out = {}
    for i in idx:
        if labels[i] >= 0:
            out.setdefault(int(labels[i]), []).append(int(i))
    return set(frozenset(v) for v in out.values())


# ---- clouds ------------------------------------------------------------------------------------------------------------------------------
def lattice(m, spacing=1.0):
    """the m x m x m integer lattice, x fastest"""
    g = np.arange(m, dtype=np.float32) * np.float32(spacing)
    z, y, x = np.meshgrid(g, g, g, indexing='ij')
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)


def chain(n, step, wider=False):
    """n points along x, `step` apart (an exact float32 and small integers of it exact too), or one ulp of the step wider"""
    s = np.float32(step)
    if wider:
        s = np.nextafter(s, np.float32(np.inf))
    P = np.zeros((n, 3), np.float32)
    P[:, 0] = np.arange(n, dtype=np.float32) * s
    # (every gap must be the step itself: a step of 1 + 2^-23 is exact up to 2 steps only, so the wider chain is a short one; for a long
    # chain "one ulp beside" is an eps one float64 ulp below the step)
    assert np.all(np.diff(P[:, 0].astype(np.float64)) == float(s))
    return P


def bridge():
    """two 3 x 3 x 3 unit lattices, 4 apart along x (x = 0..2 and 6..8), and one point at (4, 1, 1): exactly 2 from the core (2, 1, 1) of
    the first and from the core (6, 1, 1) of the second, and further from every other point.  The bridge comes last."""
    A = lattice(3)
    B = A + np.array([6.0, 0.0, 0.0], np.float32)
    return np.concatenate([A, B, np.array([[4.0, 1.0, 1.0]], np.float32)]).astype(np.float32)


def two_vesicles(seed, n_each=1500, n_background=300, R=100.0, gap=400.0, sigma=5.0):
    """two spheres of radius R with centres `gap` apart along x, n_each points on each with N(0, sigma^2) added per axis, and n_background
    uniform points in the cloud's box scaled by 1.2 about its centre -> (float32 cloud, source: 0 / 1 the sphere, 2 background)"""
    rng = np.random.default_rng(seed)
    parts, src = [], []
    for s in range(2):
        u = rng.normal(size=(n_each, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        parts.append(u * R + np.array([s * gap, 0.0, 0.0]) + rng.normal(0.0, sigma, (n_each, 3)))
        src.append(np.full(n_each, s))
    P = np.concatenate(parts)
    lo, hi = P.min(0), P.max(0)
    c, half = 0.5 * (lo + hi), 0.6 * (hi - lo)
    parts.append(rng.uniform(c - half, c + half, (n_background, 3)))
    src.append(np.full(n_background, 2))
    return np.concatenate(parts).astype(np.float32), np.concatenate(src)
