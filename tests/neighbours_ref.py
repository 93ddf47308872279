"""
NumPy restatement of include/nw_neighbours.h by brute force: the yardstick the k-th-neighbour kernels are compared with bit for bit
(tests/test_hip_neighbours.py) and that is itself checked against scipy's cKDTree and on the topology of its level sets
(tests/test_neighbours.py).  Every distance to every point, chunked over the queries, in the header's expressions:

    d2(x, p) = (ex*ex + ey*ey) + ez*ez in float64, e = (double)p - x;  r_k = sqrt(k-th smallest d2);  result = min(r_k, r_cap)
    node (i, j, k) at (double)lo + ((double)index + 0.5) * (double)h;  field = uint64(floor((r_cap - result) * 2^20)), [z, y, x]

and ch_shrinkwrap_amd.isosurface.knn_isosurface's chain on top of them, with isosurface_ref.surface_nets as the mesher.  It also holds
the inputs of both test modules, each seeded.
"""
import functools

import numpy as np

import isosurface_ref as IR

MAX_K = 32
CHUNK = 1 << 22                                                      # distances in flight


def dist2(points, x):
    """(len(x), len(points)) float64: the squared distance of every float32 point from every float64 position"""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    x = np.asarray(x, np.float64).reshape(-1, 3)
    ex, ey, ez = (p[None, :, a] - x[:, None, a] for a in range(3))
    return (ex * ex + ey * ey) + ez * ez


def kth_at(points, x, k, r_cap=np.inf):
    """min(r_k, r_cap) at the float64 positions x"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    x = np.asarray(x, np.float64).reshape(-1, 3)
    k = int(k)
    assert 1 <= k <= MAX_K and r_cap > 0
    out = np.full(x.shape[0], np.inf)
    if p.shape[0] >= k:
        step = max(1, CHUNK // p.shape[0])
        for s in range(0, x.shape[0], step):
            d2 = dist2(p, x[s:s + step])
            out[s:s + step] = np.sqrt(np.partition(d2, k - 1, axis=1)[:, k - 1])
    return np.minimum(out, float(r_cap))


def kth_distance(points, queries, k, r_cap=np.inf):
    """min(r_k, r_cap) at float32 queries"""
    return kth_at(points, np.asarray(queries, np.float32).reshape(-1, 3).astype(np.float64), k, r_cap)


def node_positions(lo, h, dims):
    """(nz * ny * nx, 3) float64, x fastest"""
    lo = np.asarray(lo, np.float32).reshape(3).astype(np.float64)
    h = float(np.float32(h))
    ax = [lo[a] + (np.arange(int(dims[a]), dtype=np.float64) + 0.5) * h for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing='ij')
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1)


def quantise(r, r_cap):
    return np.floor((float(r_cap) - np.asarray(r, np.float64)) * 1048576.0).astype(np.uint64)


def node_field(points, lo, h, dims, k, r_cap):
    """uint64 [z, y, x]"""
    assert np.isfinite(r_cap) and r_cap <= 2.0 ** 40
    r = kth_at(points, node_positions(lo, h, dims), k, r_cap)
    return quantise(r, r_cap).reshape(int(dims[2]), int(dims[1]), int(dims[0]))


def local_density(points, k):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    if p.shape[0] <= k:
        raise ValueError('no k-th neighbour')
    r = kth_distance(p, p, k + 1)
    with np.errstate(divide='ignore'):
        return float(k) / ((4.0 / 3.0 * np.pi) * (r * r * r))


def knn_threshold(h, k, threshold_density):
    """(R_thr, r_cap, pad, thr)"""
    R_thr = float(np.cbrt(3.0 * int(k) / (4.0 * np.pi * float(threshold_density))))
    r_cap = R_thr + 2.0 * float(h)
    return R_thr, r_cap, int(np.ceil(R_thr / float(h))) + 2, int(np.floor((r_cap - R_thr) * float(1 << 20)))


def knn_isosurface(points, h, k=20, threshold_density=None, fraction=0.3):
    """(vertices, faces, keys, info): the whole chain with the package's grid rule"""
    from ch_shrinkwrap_amd.isosurface import grid_for
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    h = float(np.float32(h))
    median = None
    if threshold_density is None:
        median = float(np.median(local_density(p, k)))
        threshold_density = float(fraction) * median
    R_thr, r_cap, pad, thr = knn_threshold(h, k, threshold_density)
    lo, dims = grid_for(p, h, pad)
    field = node_field(p, lo, h, dims, k, r_cap)
    v, f, keys = IR.surface_nets(field, thr, lo, h)
    return v, f, keys, dict(lo=lo, h=h, dims=dims, pad=pad, thr=thr, R_thr=R_thr, r_cap=r_cap, threshold_density=float(threshold_density),
                            median_density=median, field=field)


def outer_component(v, f):
    """(Euler characteristic, signed volume) of the component of the largest volume"""
    comps = IR.components(v, f)
    _, chi, vol = max(comps, key=lambda c: c[2])
    return chi, vol


# ---- the list of the k best (csrc/nw_neighbours_core.h: nwk_list_insert) -----------------------------------------------------------------
def list_trace(d2, k):
    """The list after every insertion of the stream d2: (slots (n, k) with nan in unused slots, cnt (n,), at (n,), mx (n,))"""
    s = np.full(k, np.nan)
    cnt, at, mx = 0, 0, -1.0
    rows, cnts, ats, mxs = [], [], [], []
    for v in np.asarray(d2, np.float64):
        if cnt < k:
            s[cnt] = v
            if cnt == 0 or v > mx:
                mx, at = v, cnt
            cnt += 1
        elif v < mx:
            s[at] = v
            at = int(np.argmax(s))                                   # (the first of equal maxima, as the ascending rescan with > finds)
            mx = float(s[at])
        rows.append(s.copy()); cnts.append(cnt); ats.append(at); mxs.append(mx)
    return np.array(rows), np.array(cnts), np.array(ats), np.array(mxs)


# ---- inputs, each seeded -----------------------------------------------------------------------------------------------------------------
def sphere_cloud(n, seed, R=100.0, sigma=10.0):
    """n localizations on a sphere of radius R, each displaced by an isotropic Gaussian of width sigma"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return (R * d + rng.normal(scale=sigma, size=(n, 3))).astype(np.float32)


def torus_cloud(n, seed, R=100.0, r=30.0, sigma=5.0):
    """n localizations on a torus (uniform in both angles), each displaced by an isotropic Gaussian of width sigma"""
    rng = np.random.default_rng(seed)
    u, w = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    p = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], 1)
    return (p + rng.normal(scale=sigma, size=(n, 3))).astype(np.float32)


# seeds at which the restatement's knn_isosurface alone shows the topology tests/test_neighbours.py asserts (checked when they were chosen)
TOPOLOGY_CASES = {('sphere', 300): 1, ('sphere', 1000): 1, ('sphere', 5000): 1, ('torus', 300): 2, ('torus', 1000): 1, ('torus', 5000): 1}
TOPOLOGY_H = {'sphere': 10.0, 'torus': 8.0}


@functools.lru_cache(maxsize=None)
def topology_cloud(shape, n):
    return (sphere_cloud if shape == 'sphere' else torus_cloud)(n, TOPOLOGY_CASES[(shape, n)])


@functools.lru_cache(maxsize=None)
def topology_reference(shape, n):
    """knn_isosurface of the restatement at the issue's settings: k = 20, 0.3 x the median local density, fixed voxels"""
    return knn_isosurface(topology_cloud(shape, n), TOPOLOGY_H[shape], 20, None, 0.3)


def random_cloud(n, seed, scale=100.0, offset=(5e3, -3e3, 1e3)):
    rng = np.random.default_rng(seed)
    return (np.asarray(offset)[None, :] + rng.normal(scale=scale, size=(n, 3))).astype(np.float32)


def queries_around(points, n, seed, spread=1.5):
    """n float32 queries in the cloud's box blown up by `spread`, the first few being cloud points themselves"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    c, e = (p.max(0) + p.min(0)) / 2, np.maximum((p.max(0) - p.min(0)) / 2, 1.0)
    q = (c[None, :] + rng.uniform(-spread, spread, size=(n, 3)) * e[None, :]).astype(np.float32)
    m = min(n // 4, p.shape[0])
    q[:m] = p[rng.permutation(p.shape[0])[:m]]
    return q


def lattice_case(m=7, seed=3):
    """(points, queries): the integer lattice 0..m-1 cubed, shuffled, queried at the centres of its cells, faces and edges, where 8, 4
    and 2 points tie for the nearest in exact arithmetic (and more further out)"""
    g = np.arange(m, dtype=np.float64)
    pts = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    np.random.default_rng(seed).shuffle(pts, axis=0)
    c = np.stack(np.meshgrid(g[:-1], g[:-1], g[:-1], indexing='ij'), -1).reshape(-1, 3)
    q = np.concatenate([c + [0.5, 0.5, 0.5], c + [0.5, 0.5, 0.0], c + [0.0, 0.5, 0.5], c + [0.5, 0.0, 0.0], c + [0.0, 0.0, 0.5]])
    return pts.astype(np.float32), q.astype(np.float32)


def copies_case(n=300):
    """(points, queries): n copies of one point; queried at the point and beside it"""
    p = np.tile(np.array([[12.5, -7.25, 3.0]], np.float32), (n, 1))
    q = np.array([[12.5, -7.25, 3.0], [13.5, -7.25, 3.0], [0.0, 0.0, 0.0]], np.float32)
    return p, q


def flat_case(kind, n=500, seed=4):
    """(points, queries): a cloud on a plane (z constant), on an axis (y and z constant) or on the space diagonal of a cube"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-50.0, 50.0, size=(n, 3))
    if kind == 'plane':
        p[:, 2] = 7.0
    elif kind == 'axis':
        p[:, 1], p[:, 2] = -3.0, 7.0
    elif kind == 'diagonal':
        p[:, 1] = p[:, 2] = p[:, 0]
    else:
        raise ValueError(kind)
    p = p.astype(np.float32)
    q = np.concatenate([p[:40], (p[:80].astype(np.float64) + rng.normal(scale=5.0, size=(80, 3))).astype(np.float32)])
    return p, q


def far_case(seed=5):
    """(points, queries): queries ten box diagonals outside the cloud's box, along the axes and along a diagonal"""
    p = random_cloud(400, seed, scale=20.0, offset=(0.0, 0.0, 0.0))
    diag = float(np.linalg.norm(p.max(0).astype(np.float64) - p.min(0)))
    d = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1], [1, 1, 1], [-1, 1, -1]], np.float64)
    d /= np.linalg.norm(d, axis=1)[:, None]
    c = (p.max(0).astype(np.float64) + p.min(0)) / 2
    return p, (c[None, :] + d * 10.5 * diag).astype(np.float32), diag


def cap_case(where, seed=6):
    """(points, query, k, r_cap): nineteen points within 1 nm of the query at the origin and the twentieth on the x axis at x = 40, plus
    far points that fill the box.  r_cap is chosen so that the twentieth lies at 0.999 r_cap ('below'), at exactly r_cap ('at') or at
    1.001 r_cap ('above'): where the walk's stopping rule and the cap meet."""
    rng = np.random.default_rng(seed)
    near = rng.normal(size=(19, 3))
    near *= (rng.uniform(0.1, 0.9, size=19) / np.linalg.norm(near, axis=1))[:, None]
    far = rng.uniform(-400.0, 400.0, size=(200, 3))
    far = far[np.linalg.norm(far, axis=1) > 80.0]
    p = np.concatenate([near, [[40.0, 0.0, 0.0]], far]).astype(np.float32)
    p = p[rng.permutation(p.shape[0])]
    r_cap = {'below': 40.0 / 0.999, 'at': 40.0, 'above': 40.0 / 1.001}[where]
    return p, np.zeros((1, 3), np.float32), 20, r_cap


NODE_GRIDS = {'3x3x3': (3, 3, 3), '3x5x70': (3, 5, 70), '70x3x5': (70, 3, 5)}


def node_case(name, seed=8):
    """(points, lo, h, dims): five localizations a voxel strewn over a small lattice of h = 7.3 off the origin (r_3 is about 3.8 nm and
    r_20 about 7.2 nm), one of them as near a node as float32 allows"""
    dims = np.array(NODE_GRIDS[name], np.int32)
    lo, h = np.array([5e3, -3e3, 1e3], np.float32), np.float32(7.3)
    rng = np.random.default_rng(seed)
    p = (lo.astype(np.float64)[None, :] + rng.uniform(0.0, 1.0, size=(5 * int(dims.prod()), 3)) * dims[None, :] * float(h)).astype(np.float32)
    p[0] = on_node(lo, h, dims // 2)
    return p, lo, float(h), dims


def on_node(lo, h, index):
    """The float32 point nearest to node `index`; it coincides with the node when the node's float64 coordinates are float32 numbers"""
    lo = np.asarray(lo, np.float32).astype(np.float64)
    return (lo + (np.asarray(index, np.float64) + 0.5) * float(np.float32(h))).astype(np.float32)


def coincident_node_case():
    """(points, lo, h, dims, index): lo and h dyadic, so that node `index` is a float32 point, and a localization exactly there"""
    lo, h, dims, index = np.array([-16.0, 8.0, 0.0], np.float32), 2.0, np.array([9, 8, 7], np.int32), np.array([4, 3, 5])
    rng = np.random.default_rng(9)
    p = (lo.astype(np.float64)[None, :] + rng.uniform(0.0, 1.0, size=(60, 3)) * dims[None, :] * h).astype(np.float32)
    p[17] = on_node(lo, h, index)
    return p, lo, h, dims, index
