"""
The geodesic graph distance of csrc/nw_geodesic_core.h, restated in NumPy with no tricks: the arcs straight from the definition (edge
weights, the diagonal rule with its canonical orientation), D computed twice -- a heapq Dijkstra and a vectorised Bellman-Ford
(np.minimum.at until nothing changes) -- and asserted equal bit for bit, labels from the fixed-point rule.  All float64 on the float32
positions; NumPy's elementwise arithmetic neither contracts nor reorders, and its sqrt is correctly rounded.

The three keyword switches of `arcs` and `labels` (crossing_inclusive, keep_flat, any_arc) are one-line mutations of the definition that
tests/test_mesh_geodesic_ref.py shows to be caught; nothing else sets them.
"""
import heapq

import numpy as np

NONE = np.iinfo(np.int32).max


def mesh32(vertices, faces):
    return np.ascontiguousarray(vertices, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)


def twins(faces):
    """twin[3f+k] of the half-edge faces[f][k] -> faces[f][(k+1)%3], -1 on a border; raises on an edge that is not shared by exactly two
    opposite half-edges"""
    F = np.asarray(faces).reshape(-1, 3)
    seen = {}
    for h in range(3 * F.shape[0]):
        key = (int(F[h // 3, h % 3]), int(F[h // 3, (h + 1) % 3]))
        if key in seen:
            raise ValueError('non-manifold: the half-edge %r appears twice' % (key,))
        seen[key] = h
    twin = np.full(3 * F.shape[0], -1, np.int32)
    for (u, v), h in seen.items():
        twin[h] = seen.get((v, u), -1)
    return twin


def _len2(e):
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


def _unfold(P, a, e, L, c):
    p = P[c] - P[a]
    cr = np.stack([p[:, 1] * e[:, 2] - p[:, 2] * e[:, 1], p[:, 2] * e[:, 0] - p[:, 0] * e[:, 2], p[:, 0] * e[:, 1] - p[:, 1] * e[:, 0]], 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return ((p[:, 0] * e[:, 0] + p[:, 1] * e[:, 1]) + p[:, 2] * e[:, 2]) / L, np.sqrt(_len2(cr)) / L


def diagonals(vertices, faces, twin, crossing_inclusive=False, keep_flat=False):
    """(c, d, weight) of the diagonals that exist: one per interior edge at most, computed in the canonical orientation"""
    V, F = mesh32(vertices, faces)
    P = V.astype(np.float64)
    h = np.arange(3 * F.shape[0])
    t = np.asarray(twin, np.int64)
    u, v = F.reshape(-1)[h], F[h // 3, (h + 1) % 3]
    own = (t >= 0) & ((u < v) | ((u == v) & (h < t)))
    h, t = h[own], t[own]
    a, b = F[h // 3, h % 3], F[h // 3, (h + 1) % 3]
    c, d = F[h // 3, (h + 2) % 3], F[t // 3, (t + 2) % 3]
    e = P[b] - P[a]
    L = np.sqrt(_len2(e))
    xc, yc = _unfold(P, a, e, L, c)
    xd, yd = _unfold(P, a, e, L, d)
    dx, sy = xd - xc, yc + yd
    with np.errstate(invalid='ignore', divide='ignore'):
        xs = xc + dx * yc / sy
        w = np.sqrt(dx * dx + sy * sy)
    if keep_flat:                                             # MUTATION: a face without a height keeps its diagonal
        ok = (L > 0) & (yc >= 0) & (yd >= 0) & (sy > 0)
    else:
        ok = (L > 0) & (yc > 0) & (yd > 0)
    if crossing_inclusive:                                    # MUTATION: <= in the crossing test
        ok &= (xs >= 0) & (xs <= L)
    else:
        ok &= (xs > 0) & (xs < L)
    return c[ok], d[ok], w[ok]


def arcs(vertices, faces, use_diagonals=True, twin=None, **mutation):
    """(tail, head, weight) of every directed arc: each half-edge's edge in both directions, and each diagonal in both directions"""
    V, F = mesh32(vertices, faces)
    P = V.astype(np.float64)
    u, v = F.reshape(-1), F[:, [1, 2, 0]].reshape(-1)
    w = np.sqrt(_len2(P[u] - P[v]))
    tail, head, weight = [u, v], [v, u], [w, w]
    if use_diagonals:
        c, d, wd = diagonals(V, F, twins(F) if twin is None else twin, **mutation)
        tail += [c, d]
        head += [d, c]
        weight += [wd, wd]
    return np.concatenate(tail).astype(np.int64), np.concatenate(head).astype(np.int64), np.concatenate(weight)


def _sources(ids, d0):
    ids = np.asarray(ids, np.int64).reshape(-1)
    d0 = np.zeros(ids.size) if d0 is None else np.asarray(d0, np.float64).reshape(-1) + 0.0
    assert ids.size >= 1 and d0.shape == ids.shape and (d0 >= 0).all() and np.isfinite(d0).all()
    return ids, d0


def dijkstra(n, A, ids, d0, cap=np.inf):
    tail, head, w = A
    order = np.argsort(tail, kind='stable')
    start = np.searchsorted(tail[order], np.arange(n + 1))
    hd, wt = head[order], w[order]
    D = np.full(n, np.inf)
    heap = []
    for i, x in zip(ids.tolist(), d0.tolist()):
        if x < D[i]:
            D[i] = x
            heapq.heappush(heap, (x, i))
    while heap:
        x, i = heapq.heappop(heap)
        if x > D[i] or x > cap:
            continue
        for k in range(start[i], start[i + 1]):
            y = np.float64(x) + wt[k]
            j = hd[k]
            if y < D[j]:
                D[j] = y
                heapq.heappush(heap, (float(y), int(j)))
    return D


def bellman_ford(n, A, ids, d0, cap=np.inf):
    tail, head, w = A
    D = np.full(n, np.inf)
    np.minimum.at(D, ids, d0)
    rounds = 0
    while True:
        go = D[tail] <= cap
        new = D.copy()
        np.minimum.at(new, head[go], D[tail[go]] + w[go])
        if (new.view(np.uint64) == D.view(np.uint64)).all():
            return D, rounds
        D = new
        rounds += 1


def labels(n, A, D, ids, d0, cap=np.inf, any_arc=False):
    """the label rule on the final D (before the cap is applied to it)"""
    tail, head, w = A
    S = np.full(n, NONE, np.int64)
    own = d0 == D[ids]
    np.minimum.at(S, ids[own], np.arange(ids.size)[own])
    if any_arc:                                               # MUTATION: the label comes along any arc from a labelled vertex
        tight = (D[tail] <= cap) & (D[head] < np.inf)
    else:
        tight = (D[tail] <= cap) & (D[tail] + w == D[head]) & (D[head] < np.inf)
    t, h = tail[tight], head[tight]
    while True:
        new = S.copy()
        np.minimum.at(new, h, S[t])
        if (new == S).all():
            return S
        S = new


def geodesic(vertices, faces, sources, d0=None, max_distance=np.inf, diagonals=True, twin=None, want_labels=True, **mutation):
    """dict(distance (V,) float64, source (V,) int32 or None, D (before the cap), arcs, bf_rounds): the restatement of
    geodesic.geodesic_distance"""
    V, F = mesh32(vertices, faces)
    n = V.shape[0]
    any_arc = mutation.pop('any_arc', False)
    A = arcs(V, F, diagonals, twin, **mutation)
    ids, start = _sources(np.flatnonzero(sources) if np.asarray(sources).dtype == np.bool_ else sources, d0)
    cap = float(max_distance)
    assert cap > 0
    D, rounds = bellman_ford(n, A, ids, start, cap)
    D2 = dijkstra(n, A, ids, start, cap)
    assert (D.view(np.uint64) == D2.view(np.uint64)).all(), 'Dijkstra and Bellman-Ford disagree'
    in_band = (D <= cap) & (D < np.inf)
    out = dict(distance=np.where(in_band, D, np.inf), source=None, D=D, arcs=A, bf_rounds=rounds)
    if want_labels:
        S = labels(n, A, D, ids, start, cap, any_arc=any_arc)
        out['source'] = np.where(in_band & (S != NONE), S, -1).astype(np.int32)
    return out


# ---- meshes the tests share ---------------------------------------------------------------------------------------------------------------
def grid_mesh(nx, ny, dx=1.0, dy=1.0, flip=False):
    """(nx x ny) vertices on a flat lattice, two faces per square; the squares' own diagonal runs from (i, j) to (i+1, j+1), with
    flip from (i+1, j) to (i, j+1).  Vertex (i, j) has the id j * nx + i."""
    x, y = np.meshgrid(np.arange(nx) * dx, np.arange(ny) * dy)
    V = np.stack([x.ravel(), y.ravel(), np.zeros(nx * ny)], 1).astype(np.float32)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1))
    a = (j * nx + i).ravel()
    b, c, d = a + 1, a + nx + 1, a + nx
    if flip:
        F = np.concatenate([np.stack([a, b, d], 1), np.stack([b, c, d], 1)])
    else:
        F = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    return V, F.astype(np.int32)


def equilateral_mesh(nx, ny, s=1.0):
    """a flat tiling by equilateral triangles of side s: rows sheared by half a side"""
    V, F = grid_mesh(nx, ny, flip=True)
    P = V.astype(np.float64)
    P = np.stack([s * (P[:, 0] + 0.5 * P[:, 1]), s * np.sqrt(0.75) * P[:, 1], P[:, 2]], 1)
    return P.astype(np.float32), F
