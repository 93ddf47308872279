"""
The point-to-mesh distance restated in NumPy, brute force over all faces: what ch_shrinkwrap_amd/csrc/nw_distance_core.h computes,
operation for operation in float64 (NumPy rounds every product and every sum, as the header does when it is compiled with
-ffp-contract=off), and the meshes the tests of the core and of the device share.

    point_triangles   d2, closest point and feature code of every query against every face (plane first, then the three clamped
                      segments; a later candidate wins only when strictly nearer)
    pseudonormal      face normal, sum of the two unit normals at an edge, angle-weighted sum over the fan at a vertex (walked through
                      `twin`, both ways from a border, at most FAN_CAP faces)
    distance          the smallest (d2, face id) per query, its pseudonormal and the sign

tests/test_mesh_distance_ref.py ties this file to ground truth that does not come from it (a box's closed-form distance, a sphere).
"""
import math

import numpy as np

FAN_CAP = 256
CAPPED = 8


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _segment(p, v, w, fe, f0, f1, best, closest, feature):
    """one clamped segment v -> w (F,3) against the queries p (Q,1,3); updates best (Q,F), closest (Q,F,3), feature (Q,F) in place"""
    d = w - v
    dd = _dot(d, d)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(dd > 0.0, _dot(p - v, d) / dd, 0.0)
    lo, hi = ~(t > 0.0), t >= 1.0
    q = v + t[..., None] * d
    q = np.where(lo[..., None], v, np.where(hi[..., None], w, q))
    code = np.where(lo, f0, np.where(hi, f1, fe))
    e = p - q
    d2 = _dot(e, e)
    upd = d2 < best
    best[upd] = d2[upd]
    closest[upd] = q[upd]
    feature[upd] = code[upd]


def point_triangles(points, vertices, faces):
    """(d2 (Q,F), closest (Q,F,3), feature (Q,F)) of every query against every face"""
    p = np.asarray(points, np.float64).reshape(-1, 1, 3)
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    Q, F = p.shape[0], f.shape[0]
    best = np.full((Q, F), np.inf)
    closest = np.broadcast_to(a, (Q, F, 3)).copy()
    feature = np.full((Q, F), 4, np.int32)
    u, w = b - a, c - a
    n = _cross(u, w)
    nn = _dot(n, n)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = _dot(p - a, n) / nn
        h = p - t[..., None] * n
        w0 = _dot(_cross(u, h - a), n)
        w1 = _dot(_cross(c - b, h - b), n)
        w2 = _dot(_cross(a - c, h - c), n)
        e = p - h
        inside = (nn > 0.0) & (w0 >= 0.0) & (w1 >= 0.0) & (w2 >= 0.0)
        d2 = _dot(e, e)
    best[inside] = d2[inside]
    closest[inside] = h[inside]
    feature[inside] = 0
    _segment(p, a, b, 1, 4, 5, best, closest, feature)
    _segment(p, b, c, 2, 5, 6, best, closest, feature)
    _segment(p, c, a, 3, 6, 4, best, closest, feature)
    return best, closest, feature


def _add_face_normal(v, faces, g, corner, N):
    k = 0 if corner < 0 else corner
    a, b, c = (v[faces[g][(k + j) % 3]] for j in range(3))
    ux, uy, uz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
    vx, vy, vz = c[0] - a[0], c[1] - a[1], c[2] - a[2]
    nx, ny, nz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
    nn = (nx * nx + ny * ny) + nz * nz
    if not nn > 0.0:
        return
    ln = math.sqrt(nn)
    w = 1.0 if corner < 0 else math.atan2(ln, (ux * vx + uy * vy) + uz * vz)
    N[0] = N[0] + w * (nx / ln)
    N[1] = N[1] + w * (ny / ln)
    N[2] = N[2] + w * (nz / ln)


def pseudonormal(v, faces, twin, f, feature, taken=None):
    """(N, capped flag) of feature 0..6 of face f; v: the positions as nested lists of Python floats, faces and twin as lists.
    `taken` counts which branches ran ('closed', 'border', 'border_edge', 'capped')."""
    N = [0.0, 0.0, 0.0]
    taken = {} if taken is None else taken

    def count(k):
        taken[k] = taken.get(k, 0) + 1
    if feature == 0:
        _add_face_normal(v, faces, f, -1, N)
        return N, 0
    if feature <= 3:
        _add_face_normal(v, faces, f, -1, N)
        t = twin[3 * f + feature - 1]
        if t >= 0:
            _add_face_normal(v, faces, t // 3, -1, N)
        else:
            count('border_edge')
        return N, 0
    h0 = 3 * f + feature - 4
    h, steps, border = h0, 0, False
    while True:
        _add_face_normal(v, faces, h // 3, h % 3, N)
        steps += 1
        t = twin[3 * (h // 3) + (h % 3 + 2) % 3]
        if t < 0:
            border = True
            break
        if t == h0:
            count('closed')
            return N, 0
        if steps >= FAN_CAP:
            count('capped')
            return N, CAPPED
        h = t
    count('border')
    h = h0
    while border:
        t = twin[h]
        if t < 0:
            break
        h = 3 * (t // 3) + (t % 3 + 1) % 3
        if h == h0:
            break
        if steps >= FAN_CAP:
            count('capped')
            return N, CAPPED
        _add_face_normal(v, faces, h // 3, h % 3, N)
        steps += 1
    return N, 0


def distance(points, vertices, faces, twin=None, chunk=256, taken=None):
    """dict(d2, dist, closest, face, feature, normal, margin) per query.  dist is signed when `twin` is given (-1 entries on a border);
    margin = |(p - c).N| / (|p - c| |N|), the quantity a sign is compared by (nan where either length is 0)."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3)
    Q = p.shape[0]
    d2, closest = np.empty(Q), np.empty((Q, 3))
    face, feature = np.empty(Q, np.int32), np.empty(Q, np.int32)
    for s in range(0, Q, chunk):
        b, c, ft = point_triangles(p[s:s + chunk], vertices, f)
        k = np.argmin(b, axis=1)                               # (the first of equal minima: the smallest face id)
        r = np.arange(k.size)
        d2[s:s + chunk], closest[s:s + chunk], face[s:s + chunk], feature[s:s + chunk] = b[r, k], c[r, k], k, ft[r, k]
    dist = np.sqrt(d2)
    out = dict(d2=d2, closest=closest, face=face, feature=feature)
    if twin is not None:
        v = np.asarray(vertices, np.float32).astype(np.float64).tolist()
        fl, tl = f.tolist(), np.asarray(twin).tolist()
        N = np.zeros((Q, 3))
        for i in range(Q):
            n, cap = pseudonormal(v, fl, tl, int(face[i]), int(feature[i]), taken)
            N[i] = n
            feature[i] |= cap
        e = p - closest
        s = _dot(e, N)
        dist = np.where((s < 0.0) & (d2 > 0.0), -dist, dist)
        with np.errstate(divide='ignore', invalid='ignore'):
            out['margin'] = np.abs(s) / (np.sqrt(_dot(e, e)) * np.sqrt(_dot(N, N)))
        out['normal'] = N
    out['dist'] = dist
    return out


def twins(faces):
    """twin[3f+k] of an oriented face array (-1 on a border): half-edge 3f+k runs faces[f,k] -> faces[f,(k+1)%3]"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    table = {}
    for h, (o, d) in enumerate(zip(f.ravel().tolist(), f[:, [1, 2, 0]].ravel().tolist())):
        table.setdefault((o, d), h)
    return np.array([table.get((d, o), -1) for o, d in zip(f.ravel().tolist(), f[:, [1, 2, 0]].ravel().tolist())], np.int32)


# ---- the meshes of the tests ----------------------------------------------------------------------------------------------------------
def cube():
    """12 faces, corners at +-1, wound counter-clockwise seen from outside"""
    v = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


def box_sdf(p, half=1.0):
    """the closed form of a box's signed distance"""
    q = np.abs(np.asarray(p, np.float64)) - half
    return np.sqrt((np.maximum(q, 0.0) ** 2).sum(1)) + np.minimum(q.max(1), 0.0)


def spike():
    """a tetrahedron: base of radius 1 at z = 0, apex at (0, 0, 10)"""
    ang = np.deg2rad([0.0, 120.0, 240.0])
    v = np.array([[np.cos(a), np.sin(a), 0.0] for a in ang] + [[0.0, 0.0, 10.0]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    return v, f


def spike_queries(n=400):
    a = 2.0 * np.pi * np.arange(n) / n
    return np.stack([3.0 * np.cos(a), 3.0 * np.sin(a), np.full(n, 10.2)], 1)


L_POLYGON = np.array([[0, 0], [2, 0], [2, 1], [1, 1], [1, 2], [0, 2]], np.float64)


def l_prism():
    """the L-shaped hexagon L_POLYGON extruded over z in [0, 1]: the vertical edge at (1, 1) is concave, and so are its two ends"""
    n = len(L_POLYGON)
    v = np.array([[x, y, z] for z in (0.0, 1.0) for x, y in L_POLYGON], np.float32)
    cap = [(0, 1, 2), (0, 2, 3), (0, 3, 5), (3, 4, 5)]
    f = [(a + n, b + n, c + n) for a, b, c in cap] + [(a, c, b) for a, b, c in cap]
    for i in range(n):
        j = (i + 1) % n
        f += [(i, j, j + n), (i, j + n, i + n)]
    return v, np.array(f, np.int32)


def l_prism_inside(p):
    p = np.asarray(p, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return (z > 0) & (z < 1) & (x > 0) & (y > 0) & (((x < 2) & (y < 1)) | ((x < 1) & (y < 2)))


def disk(n=8, r=(1.0, 2.0)):
    """an open disk in the plane z = 0, normal +z: a centre, an inner and an outer ring of n vertices"""
    a = 2.0 * np.pi * np.arange(n) / n
    v = [[0.0, 0.0, 0.0]] + [[rr * np.cos(t), rr * np.sin(t), 0.0] for rr in r for t in a]
    f = []
    for i in range(n):
        j = (i + 1) % n
        f += [(0, 1 + i, 1 + j), (1 + i, 1 + n + i, 1 + n + j), (1 + i, 1 + n + j, 1 + j)]
    return np.array(v, np.float32), np.array(f, np.int32)


def needles(n=40, length=1000.0, width=0.1, seed=3):
    """n separate triangles of aspect length / width = 10^4 in random orientations"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1)[:, None]
    p0 = rng.uniform(-300.0, 300.0, (n, 3))
    tri = np.stack([p0, p0 + length * u, p0 + rng.uniform(0.2, 0.8, (n, 1)) * length * u + width * w], 1)
    return tri.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def triangle_region_queries():
    """one triangle in the plane z = 0 and queries in each of its seven regions (above the plane and in it), on its edges, at its
    vertices -> (vertices, faces, queries, the feature code each is meant for)"""
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    xy = [((1.0, 1.0), 0), ((2.0, -1.0), 1), ((3.0, 2.5), 2), ((-1.0, 1.5), 3), ((-1.0, -1.0), 4), ((6.0, -0.5), 5), ((-0.5, 5.0), 6)]
    q, code = [], []
    for (x, y), k in xy:
        for z in (0.7, 0.0, -0.3):
            q.append((x, y, z))
            code.append(k)
    # on the edges and at the vertices, in the plane: the projection is the query itself and no edge function is negative, so the plane
    # candidate answers first with d2 = 0 and no segment is strictly nearer
    for pt in ((2.0, 0.0, 0.0), (2.0, 1.5, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 3.0, 0.0)):
        q.append(pt)
        code.append(0)
    return v, f, np.array(q, np.float64), np.array(code)


def degenerate_faces():
    """a face with a zero-length edge (two corners equal), one with three collinear corners, one that is a point, beside a proper one"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [3, 0, 0], [5, 0, 0], [2, 2, 2]], np.float32)
    f = np.array([[0, 1, 2], [3, 3, 4], [3, 4, 5], [6, 6, 6], [4, 4, 6]], np.int32)
    return v, f


# ---- what the tests of the compiled core and of the device share -----------------------------------------------------------------------
SIGN_MARGIN = 1e-9            # signs are compared where |(p - c).N| > SIGN_MARGIN |p - c| |N|


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_as_restatement(mine, ref, signed):
    """the equalities every implementation owes the restatement -> how many signs were compared"""
    assert np.array_equal(bits(mine['d2']), bits(ref['d2']))
    assert np.array_equal(bits(mine['closest']), bits(ref['closest']))
    assert np.array_equal(mine['face'], ref['face']) and np.array_equal(mine['feature'], ref['feature'])
    assert np.array_equal(bits(np.abs(mine['dist'])), bits(np.abs(ref['dist'])))
    assert not np.signbit(mine['dist'][mine['d2'] == 0]).any()
    if not signed:
        assert not np.signbit(mine['dist']).any()
        return 0
    clear = ref['margin'] > SIGN_MARGIN                        # (nan where the distance or the normal is 0: not compared)
    assert np.array_equal(np.signbit(mine['dist'][clear]), np.signbit(ref['dist'][clear]))
    return int(clear.sum())


def around(v, n, seed, spread=1.5):
    """queries in and around a mesh's box, some of them at its vertices"""
    v = np.asarray(v, np.float64)
    lo, hi = v.min(0), v.max(0)
    c, e = (lo + hi) / 2, np.maximum(hi - lo, 1e-3 * (hi - lo).max())
    q = c + np.random.default_rng(seed).uniform(-spread, spread, (n, 3)) * e / 2
    q[:min(8, len(v))] = v[:min(8, len(v))]
    return q
