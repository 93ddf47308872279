"""
The self-intersection check of ch_shrinkwrap_amd/csrc/nw_intersections_core.h, restated in NumPy operation for operation: float64 on the
float32 positions widened to double, a dot product (u0 v0 + u1 v1) + u2 v2, a cross product that rounds each product and subtracts
(NumPy contracts nothing).  It is brute force over all pairs f < g of faces -- no grid, no centroid filter -- so that it is an
independent check of the device's walk as well as of its arithmetic.

A crossing is proper: the interior of an edge of one face passes through the interior of the other.  Touching, coplanar overlap and
faces sharing an edge are none.  See the header for the definition; the names below are its names.

`mutate` switches on one deliberate mistake (tests/test_mesh_intersections_ref.py shows that each is caught):
    'ge'          the sign tests of seg_tri accept zero (>= for >, <= for <)
    'wrong_edge'  a shared corner k tests the edge k -> k+1 instead of the opposite one
    'one_plane'   the plane rejection of the s = 0 case is only made on B's side
"""
import numpy as np

MUTATIONS = ('ge', 'wrong_edge', 'one_plane')


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def normal(T):
    """T: (n,3,3) corners -> n = (b - a) x (c - a)"""
    return cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])


def seg_tri(p, q, T, n, mutate=None):
    sp, sq = dot(n, p - T[:, 0]), dot(n, q - T[:, 0])
    if mutate == 'ge':
        opposite = ((sp >= 0) & (sq <= 0)) | ((sp <= 0) & (sq >= 0))
    else:
        opposite = ((sp > 0) & (sq < 0)) | ((sp < 0) & (sq > 0))
    d = q - p
    ea, eb, ec = T[:, 0] - p, T[:, 1] - p, T[:, 2] - p
    w0, w1, w2 = dot(cross(ea, eb), d), dot(cross(eb, ec), d), dot(cross(ec, ea), d)
    if mutate == 'ge':
        return opposite & (((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0)))
    return opposite & (((w0 > 0) & (w1 > 0) & (w2 > 0)) | ((w0 < 0) & (w1 < 0) & (w2 < 0)))


def straddles(x, y, z):
    return ((x > 0) | (y > 0) | (z > 0)) & ((x < 0) | (y < 0) | (z < 0))


def pair_bits(vertices, faces, fa, fb, mutate=None):
    """The bit of every pair (fa[i], fb[i]) of distinct faces; the smaller id is A whichever way round it is given."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    fa, fb = np.asarray(fa, np.int64), np.asarray(fb, np.int64)
    assert (fa != fb).all()
    lo, hi = np.minimum(fa, fb), np.maximum(fa, fb)
    IA, IB = f[lo], f[hi]
    A, B = v[IA], v[IB]
    nA, nB = normal(A), normal(B)
    flat = ~(dot(nA, nA) > 0) | ~(dot(nB, nB) > 0)
    eq = IA[:, :, None] == IB[:, None, :]                             # eq[i, k, l]: corner k of A and corner l of B are one vertex
    s = eq.sum((1, 2))
    # s = 1: the first corner of A (of B) that is shared, and the edge opposite it
    ka = np.where(eq[:, 0].any(1), 0, np.where(eq[:, 1].any(1), 1, 2))
    kb = np.where(eq[:, :, 0].any(1), 0, np.where(eq[:, :, 1].any(1), 1, 2))
    r = np.arange(len(lo))
    o1, o2 = (0, 1) if mutate == 'wrong_edge' else (1, 2)
    one = seg_tri(A[r, (ka + o1) % 3], A[r, (ka + o2) % 3], B, nB, mutate) | seg_tri(B[r, (kb + o1) % 3], B[r, (kb + o2) % 3], A, nA, mutate)
    # s = 0
    rej_a = straddles(dot(nA, B[:, 0] - A[:, 0]), dot(nA, B[:, 1] - A[:, 0]), dot(nA, B[:, 2] - A[:, 0]))
    rej_b = straddles(dot(nB, A[:, 0] - B[:, 0]), dot(nB, A[:, 1] - B[:, 0]), dot(nB, A[:, 2] - B[:, 0]))
    if mutate == 'one_plane':
        rej_a = np.ones_like(rej_a)
    six = np.zeros(len(lo), bool)
    for k in range(3):
        six |= seg_tri(A[:, k], A[:, (k + 1) % 3], B, nB, mutate)
    for k in range(3):
        six |= seg_tri(B[:, k], B[:, (k + 1) % 3], A, nA, mutate)
    zero = rej_a & rej_b & six
    return ~flat & np.where(s == 0, zero, np.where(s == 1, one, False))


def self_intersections(vertices, faces, mutate=None):
    """dict(n_pairs, n_crossed_faces, count (F,) int32, pairs (n_pairs, 2) int32 sorted by (f, g) with f < g) over all pairs of faces"""
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nf = f.shape[0]
    fa, fb = np.triu_indices(nf, 1)
    hit = pair_bits(vertices, f, fa, fb, mutate) if fa.size else np.zeros(0, bool)
    pairs = np.stack([fa[hit], fb[hit]], axis=1).astype(np.int32)
    count = (np.bincount(pairs[:, 0], minlength=nf) + np.bincount(pairs[:, 1], minlength=nf)).astype(np.int32)
    return dict(n_pairs=int(pairs.shape[0]), n_crossed_faces=int((count > 0).sum()), count=count, pairs=pairs)


def shared_corners(faces, pairs):
    f = np.asarray(faces)
    return (f[pairs[:, 0]][:, :, None] == f[pairs[:, 1]][:, None, :]).sum((1, 2))


# ---- the inputs the CPU tests and the GPU tests share ------------------------------------------------------------------------------------
A_TRI = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)


def soup(*tris):
    """triangles given by their corners -> (vertices, faces) with no shared vertex"""
    v = np.concatenate([np.asarray(t, np.float32).reshape(3, 3) for t in tris])
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def cube_and_plane():
    v = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32)
    f = [[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6],                # z = 0, z = 1
         [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]]
    v = np.concatenate([v, np.array([[-5, -5, 0.3], [7, -5, 0.3], [-5, 7, 0.3]], np.float32)])
    return v, np.array(f + [[8, 9, 10]], np.int32)


# A against B, no vertex shared: name -> (B's corners, pairs expected)
TWO_TRIANGLES = {
    'pierced':            ([[1, 1, -1], [1, 1, 1], [5, 5, 1]], 1),
    'corner_on_interior': ([[1, 1, 0], [1, 2, 2], [2, 1, 2]], 0),
    'edge_in_plane':      ([[1, 1, 0], [2, 1, 0], [1, 1, 3]], 0),
    'coplanar_overlap':   ([[1, 1, 0], [5, 1, 0], [1, 5, 0]], 0),
    'edge_through_edge':  ([[2, -1, -1], [2, -1, 1], [2, 5, 5]], 0),
}


def shared_corner(crossing, rot_a=0, rot_b=0):
    """A and a face with A's corner 0 as one of its own, each with its corner order rotated"""
    other = [[2, 1, -1], [1, 2, 1]] if crossing else [[3, 1, 1], [1, 3, 1]]
    v = np.concatenate([A_TRI, np.array(other, np.float32)])
    fa, fb = np.roll([0, 1, 2], rot_a), np.roll([0, 3, 4], rot_b)
    return v, np.array([fa, fb], np.int32)


def noisy_sphere(scale):
    from ch_shrinkwrap_amd.trimesh import icosphere
    v, f = icosphere(2)
    noise = np.random.default_rng(0).normal(size=v.shape)          # (drawn first)
    return (v + scale * noise).astype(np.float32), f


def two_spheres(radius=1.0, centre=0.0):
    from ch_shrinkwrap_amd.trimesh import icosphere
    v, f = icosphere(2)
    v = np.asarray(v, np.float64)
    off = np.array([1.1, 0.13, 0.07])
    both = np.concatenate([radius * v + centre, radius * (v + off) + centre]).astype(np.float32)
    return both, np.concatenate([f, f + len(v)]).astype(np.int32), len(f)


def cushion(n=20, seed=3):
    """n random triangles with a common centroid"""
    t = np.random.default_rng(seed).normal(size=(n, 3, 3))
    t -= t.mean(1, keepdims=True)
    return soup(*t)


def with_flat_faces():
    v, f, _ = two_spheres()
    # a repeated vertex id, three collinear vertices (new ones, through the spheres), a face of three equal positions
    extra = np.array([[-3, 0, 0], [0, 0, 0], [3, 0, 0], [0.5, 0.1, 0.1], [0.5, 0.1, 0.1], [0.5, 0.1, 0.1]], np.float32)
    n = len(v)
    flat = np.array([[0, 0, 5], [7, 9, 7], [n, n + 1, n + 2], [n + 3, n + 4, n + 5]], np.int32)
    return np.concatenate([v, extra]), np.concatenate([f[:100], flat, f[100:]]).astype(np.int32), np.arange(100, 104)


def strip(m):
    """m pairs of triangles, 10 apart along x: face 2i is pierced by face 2i + 1 -> pairs (2i, 2i + 1)"""
    tris = []
    for i in range(m):
        o = np.array([10.0 * i, 0, 0])
        tris += [A_TRI + o, np.array(TWO_TRIANGLES['pierced'][0], np.float64) + o]
    v, f = soup(*tris)
    return v, f, np.stack([2 * np.arange(m), 2 * np.arange(m) + 1], axis=1).astype(np.int32)


def sphere_and_oversize_face():
    """icosphere(2) and one face spanning three times its box: rho_max makes every face's box the whole grid"""
    from ch_shrinkwrap_amd.trimesh import icosphere
    v, f = icosphere(2)
    big = np.array([[-3, -3, 0.21], [3, -3, 0.21], [0, 3, 0.21]], np.float32)
    n = len(v)
    return np.concatenate([np.asarray(v, np.float32), big]), np.concatenate([f, [[n, n + 1, n + 2]]]).astype(np.int32)


def same_as_restatement(mine, ref):
    """count, n_pairs, n_crossed_faces and the sorted pair list, exactly"""
    assert mine['n_pairs'] == ref['n_pairs'] and mine['n_crossed_faces'] == ref['n_crossed_faces'], (mine['n_pairs'], ref['n_pairs'])
    assert np.array_equal(mine['count'], ref['count'])
    if mine.get('pairs') is not None:
        assert np.array_equal(np.asarray(mine['pairs']).reshape(-1, 2), ref['pairs'])
