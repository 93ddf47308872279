"""
Ray casting against a triangle mesh as ch_shrinkwrap_amd/csrc/nw_rays_core.h defines it, restated in NumPy operation for operation:
float64 on the float32 positions widened to double, a dot product (u0 v0 + u1 v1) + u2 v2, a cross product that rounds each product
and subtracts (NumPy contracts nothing).  It is brute force over all faces for every ray -- no grid, no clipping, no pieces -- so that
it is an independent check of the device's walk as well as of its arithmetic.  See the header for the definition; the names below
are its names.

`mutate` switches on one deliberate mistake (tests/test_mesh_rays_ref.py shows that each is caught):
    'strict'      the edge test is strict (> for >=, < for <=)
    't_ge'        t >= 0 is accepted instead of t > 0
    'tie_larger'  of two hits with the same t the larger face id wins
"""
import numpy as np

from mesh_intersections_ref import cross, dot

MUTATIONS = ('strict', 't_ge', 'tie_larger')
RHO_SLACK = 1e-9
EXITS = 1


def face_balls(v, f):
    """centroid ((a + b) + c) / 3 per axis and rho, the largest distance to a corner, enlarged"""
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cen = ((a + b) + c) / 3.0
    r2 = np.zeros(len(f))
    for p in (a, b, c):
        e = p - cen
        r2 = np.maximum(r2, dot(e, e))
    return cen, np.sqrt(r2) * (1.0 + RHO_SLACK)


def hit_matrix(vertices, faces, origins, directions, skip_vertex=None, skip_face=None, t_max=np.inf, mutate=None):
    """(hit (n, F) bool, t (n, F), den (n, F)) of every ray against every face"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    o = np.ascontiguousarray(origins, np.float64).reshape(-1, 1, 3)
    d = np.ascontiguousarray(directions, np.float64).reshape(-1, 1, 3)
    n_rays, nf = o.shape[0], f.shape[0]
    sv = np.full(n_rays, -1, np.int64) if skip_vertex is None else np.asarray(skip_vertex, np.int64)
    sf = np.full(n_rays, -1, np.int64) if skip_face is None else np.asarray(skip_face, np.int64)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    n = cross(b - a, c - a)                                           # (1, F, 3)
    cen, rho = face_balls(v, f)
    L = np.sqrt(dot(d, d))                                            # (n, 1)
    ok = (L > 0) & (dot(n, n) > 0)
    ok = ok & ~(f[None, :, :] == sv[:, None, None]).any(2) & (np.arange(nf)[None, :] != sf[:, None])
    ea, eb, ec = a - o, b - o, c - o
    w0, w1, w2 = dot(cross(ea, eb), d), dot(cross(eb, ec), d), dot(cross(ec, ea), d)
    if mutate == 'strict':
        ok = ok & (((w0 > 0) & (w1 > 0) & (w2 > 0)) | ((w0 < 0) & (w1 < 0) & (w2 < 0)))
    else:
        ok = ok & (((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))) & ~((w0 == 0) & (w1 == 0) & (w2 == 0))
    den = dot(n, d) + np.zeros_like(w0)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        t = dot(n, ea) / den
        ok = ok & (den != 0) & ((t >= 0) if mutate == 't_ge' else (t > 0)) & (t <= t_max)
        x = o + t[..., None] * d
        e = x - cen[None]
        ok = ok & (dot(e, e) <= (rho * rho)[None])
    return ok, t, den


def cast(vertices, faces, origins, directions, skip_vertex=None, skip_face=None, t_max=np.inf, mutate=None, chunk=256):
    """dict(t (n,) float64 with +inf for a miss, face (n,) int32 with -1, info (n,) int32, hits (n,) int32)"""
    o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float64).reshape(-1, 3)
    n = o.shape[0]
    out = dict(t=np.full(n, np.inf), face=np.full(n, -1, np.int32), info=np.zeros(n, np.int32), hits=np.zeros(n, np.int32))
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        hit, t, den = hit_matrix(vertices, faces, o[s:e], d[s:e], None if skip_vertex is None else np.asarray(skip_vertex)[s:e],
                                 None if skip_face is None else np.asarray(skip_face)[s:e], t_max, mutate)
        tt = np.where(hit, t, np.inf)
        best = tt.min(1)
        at = hit & (tt == best[:, None])
        nf = hit.shape[1]
        face = np.where(at, np.arange(nf)[None, :], -1).max(1) if mutate == 'tie_larger' else np.where(at, np.arange(nf)[None, :], nf).min(1)
        any_ = hit.any(1)
        face = np.where(any_, face, -1)
        out['t'][s:e] = best
        out['face'][s:e] = face
        out['info'][s:e] = np.where(any_ & (den[np.arange(e - s), np.maximum(face, 0)] > 0), EXITS, 0)
        out['hits'][s:e] = hit.sum(1)
    return out


def inside(points, vertices, faces, direction):
    """parity of the faces hit along one direction"""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    return (cast(vertices, faces, p, np.broadcast_to(np.asarray(direction, np.float64), p.shape))['hits'] & 1).astype(bool)


def same(mine, ref, count=True):
    """t, face and the info bit exactly; hits too if the cast counted"""
    assert np.array_equal(np.asarray(mine['t']), ref['t']), np.flatnonzero(np.asarray(mine['t']) != ref['t'])[:10]
    assert np.array_equal(np.asarray(mine['face']), ref['face'])
    assert np.array_equal(np.asarray(mine['info']) & EXITS, ref['info'])
    if count:
        assert np.array_equal(np.asarray(mine['hits']), ref['hits'])


# ---- the inputs the CPU tests and the GPU tests share ------------------------------------------------------------------------------------
def lattice_box(a=4, b=4, c=4):
    """the closed surface of the box [0,a] x [0,b] x [0,c] on the integer lattice, every unit square cut along one diagonal, wound
    counter-clockwise seen from outside: (vertices float32, faces int32, {lattice point: vertex id})"""
    ids, faces, dims = {}, [], (a, b, c)

    def vid(p):
        return ids.setdefault(tuple(p), len(ids))
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, dims[axis]):
            for i in range(dims[u]):
                for j in range(dims[w]):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):                      # counter-clockwise seen from +axis
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        q.append(vid(p))
                    if side == 0:
                        q = q[::-1]
                    faces += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    v = np.array(sorted(ids, key=ids.get), np.float32)
    return v, np.array(faces, np.int32), ids


def sphere(nsub, radius=100.0, centre=0.0):
    from ch_shrinkwrap_amd.trimesh import icosphere
    v, f = icosphere(nsub)
    return (np.asarray(v, np.float64) * radius + centre).astype(np.float32), np.asarray(f, np.int32)


def noisy_sphere(scale=0.05, centre=0.0, oversize=False):
    """icosphere(2) with Gaussian noise, optionally at an offset, optionally with one face spanning four times the mesh"""
    from ch_shrinkwrap_amd.trimesh import icosphere
    v, f = icosphere(2)
    v = np.asarray(v, np.float64) + scale * np.random.default_rng(0).normal(size=v.shape)
    f = np.asarray(f, np.int32)
    if oversize:
        n = len(v)
        v = np.concatenate([v, [[-4, -4, 0.21], [4, -4, 0.21], [0, 4, 0.21]]])
        f = np.concatenate([f, [[n, n + 1, n + 2]]]).astype(np.int32)
    return (v + centre).astype(np.float32), f


def vertex_normals(v, f):
    """area-weighted, normalised, float64 (the test's own: which normal is used does not matter to an exact comparison)"""
    d = np.asarray(v, np.float64)
    cr = np.cross(d[f[:, 1]] - d[f[:, 0]], d[f[:, 2]] - d[f[:, 0]])
    n = np.zeros_like(d)
    for k in range(3):
        np.add.at(n, f[:, k], cr)
    return n / np.linalg.norm(n, axis=1)[:, None]


def mixed_rays(v, n, seed, far=10.0):
    """n rays around a mesh: origins inside its box, outside it, on its box faces and `far` diagonals away; Gaussian directions, some
    aimed at the mesh, some axis-parallel with one or two zero components"""
    rng = np.random.default_rng(seed)
    d = np.asarray(v, np.float64)
    lo, hi = d.min(0), d.max(0)
    mid, half, diag = 0.5 * (lo + hi), 0.5 * (hi - lo), np.linalg.norm(hi - lo)
    o = mid + rng.uniform(-1, 1, (n, 3)) * half
    kind = np.arange(n) % 8
    o[kind == 1] = (mid + rng.uniform(-3, 3, (n, 3)) * half)[kind == 1]
    on = np.flatnonzero(kind == 2)
    axis = rng.integers(3, size=on.size)
    o[on, axis] = np.where(rng.random(on.size) < 0.5, lo[axis], hi[axis])
    u = rng.normal(size=(n, 3))
    fa = np.flatnonzero(kind == 3)
    o[fa] = mid + far * diag * u[fa] / np.linalg.norm(u[fa], axis=1)[:, None]
    dirs = rng.normal(size=(n, 3))
    aim = (kind == 3) | (kind == 4)
    dirs[aim] = (mid + rng.uniform(-0.6, 0.6, (n, 3)) * half - o)[aim]
    one = np.flatnonzero(kind == 5)
    dirs[one, rng.integers(3, size=one.size)] = 0.0
    two = np.flatnonzero(kind == 6)
    keep = rng.integers(3, size=two.size)
    z = np.zeros((two.size, 3))
    z[np.arange(two.size), keep] = rng.choice([-2.5, 0.7], two.size)
    dirs[two] = z
    away = np.flatnonzero(kind == 7)                                  # rays that miss the box: from outside, pointing away
    o[away] = mid + (1.5 + rng.random((away.size, 1))) * diag * u[away] / np.linalg.norm(u[away], axis=1)[:, None]
    dirs[away] = o[away] - mid + 0.1 * diag * rng.normal(size=(away.size, 3))
    return o, dirs


def parity_points():
    """300 points around a sphere of radius 100 and a Gaussian direction for each"""
    rng = np.random.default_rng(0)
    p = rng.uniform(-130, 130, (300, 3))
    return p, rng.normal(size=(300, 3))


def centroid_grid(vertices, faces, h=None):
    """The walk's cell grid over the face centroids as nwc_set_mesh lays it out (cell size: twice the mean rho unless given), built
    here in NumPy: dict(cen, rho, rho_max, lo, hi, h, dims, cstart, order) -- `order` lists the faces in cell order."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    cen, rho = face_balls(v, f)
    lo, hi = cen.min(0), cen.max(0)
    ext = hi - lo
    if h is None:
        h = max(2.0 * rho.sum() / len(f), ext.max() / 1024.0) if ext.max() > 0 else 1.0
    dims = np.minimum(1025, np.floor(ext / h) + 1).astype(np.int64)
    cell3 = np.minimum(np.maximum(np.floor((cen - lo) / h), 0), dims - 1).astype(np.int64)
    cell = (cell3[:, 2] * dims[1] + cell3[:, 1]) * dims[0] + cell3[:, 0]
    order = np.argsort(cell, kind='stable')
    cstart = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=int(dims.prod())))]).astype(np.int32)
    return dict(cen=cen, rho=rho, rho_max=float(rho.max()), lo=lo, hi=hi, h=float(h), dims=dims, cstart=cstart, order=order)
