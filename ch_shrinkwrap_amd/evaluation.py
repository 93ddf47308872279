"""
Fit quality in the reference's own terms: the evaluation recipes of the reference compare
a fitted mesh with the true object by

    PointsFromMesh           recipe_modules/surface_feature_extraction.py:76-105  -> evaluation_utils.points_from_mesh  (:35-150)
    AverageSquaredDistance   recipe_modules/surface_feature_extraction.py:107-138 -> evaluation_utils.average_squared_distance (:153-180)

i.e. a regular grid of points laid over every triangle of the mesh (spacing dx_min in the triangle's own plane) against a cloud of
points on the true surface, nearest-neighbour squared distances both ways: mse01, mse10 and mse_rms = sqrt((mse01 + mse10) / 2).
This module restates the two functions (paths relative to /root/reference/ch_shrinkwrap/) with the per-triangle loop vectorised; the
restatement is pinned by tests/golden/fit_quality.npz, produced by the reference's own functions (tests/golden/make_golden.py).
The metric is a block-boundary / end-of-fit diagnostic, not part of the iteration.  Every function runs on the host by default
(`backend='host'`: NumPy and scipy's cKDTree, the definition); `backend='device'` runs the same computation as kernels
(include/nw_evaluation.h, in libnanowrap_hip.so): the samples are the host function's bit for bit and in its order, the nearest
neighbours are exact, and fit_quality never brings the samples to the host.  There is no fallback from 'device' to 'host': without a
GPU it raises.  The recipe modules downstream of ShrinkwrapMembrane are mirrored at the end of the file: PointsFromMesh,
AverageSquaredDistance, MeshProperties (recipe_modules/surface_feature_extraction.py:76-167).
"""
import ctypes

import numpy as np
import scipy.spatial

from . import _lib

SYMBOLS = ['nwe_abi_version', 'nwe_create', 'nwe_destroy', 'nwe_last_error', 'nwe_sample_mesh', 'nwe_get_samples', 'nwe_nearest',
           'nwe_average_squared_distance']
ABI_VERSION = 1
NWE_OK, NWE_ERR_BADARG, NWE_ERR_HIP, NWE_ERR_NONFINITE, NWE_ERR_NOMEM, NWE_ERR_NOSAMPLES, NWE_ERR_TOOMANY = 0, -1, -2, -3, -4, -5, -6
ERRORS = {NWE_ERR_BADARG: 'bad argument', NWE_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWE_ERR_NONFINITE: 'non-finite point',
          NWE_ERR_NOMEM: 'out of device memory', NWE_ERR_NOSAMPLES: 'the context holds no samples', NWE_ERR_TOOMANY: 'too many grid nodes'}
NWE_SAMPLES = -1
SAMPLES = 'samples'               # in place of a cloud: the samples the context holds since its last sample_mesh

_L = None


def load():
    """The library's nwe_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        _L = _lib.load_entry_points(SYMBOLS, {
            'nwe_abi_version': [], 'nwe_create': [i32, ctypes.POINTER(vp)], 'nwe_destroy': [vp], 'nwe_last_error': [vp],
            'nwe_sample_mesh': [vp, vp, i64, vp, i64, f64, ctypes.POINTER(i64)],
            'nwe_get_samples': [vp, vp, vp],
            'nwe_nearest': [vp, vp, i64, vp, i64, vp, vp, ctypes.POINTER(f64)],
            'nwe_average_squared_distance': [vp, vp, i64, vp, i64, ctypes.POINTER(f64), ctypes.POINTER(f64)]},
            'nwe_abi_version', ABI_VERSION, 'nw_evaluation')
    return _L


_p = _lib.ptr


def _cloud(points):
    """-> (what keeps the memory alive, pointer, n): SAMPLES, an (n,3) array (copied to float64 if it is not), or (device pointer, n)."""
    if isinstance(points, str):
        if points != SAMPLES:
            raise ValueError('a cloud is an (n,3) array, (device pointer, n) or evaluation.SAMPLES')
        return None, None, NWE_SAMPLES
    if isinstance(points, tuple) and len(points) == 2 and isinstance(points[0], (int, np.integer)):
        return None, _p(int(points[0])), int(points[1])
    a = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    return a, _p(a), a.shape[0]


class EvaluationContext(_lib.QueryContext):
    """One nwe_ctx: the mesh sampler, whose samples stay on the device, and the exact nearest-neighbour query between two clouds."""
    prefix, errors, gpu_only, load = 'nwe_', ERRORS, "backend='device' of the fit-quality metric runs", staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_samples = 0

    def sample_mesh(self, pos, faces, dx_min=5.0):
        """points_from_mesh(p=1) of a float32 mesh, kept on the device; returns the number of samples."""
        pos, faces = _lib.mesh_arrays(pos, faces)
        n = ctypes.c_int64()
        self.n_samples = 0
        if faces.shape[0] == 0:
            return 0
        self.check(self.L.nwe_sample_mesh(self.h, _p(pos), pos.shape[0], _p(faces), faces.shape[0], float(dx_min), ctypes.byref(n)), 'nwe_sample_mesh')
        self.n_samples = int(n.value)
        return self.n_samples

    def samples(self, return_faces=False):
        """The samples held: (n,3) float64 (and the face each came from, (n,) int32)."""
        pos, face = np.zeros((self.n_samples, 3), np.float64), np.zeros(self.n_samples, np.int32)
        if self.n_samples:
            self.check(self.L.nwe_get_samples(self.h, _p(pos), _p(face) if return_faces else None), 'nwe_get_samples')
        return (pos, face) if return_faces else pos

    def nearest(self, reference, queries, return_dist=True, return_index=True):
        """(dist (Q,) float64, idx (Q,) int32, sum of dist^2): the nearest point of `reference` for every point of `queries`; ties go to
        the smallest index.  An output that is not asked for is None."""
        k0, p0, n0 = _cloud(reference)
        k1, p1, n1 = _cloud(queries)
        nq = self.n_samples if n1 == NWE_SAMPLES else n1
        dist = np.empty(nq, np.float64) if return_dist else None
        idx = np.empty(nq, np.int32) if return_index else None
        s = ctypes.c_double()
        self.check(self.L.nwe_nearest(self.h, p0, n0, p1, n1, _p(dist), _p(idx), ctypes.byref(s)), 'nwe_nearest')
        return dist, idx, float(s.value)

    def average_squared_distance(self, points0, points1):
        k0, p0, n0 = _cloud(points0)
        k1, p1, n1 = _cloud(points1)
        m0, m1 = ctypes.c_double(), ctypes.c_double()
        self.check(self.L.nwe_average_squared_distance(self.h, p0, n0, p1, n1, ctypes.byref(m0), ctypes.byref(m1)), 'nwe_average_squared_distance')
        return float(m0.value), float(m1.value)


class _borrowed(object):
    """`with _borrowed(context, device) as ctx`: the caller's context, or one of its own that is closed on the way out."""

    def __init__(self, context, device):
        self.own = context is None
        self.ctx = EvaluationContext(device) if self.own else context

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        if self.own:
            self.ctx.close()


def _backend(backend):
    if backend not in ('host', 'device'):
        raise ValueError("backend must be 'host' or 'device'")
    return backend == 'device'


def _float32_positions(mesh):
    pos = np.asarray(mesh._vertices['position'])
    if pos.dtype != np.float32:
        raise ValueError("backend='device' samples a float32 mesh (the dtype of the mesh records); this one is %s" % pos.dtype)
    return pos


def points_from_mesh(mesh, dx_min=5.0, p=1.0, rng=None, backend='host', return_normals=False, context=None, device=0):
    """evaluation_utils.points_from_mesh (:35-150): every triangle gets the points of a regular grid in its own
    plane (axes e0 = the first edge, e1 = normal x e0; origin at the grid offset the reference uses) that fall inside it.
    `mesh` needs `_vertices['position']` and `faces` like the reference's.  p < 1 keeps a random share (the reference draws it with
    the global numpy state, `np.random.choice`: pass `rng` to reproduce a draw); on the device it is drawn on the host from the
    device's result, exactly as here.  return_normals=True returns (points, normals) as the reference does (:136-149): the normal of
    the face whose centroid (the float32 mean of its corners) is nearest to each sample, from `mesh.face_normals`."""
    dev = _backend(backend)
    if dev:
        with _borrowed(context, device) as ctx:
            n = ctx.sample_mesh(_float32_positions(mesh), mesh.faces, dx_min)
            d = ctx.samples()                                   # ((0,3) float64 for a mesh without samples)
            normals = _sample_normals(mesh, d, ctx) if return_normals and n else None
    else:
        d = _points_from_mesh_host(mesh, dx_min)
        normals = _sample_normals(mesh, d, None) if return_normals and d.shape[0] else None
    if return_normals and normals is None:
        normals = np.zeros((0, 3), np.float32)
    if p < 1.0 and d.shape[0]:
        rng = np.random.default_rng() if rng is None else rng
        sub = rng.choice(d.shape[0], size=int(p * d.shape[0]), replace=False)
        d = d[sub]
        if return_normals:
            normals = normals[sub]
    return (d, normals) if return_normals else d


def _sample_normals(mesh, d, ctx):
    """normals[_faces] of evaluation_utils.py:136-149; ctx None = scipy's tree, else the device query against the held samples"""
    centers = np.asarray(mesh._vertices['position'])[np.asarray(mesh.faces)].mean(1)
    fn = np.asarray(mesh.face_normals if hasattr(mesh, 'face_normals') else mesh._faces['normal'])
    if ctx is None:
        _, face = scipy.spatial.cKDTree(centers).query(d, k=1)
    else:
        _, face, _ = ctx.nearest(centers, SAMPLES, return_dist=False)
    return fn[face]


def _face_grids(mesh, dx_min):
    """The float32 set-up of points_from_mesh for every face of non-zero area: its in-plane frame, the slopes of its edges and its
    grid (first node xa, ya relative to corner 0; nx x ny nodes).  -> a dict of arrays over those faces, and `ok`, which faces they are."""
    tris = np.asarray(mesh._vertices['position'])[np.asarray(mesh.faces)]                       # (F, 3, 3)
    norms = np.cross(tris[:, 2, :] - tris[:, 1, :], tris[:, 0, :] - tris[:, 1, :])               # :56
    nn = np.linalg.norm(norms, axis=1)
    ok = nn != 0                                                                                 # :63 degenerate triangles are left out
    norms = norms[ok] / nn[ok, None]
    tris = tris[ok]
    v0 = tris[:, 1, :] - tris[:, 0, :]
    e0 = v0 / np.linalg.norm(v0, axis=1)[:, None]
    e1 = np.cross(norms, e0, axis=1)
    x0, y0 = (tris[:, 0, :] * e0).sum(1), (tris[:, 0, :] * e1).sum(1)                            # :82-87
    x1, y1 = (tris[:, 1, :] * e0).sum(1), (tris[:, 1, :] * e1).sum(1)
    x2, y2 = (tris[:, 2, :] * e0).sum(1), (tris[:, 2, :] * e1).sum(1)
    xs, ys = np.vstack([x0, x1, x2]).T, np.vstack([y0, y1, y2]).T
    xl, xu, yl, yu = xs.min(1), xs.max(1), ys.min(1), ys.max(1)
    with np.errstate(divide='ignore', invalid='ignore'):
        x1x0, x2x1, x0x2 = x1 - x0, x2 - x1, x0 - x2
        m0 = (y1 - y0) / x1x0
        m0[x1x0 == 0] = 0
        m1 = (y2 - y1) / x2x1
        m1[x2x1 == 0] = 0
        m2 = (y0 - y2) / x0x2
        m2[x0x2 == 0] = 0
    s1, s2 = np.sign(m1), np.sign(m2)
    # the grid of triangle i: x = arange(xl - x0 - dx/2, xu - x0, dx), y likewise (:117-118), coordinates relative to vertex 0
    xa, xb = xl - x0 - dx_min / 2, xu - x0
    ya, yb = yl - y0 - dx_min / 2, yu - y0
    nx = np.maximum(np.ceil((xb - xa) / dx_min), 0).astype(np.int64)                            # numpy.arange's length
    ny = np.maximum(np.ceil((yb - ya) / dx_min), 0).astype(np.int64)
    return dict(ok=ok, tris=tris, e0=e0, e1=e1, x0=x0, y0=y0, x1=x1, y1=y1, x2=x2, y2=y2, m0=m0, m1=m1, m2=m2, s1=s1, s2=s2, xa=xa, ya=ya,
                nx=nx, ny=ny)


def node_counts(mesh, dx_min=5.0):
    """(F,) int64: the grid nodes points_from_mesh lays over each face before it tests them against the triangle; 0 for a face of zero
    area.  A face of non-zero area has at least one: its grid starts dx_min / 2 before the triangle's lower corner on both axes."""
    g = _face_grids(mesh, dx_min)
    per = np.zeros(g['ok'].shape[0], np.int64)
    per[g['ok']] = g['nx'] * g['ny']
    return per


def _points_from_mesh_host(mesh, dx_min):
    """points_from_mesh with p = 1 on the host: the definition the kernels follow operation for operation."""
    g = _face_grids(mesh, dx_min)
    tris, e0, e1, x0, y0, x1, y1, x2, y2 = (g[k] for k in ('tris', 'e0', 'e1', 'x0', 'y0', 'x1', 'y1', 'x2', 'y2'))
    m0, m1, m2, s1, s2, xa, ya, nx, ny = (g[k] for k in ('m0', 'm1', 'm2', 's1', 's2', 'xa', 'ya', 'nx', 'ny'))
    per = nx * ny
    tot = int(per.sum())
    if tot == 0:
        return np.zeros((0, 3), tris.dtype)
    t = np.repeat(np.arange(tris.shape[0]), per)                                                # triangle of every grid node
    k = np.arange(tot) - np.repeat(np.cumsum(per) - per, per)                                   # node number inside its grid (row-major: y outer)
    X = xa[t] + (k % nx[t]) * dx_min
    Y = ya[t] + (k // nx[t]) * dx_min
    inside = (Y > X * m0[t]) & (s1[t] * Y > s1[t] * (y1[t] - y0[t] + (X - x1[t] + x0[t]) * m1[t])) \
        & (s2[t] * Y < s2[t] * (y2[t] - y0[t] + (X - x2[t] + x0[t]) * m2[t]))                    # :123
    t, X, Y = t[inside], X[inside], Y[inside]
    return X[:, None] * e0[t] + Y[:, None] * e1[t] + tris[t, 0, :]                              # :126


def nearest(points0, points1, context=None, device=0):
    """(dist, idx): for every point of points1 its nearest point in points0, as cKDTree(points0).query(points1) -- on the device, exact,
    float64, ties to the smallest index."""
    with _borrowed(context, device) as ctx:
        dist, idx, _ = ctx.nearest(points0, points1)
    return dist, idx


def average_squared_distance(points0, points1, backend='host', context=None, device=0):
    """evaluation_utils.average_squared_distance (:153-180): (mean squared distance of points1 from their nearest neighbours in
    points0, the same of points0 from points1)."""
    if _backend(backend):
        with _borrowed(context, device) as ctx:
            return ctx.average_squared_distance(points0, points1)
    e0, _ = scipy.spatial.cKDTree(points0).query(points1, k=1)
    e1, _ = scipy.spatial.cKDTree(points1).query(points0, k=1)
    return np.nansum(e0 ** 2) / len(e0), np.nansum(e1 ** 2) / len(e1)


def fit_quality(mesh, surface_points, dx_min=5.0, backend='host', context=None, device=0):
    """What the reference's evaluation recipe records for a fit (recipe_modules/surface_feature_extraction.py:133-138):
    dict(mse01, mse10, mse_rms) between the grid points of the fitted mesh and points on the true surface (nm^2, nm^2, nm).
    backend='device': the samples are made, binned and queried on the device and never come to the host."""
    if _backend(backend):
        with _borrowed(context, device) as ctx:
            n = ctx.sample_mesh(_float32_positions(mesh), mesh.faces, dx_min)
            if n == 0:
                raise ValueError('fit_quality: the mesh has no sample at dx_min = %g' % dx_min)
            mse0, mse1 = ctx.average_squared_distance(SAMPLES, np.asarray(surface_points, np.float64))
        return dict(mse01=float(mse0), mse10=float(mse1), mse_rms=float(np.sqrt((mse0 + mse1) / 2)), n_mesh_points=int(n))
    m = points_from_mesh(mesh, dx_min=dx_min, p=1.0)
    mse0, mse1 = average_squared_distance(m, np.asarray(surface_points, m.dtype))
    return dict(mse01=float(mse0), mse10=float(mse1), mse_rms=float(np.sqrt((mse0 + mse1) / 2)), n_mesh_points=int(m.shape[0]))


# ---- mesh properties ----------------------------------------------------------------------------------------------------------------
def mesh_topology(faces, n_vertices=None):
    """dict(euler, manifold, border_loops, twin) of a face array, on the host.  euler = V - E + F over the vertices and edges the faces
    use.  manifold: no directed edge occurs twice (so no edge has more than two faces, and neighbours agree in orientation) and the
    faces at every vertex form one fan.  border_loops: the connected pieces of the border."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from . import surgery
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = (int(f.max()) + 1 if f.size else 0) if n_vertices is None else int(n_vertices)
    if f.shape[0] == 0:
        return dict(euler=0, manifold=True, border_loops=0, twin=np.zeros(0, np.int32))
    o, d = f.ravel(), f[:, [1, 2, 0]].ravel()
    distinct = np.unique(o * nv + d).size == o.size and bool((o != d).all())
    twin = surgery.twins(f, nv)
    # fans: corner 3f+k (vertex faces[f,k]) is linked to the corner of the same vertex in the face across half-edge 3f+k
    h = np.flatnonzero(twin >= 0)
    t = twin[h].astype(np.int64)
    across = 3 * (t // 3) + (t % 3 + 1) % 3
    g = coo_matrix((np.ones(h.size), (h, across)), shape=(o.size, o.size))
    n_fans, fan = connected_components(g, directed=False)
    used = np.unique(o)
    one_fan = np.unique(np.stack([o, fan], 1), axis=0).shape[0] == used.size
    # border loops: components of the graph of border edges
    b = np.flatnonzero(twin < 0)
    loops = 0
    if b.size:
        bv, inv = np.unique(np.concatenate([o[b], d[b]]), return_inverse=True)
        gb = coo_matrix((np.ones(b.size), (inv[:b.size], inv[b.size:])), shape=(bv.size, bv.size))
        loops = int(connected_components(gb, directed=False)[0])
    return dict(euler=surgery.euler_characteristic(f), manifold=bool(distinct and one_fan), border_loops=loops, twin=twin)


def mesh_properties(mesh, label_faces='device', device=0, self_intersections=False):
    """dict(euler, genus, manifold, components, area, volume) of a mesh with `vertices` / `faces` (or the reference's `_vertices['position']`).
    euler, manifold: mesh_topology.  components: edge-connected components of the faces.  genus: the sum of the components' genera,
    (2 components - euler - border loops) / 2 (a sphere 0, a torus 1, two spheres 0).  area and the signed volume (positive for a
    closed surface whose faces wind counter-clockwise seen from outside) are the sums over the components.
    label_faces='device': components, area and volume by nws_label_faces / nws_component_stats (include/nw_surgery.h); or a labeller
    `label_faces(faces, twin, mask) -> (label, n)` (surgery.scipy_label_faces), with area and volume summed in NumPy float64.
    self_intersections=True: two more entries, whether the surface is embedded as well as closed and manifold --
    `self_intersections`, the number of pairs of faces that properly cross, and `self_intersecting_faces`, the faces in such a pair
    (intersections.self_intersections, include/nw_intersections.h: on the device, no host fallback)."""
    from . import surgery
    pos = np.ascontiguousarray(mesh.vertices if hasattr(mesh, 'vertices') else mesh._vertices['position'], np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(mesh.faces, np.int32).reshape(-1, 3)
    top = mesh_topology(faces, pos.shape[0])
    if isinstance(label_faces, str):
        if label_faces != 'device':
            raise ValueError("label_faces must be 'device' or a callable(faces, twin, mask)")
        ctx = surgery.SurgeryContext(device)
        try:
            label, n = ctx.label_faces(faces, top['twin'])
            st = ctx.component_stats(pos, faces, top['twin'], label, n)
        finally:
            ctx.close()
        area, volume = float(st['area'].sum()), float(st['volume'].sum())
    else:
        n = label_faces(faces, top['twin'], None)[1]
        p0, p1, p2 = (pos[faces[:, k]].astype(np.float64) for k in range(3))
        area = float(0.5 * np.sqrt((np.cross(p1 - p0, p2 - p0) ** 2).sum(1)).sum())
        volume = float((p0 * np.cross(p1, p2)).sum() / 6.0)
    genus = (2 * int(n) - top['euler'] - top['border_loops']) // 2
    out = dict(euler=int(top['euler']), genus=int(genus), manifold=top['manifold'], components=int(n), area=area, volume=volume)
    if self_intersections:
        from .intersections import self_intersections as find
        x = find((pos, faces), return_pairs=False, device=device)
        out['self_intersections'], out['self_intersecting_faces'] = x['n_pairs'], x['n_faces']
    return out


# ---- recipe-module mirrors (recipe_modules/surface_feature_extraction.py:76-167) ------------------------------------------------------
class _Module(object):
    def _set(self, kw):
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)


def _table_points(src):
    return np.ascontiguousarray(np.vstack([src['x'], src['y'], src['z']]).T)


class PointsFromMesh(_Module):
    """Mirror of the recipe module `PointsFromMesh` (:76-105) in the plain-attribute style of ShrinkwrapMembrane: the mesh under `input`
    -> a table with x y z xn yn zn under `output`."""

    def __init__(self, **kw):
        self.input, self.output = 'membrane0', 'membrane0_localizations'
        self.dx_min = 5.0
        self.p = 1.0
        self.return_normals = True
        self.backend = 'host'                      # not a trait upstream: 'device' = the kernels of include/nw_evaluation.h
        self.device = 0
        self.rng = None                            # not a trait upstream (it draws from numpy's global state): reproduces a draw of p < 1
        self._set(kw)

    def execute(self, namespace):
        out = points_from_mesh(namespace[self.input], dx_min=self.dx_min, p=self.p, rng=self.rng, backend=self.backend,
                               return_normals=bool(self.return_normals), device=self.device)
        points, normals = out if self.return_normals else (out, None)
        if normals is None:                        # (upstream cannot run without them: its table always has the six columns)
            normals = np.full(points.shape, np.nan, np.float32)
        table = {'x': points[:, 0], 'y': points[:, 1], 'z': points[:, 2], 'xn': normals[:, 0], 'yn': normals[:, 1], 'zn': normals[:, 2]}
        namespace[self.output] = table
        return table


class AverageSquaredDistance(_Module):
    """Mirror of the recipe module `AverageSquaredDistance` (:107-142): two tables with x y z -> a one-row table mse01 mse10 mse_rms."""

    def __init__(self, **kw):
        self.input, self.input2, self.output = 'filtered_localizations', 'filtered', 'average_squared_distance'
        self.backend = 'host'                      # not a trait upstream
        self.device = 0
        self._set(kw)

    def execute(self, namespace):
        mse0, mse1 = average_squared_distance(_table_points(namespace[self.input]), _table_points(namespace[self.input2]),
                                              backend=self.backend, device=self.device)
        table = {'mse01': np.atleast_1d(mse0), 'mse10': np.atleast_1d(mse1), 'mse_rms': np.atleast_1d(np.sqrt((mse0 + mse1) / 2))}
        namespace[self.output] = table
        return table


class MeshProperties(_Module):
    """Mirror of the recipe module `MeshProperties` (:144-167): the mesh under `inputMesh` -> a one-row table euler genus manifold
    components, and the two columns upstream has commented out: area, volume.  With self_intersections=True two more:
    self_intersections (the crossing pairs of faces) and self_intersecting_faces."""

    def __init__(self, **kw):
        self.inputMesh, self.output = 'membrane', 'mesh_props'
        self.label_faces = 'device'                # not a trait upstream: see mesh_properties
        self.self_intersections = False            # not a trait upstream: see mesh_properties
        self.device = 0
        self._set(kw)

    def run(self, inputMesh):
        q = mesh_properties(inputMesh, label_faces=self.label_faces, device=self.device, self_intersections=bool(self.self_intersections))
        table = {'euler': np.atleast_1d(q['euler']), 'genus': np.atleast_1d(q['genus']), 'manifold': np.atleast_1d(int(q['manifold'])),
                 'components': np.atleast_1d(q['components']), 'area': np.atleast_1d(q['area']), 'volume': np.atleast_1d(q['volume'])}
        for name in ('self_intersections', 'self_intersecting_faces'):
            if name in q:
                table[name] = np.atleast_1d(q[name])
        return table

    def execute(self, namespace):
        table = self.run(namespace[self.inputMesh])
        namespace[self.output] = table
        return table
