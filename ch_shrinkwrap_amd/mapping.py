"""
Localizations mapped onto a fitted surface: per-vertex density and per-vertex means of localization columns, in exact integers.
ctypes binding of include/nw_mapping.h (kernels in libnanowrap_hip.so, csrc/nw_mapping.hip) and what sits on top of it.

A fitted membrane can say how far each localization lies from it (distance_to_mesh); this says where on it the localizations are: the
surface density of the labelled protein per vertex, in localizations per nm^2, and the per-vertex mean of any localization column --
the mesh coloured by density, the first picture an SMLM user makes of a fitted ER or vesicle.  PYME is not part of the reference tree
and upstream has no such module, so nothing here mirrors reference code: the definition is this project's own and is written down in
csrc/nw_mapping_core.h.  A localization within `band` of the mesh is split between the three corners of its closest face by integer
weights that add up to 2^20; every accumulated quantity is an integer, so the result does not depend on the order of the cloud, on how
it was chunked, or on the launch.

    MappingContext    one nwl_ctx: set_mesh once, map as often as needed (the mesh, its cell grid and the accumulators stay on the device)
    map_to_surface    one call: points, a mesh and value columns in, the raw integer arrays out
    surface_density   density, localizations, area and column means per vertex
    SurfaceDensity    the recipe-module surface: a mesh and a table of localizations -> a per-vertex table and the table plus two columns

Everything but the last division (and the optional smoothing) runs on the device; there is no host fallback: without a GPU the context
cannot be made and every entry raises.
"""
import ctypes
import math

import numpy as np

from . import _lib

SYMBOLS = ['nwl_abi_version', 'nwl_create', 'nwl_destroy', 'nwl_last_error', 'nwl_set_mesh', 'nwl_get_areas', 'nwl_map']
ABI_VERSION = 1
NWL_OK, NWL_ERR_BADARG, NWL_ERR_HIP, NWL_ERR_NONFINITE, NWL_ERR_NOMEM, NWL_ERR_NOMESH, NWL_ERR_RANGE = 0, -1, -2, -3, -4, -5, -6
ERRORS = {NWL_ERR_BADARG: 'bad argument', NWL_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWL_ERR_NONFINITE: 'non-finite coordinate or value',
          NWL_ERR_NOMEM: 'out of device memory', NWL_ERR_NOMESH: 'the context holds no mesh', NWL_ERR_RANGE: 'a value larger than its scale'}
NWL_ACCUMULATE, NWL_WALK_ONLY = 1, 2
NWL_INFO_WORDS = 5
NWL_INFO_IN_BAND, NWL_INFO_RINGS, NWL_INFO_CENTROIDS, NWL_INFO_CELLS, NWL_INFO_CELL_SIZE = range(5)
MAX_COLUMNS = 8
W_ONE = 1 << 20               # the weights of one localization add up to it
Q_ONE = 1 << 30               # a value of +-scale
CHUNK = 1 << 22               # localizations per nwl_map call

_L = None


def load():
    """The library's nwl_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        _L = _lib.load_entry_points(SYMBOLS, {
            'nwl_abi_version': [], 'nwl_create': [i32, ctypes.POINTER(vp)], 'nwl_destroy': [vp], 'nwl_last_error': [vp],
            'nwl_set_mesh': [vp, vp, i64, vp, i64], 'nwl_get_areas': [vp, vp],
            'nwl_map': [vp, vp, i64, vp, i32, vp, f64, i32] + [vp] * 9},
            'nwl_abi_version', ABI_VERSION, 'nw_mapping')
    return _L


_p = _lib.ptr


class MappingError(RuntimeError):
    """A failed nwl_ call; `code` is its status (NWL_ERR_RANGE, NWL_ERR_NONFINITE, ...)."""

    def __init__(self, code, msg):
        RuntimeError.__init__(self, msg)
        self.code = code


def _mesh(mesh):
    """(positions float32, faces int32) of a TriMesh / MembraneMesh or a (vertices, faces) pair, as distance._mesh_arrays takes them"""
    from .distance import _mesh_arrays
    pos, faces, _ = _mesh_arrays(mesh, False)
    return pos, faces


def column_scale(x):
    """The scale the binding picks for a value column: 2^ceil(log2 max|x|), the smallest power of two that is >= every |x|; 1.0 for a
    column of zeros (or an empty one).  A column with a non-finite entry gets the scale of its finite ones: whether the entry matters
    is for the device to say (only an in-band localization's value is looked at)."""
    a = np.abs(np.asarray(x, np.float64))
    a = a[np.isfinite(a)]
    m = float(a.max()) if a.size else 0.0
    if not m > 0.0:
        return 1.0
    mant, e = math.frexp(m)                                       # m = mant 2^e, 0.5 <= mant < 1
    return math.ldexp(1.0, e - 1 if mant == 0.5 else e)


def column_sums(sum_hi, sum_lo):
    """The exact integer sums sum_hi 2^32 + sum_lo as an object array of Python integers"""
    return np.asarray(sum_hi).astype(object) * (1 << 32) + np.asarray(sum_lo).astype(object)


class MappingContext(_lib.QueryContext):
    """One nwl_ctx: a mesh taken in once by set_mesh, its centroid grid, vertex areas and accumulators kept on the device."""
    prefix, errors, gpu_only, load = 'nwl_', ERRORS, 'mapping localizations onto a mesh runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_vertices = self.n_faces = 0
        self.info = None

    def check(self, code, what):
        if code != 0:
            msg = self.L.nwl_last_error(self.h) if self.h else b''
            raise MappingError(code, '%s: %s %s' % (what, self.errors.get(code, 'error %d' % code), (msg or b'').decode()))

    def set_mesh(self, vertices, faces=None):
        """Take the mesh in: a TriMesh / MembraneMesh (faces None) or float32 vertices and int32 faces."""
        pos, f = _mesh(vertices if faces is None else (vertices, faces))
        self.n_vertices = self.n_faces = 0
        self.check(self.L.nwl_set_mesh(self.h, _p(pos), pos.shape[0], _p(f), f.shape[0]), 'nwl_set_mesh')
        self.n_vertices, self.n_faces = pos.shape[0], f.shape[0]
        return self

    def areas(self):
        """area3 (V,) uint64: per vertex the sum over its faces of floor(A_f 2^20); the vertex's area is area3 / (3 2^20)"""
        out = np.zeros(self.n_vertices, np.uint64)
        self.check(self.L.nwl_get_areas(self.h, _p(out)), 'nwl_get_areas')
        return out

    def map(self, points, band=30.0, values=None, scales=None, accumulate=False, per_point=True, accumulators=True, walk_only=False):
        """Map a cloud onto the mesh in the context -> dict.
        points: (n,3) float64 on the host, or (device pointer, n).  values: (n,C) float64 on the host, or (device pointer, C), C <= 8;
        scales: C powers of two, scale_c >= max |x_c| (picked by column_scale from a host array if None).
        per_point: face (n,) int32 (-1 out of band), weights (n,3) int32 (they add up to 2^20 in band), distance (n,) float64 (+inf out
        of band), closest (n,3) float64 (NaN out of band).  accumulators: mass (V,) uint64, count (F,) int32, sum_hi (V,C) int64,
        sum_lo (V,C) uint64 -- of this cloud, or with accumulate=True of this cloud and everything mapped since the last call without
        it.  A cloud of more than 2^22 localizations is mapped in chunks; the accumulators are integers, so the chunks add up to the
        whole.  walk_only: no accumulator is touched (for measuring the walk alone).  info: the counters, summed over the chunks."""
        from .distance import _points
        keep, ptr, n = _points(points)
        if n < 1:
            raise ValueError('an empty cloud has nothing to map')
        C, vptr, vkeep = 0, None, None
        if values is not None:
            if isinstance(values, tuple) and len(values) == 2 and isinstance(values[0], (int, np.integer)):
                vptr, C = int(values[0]), int(values[1])
                if scales is None:
                    raise ValueError('values on the device need scales')
            else:
                vkeep = np.ascontiguousarray(values, np.float64)
                vkeep = vkeep.reshape(n, -1) if vkeep.size else vkeep.reshape(n, 0)
                C, vptr = vkeep.shape[1], (vkeep.ctypes.data if vkeep.shape[1] else None)
                if scales is None:
                    scales = [column_scale(vkeep[:, c]) for c in range(C)]
        if C > MAX_COLUMNS:
            raise ValueError('at most %d value columns' % MAX_COLUMNS)
        sc = np.ascontiguousarray(scales if C else [], np.float64).ravel()
        if sc.size != C:
            raise ValueError('one scale per value column')
        V, F = self.n_vertices, self.n_faces
        out = dict(n_total=n, scales=sc.copy())
        if per_point:
            out.update(face=np.full(n, -1, np.int32), weights=np.zeros((n, 3), np.int32), distance=np.full(n, np.inf), closest=np.full((n, 3), np.nan))
        want_acc = accumulators and not walk_only
        if want_acc:
            out.update(mass=np.zeros(V, np.uint64), count=np.zeros(F, np.int32), sum_hi=np.zeros((V, C), np.int64), sum_lo=np.zeros((V, C), np.uint64))
        info = np.zeros(NWL_INFO_WORDS, np.int64)
        tot = np.zeros(NWL_INFO_WORDS, np.int64)
        base = ptr.value if ptr is not None and ptr.value else 0
        for s in range(0, n, CHUNK):
            e = min(n, s + CHUNK)
            last = e == n
            flags = NWL_WALK_ONLY if walk_only else (NWL_ACCUMULATE if (accumulate or s > 0) else 0)
            pp = (lambda a, k: ctypes.c_void_p(a.ctypes.data + s * k * a.itemsize)) if per_point else (lambda a, k: None)
            acc = (lambda k: _p(out[k])) if (want_acc and last) else (lambda k: None)
            self.check(self.L.nwl_map(self.h, ctypes.c_void_p(base + 24 * s), e - s, ctypes.c_void_p(vptr + 8 * C * s) if vptr else None, C, _p(sc) if C else None,
                                      float(band), flags,
                                      pp(out.get('face'), 1), pp(out.get('weights'), 3), pp(out.get('distance'), 1), pp(out.get('closest'), 3),
                                      acc('mass'), acc('count'), acc('sum_hi'), acc('sum_lo'), _p(info)), 'nwl_map')
            tot[:3] += info[:3]
            tot[3:] = info[3:]
        self.info = out['info'] = dict(in_band=int(tot[NWL_INFO_IN_BAND]), rings=int(tot[NWL_INFO_RINGS]), centroids=int(tot[NWL_INFO_CENTROIDS]),
                                       cells=int(tot[NWL_INFO_CELLS]), cell_size=float(tot[NWL_INFO_CELL_SIZE:NWL_INFO_CELL_SIZE + 1].view(np.float64)[0]))
        out['n_in_band'] = out['info']['in_band']
        return out


def _value_table(values, n):
    """names and an (n, C) float64 array of a dict name -> (n,) array"""
    names = list(values.keys()) if values else []
    cols = np.empty((n, len(names)), np.float64)
    for c, k in enumerate(names):
        a = np.asarray(values[k], np.float64).ravel()
        if a.size != n:
            raise ValueError('value column %s has %d entries for %d points' % (k, a.size, n))
        cols[:, c] = a
    return names, cols


def map_to_surface(points, mesh, band=30.0, values=None, context=None, device=0):
    """Localizations onto a mesh, the raw arrays: MappingContext.map's dict plus area3 (V,) uint64, names (the value columns in order)
    and n_total.  points: (n,3) on the host.  mesh: a TriMesh / MembraneMesh or (vertices, faces).  values: dict name -> (n,) array, at
    most 8; each column's scale is column_scale's.  context: a MappingContext to use (it holds this mesh afterwards); one is made and
    closed otherwise."""
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    names, cols = _value_table(values, pts.shape[0])
    own = context is None
    ctx = MappingContext(device) if own else context
    try:
        ctx.set_mesh(mesh)
        out = ctx.map(pts, band=band, values=cols if names else None)
        out['area3'] = ctx.areas()
        out['names'] = names
        return out
    finally:
        if own:
            ctx.close()


def densities(raw, neighbors=None, smooth=0):
    """map_to_surface's integers -> dict(density, n, area, means): the divisions of csrc/nw_mapping_core.h's step 5.  smooth = k with a
    (V, K) table of ring vertex ids (-1 padded): k rounds, each replacing mass and area3 -- as float64 -- by the vertex's own value plus
    its ring's; host NumPy, no exactness claim."""
    mass, area3 = raw['mass'].astype(np.float64), raw['area3'].astype(np.float64)
    sums = None
    if raw['names']:
        sums = column_sums(raw['sum_hi'], raw['sum_lo']).astype(np.float64)
    if smooth:
        nb = np.asarray(neighbors)
        ok = nb >= 0
        idx = np.where(ok, nb, 0)

        def ring(a):
            return a + np.where(ok, a[idx], 0.0).sum(1)
        for _ in range(int(smooth)):
            mass, area3 = ring(mass), ring(area3)
            if sums is not None:
                sums = np.stack([ring(sums[:, c]) for c in range(sums.shape[1])], 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        density = np.where(area3 > 0, 3.0 * mass / area3, np.nan)
        means = {}
        for c, k in enumerate(raw['names']):
            means[k] = np.where(mass > 0, sums[:, c] / mass * (raw['scales'][c] / Q_ONE), np.nan)
    return dict(density=density, n=mass / W_ONE, area=area3 / (3.0 * W_ONE), means=means)


def surface_density(points, mesh, band=30.0, values=None, smooth=0, context=None, device=0):
    """The density of a cloud on a mesh, per vertex: dict(density (V,) localizations per unit area, NaN at a vertex without area; n (V,)
    the localizations' weights at the vertex; area (V,) a third of the area of its faces; count (F,) int32 localizations per closest
    face; means: name -> (V,) the weighted mean of the column, NaN where n = 0; n_in_band, n_total; raw: map_to_surface's dict).
    smooth = k: k rounds of summing each vertex's mass and area with its ring's (TriMesh.vertex_neighbors) before the ratio is taken."""
    raw = map_to_surface(points, mesh, band=band, values=values, context=context, device=device)
    nb = None
    if smooth:
        if not hasattr(mesh, 'vertex_neighbors'):
            raise ValueError('smooth needs a mesh with vertex_neighbors (a TriMesh)')
        nb = mesh._halfedges['vertex'][mesh.vertex_neighbors]
        nb = np.where(mesh.vertex_neighbors >= 0, nb, -1)
    out = densities(raw, nb, smooth)
    out.update(count=raw['count'], n_in_band=raw['n_in_band'], n_total=raw['n_total'], raw=raw)
    return out


class SurfaceDensity(object):
    """Recipe-module surface for the density of localizations on a fitted surface, in the plain-attribute style of DistanceToMesh: the
    mesh under `input_mesh` and a table with x y z under `input_points` -> under `output` a per-vertex table x y z density
    n_localizations area and mean_<column> for every name in `columns`; under `output_points` the input table plus `surface_face` (-1
    beyond `band`) and `surface_distance` (+inf there).  PYME is not in the reference tree: the traits and the columns here are this
    project's own."""

    def __init__(self, **kw):
        self.input_mesh, self.input_points = 'membrane', 'filtered_localizations'
        self.output, self.output_points = 'membrane_density', 'mapped_localizations'
        self.band = 30.0
        self.columns = []
        self.smooth = 0
        self.device = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)

    def execute(self, namespace):
        src, mesh = namespace[self.input_points], namespace[self.input_mesh]
        pts = np.ascontiguousarray(np.vstack([src['x'], src['y'], src['z']]).T, np.float64)
        r = surface_density(pts, mesh, band=float(self.band), values={k: src[k] for k in self.columns}, smooth=int(self.smooth), device=self.device)
        pos, _ = _mesh(mesh)
        table = {'x': pos[:, 0].copy(), 'y': pos[:, 1].copy(), 'z': pos[:, 2].copy(), 'density': r['density'], 'n_localizations': r['n'], 'area': r['area']}
        for k in self.columns:
            table['mean_' + k] = r['means'][k]
        table['metadata'] = {'n_in_band': r['n_in_band'], 'n_total': r['n_total'], 'band': float(self.band), 'smooth': int(self.smooth)}
        mapped = {k: src[k] for k in src.keys()}
        mapped['surface_face'] = r['raw']['face']
        mapped['surface_distance'] = r['raw']['distance']
        namespace[self.output] = table
        namespace[self.output_points] = mapped
        return table
