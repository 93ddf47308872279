"""
The local shape of a cloud: the neighbourhood covariance of every localization (structure tensor, local PCA), from exact integer
moments.  ctypes binding of include/nw_structure.h (kernels in libnanowrap_hip.so, csrc/nw_structure.hip) and what sits on top of it.

Does a localization sit on a sheet, a tubule or a blob, and which way does the structure face there: what a user needs before a fit, and
where no fit exists.  PYME is not part of the reference tree and upstream has no such module, so nothing here mirrors reference code:
the definition is this project's own and is written down in csrc/nw_structure_core.h.  The neighbourhood is a ball of radius r, not the
k nearest neighbours: a tie in distance is then harmless, and every point at exactly r is in.  tests/local_shape_ref.py restates the
whole query by brute force in NumPy.

  the exact layer: integers, a function of the input alone
    StructureContext            one nwf_ctx: set_cloud once, query as often as needed (the cloud and its grid stay on the device)
    local_moments               one call: n, S1 and S2 of every neighbourhood
  a fixed float64 procedure on those integers, on the device: covariance, cyclic Jacobi, order, signs
    local_shape                 eigenvalues, axis and normal of every neighbourhood, and the features below
    cloud_normals               the normals alone, as float32
  host float64 arithmetic with no exactness claim
    the features of local_shape linearity, planarity, scattering, surface_variation, centroid_offset
    radius_from_k               a radius from the k-th-neighbour distances of the neighbours unit
  recipe-module surface
    LocalShape                  a table -> the table plus n_neighbours linearity planarity scattering xn yn zn xa ya za shape_class

The orientation of a normal is local: its largest component is positive, or it faces a viewpoint.  Nothing is propagated over the cloud.
Everything that counts runs on the device; there is no host fallback: without a GPU the context cannot be made and every entry raises.
"""
import ctypes

import numpy as np

from . import _lib

SYMBOLS = ['nwf_abi_version', 'nwf_create', 'nwf_destroy', 'nwf_last_error', 'nwf_set_cloud', 'nwf_query']
ABI_VERSION = 1
NWF_OK, NWF_ERR_BADARG, NWF_ERR_HIP, NWF_ERR_NONFINITE, NWF_ERR_NOMEM, NWF_ERR_NOCLOUD = 0, -1, -2, -3, -4, -5
ERRORS = {NWF_ERR_BADARG: 'bad argument', NWF_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWF_ERR_NONFINITE: 'non-finite coordinate',
          NWF_ERR_NOMEM: 'out of device memory', NWF_ERR_NOCLOUD: 'the context holds no cloud yet'}
NWF_INFO_WORDS = 8
(NWF_INFO_TESTS, NWF_INFO_CELLS_READ, NWF_INFO_CELL_SIZE, NWF_INFO_CELLS, NWF_INFO_NEIGHBOURS, NWF_INFO_FEW, NWF_INFO_N_QUERIES, NWF_INFO_N_CLOUD) = range(8)
NWF_FLAG_VALID, NWF_FLAG_EMPTY, NWF_FLAG_FEW, NWF_FLAG_POINT, NWF_FLAG_TURNED = 1, 2, 4, 8, 16
NWF_MOMENT_WORDS = 10
MAX_N = 1 << 26
MAX_R = 2.0 ** 40
Q_ONE = 2.0 ** 18             # a neighbour's offset is quantised to R / 2^18, R the smallest power of two >= r
SWEEPS = 5                    # of the cyclic Jacobi iteration
CELL_OF_R = 0.5               # the cell size a grid starts from, as a share of the radius

_L = None


def load():
    """The library's nwf_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        _L = _lib.load_entry_points(SYMBOLS, {
            'nwf_abi_version': [], 'nwf_create': [i32, ctypes.POINTER(vp)], 'nwf_destroy': [vp], 'nwf_last_error': [vp],
            'nwf_set_cloud': [vp, vp, i64, i32], 'nwf_query': [vp, vp, i64, i32, f64, vp, vp, vp, vp, vp, vp]},
            'nwf_abi_version', ABI_VERSION, 'nw_structure')
    return _L


_p = _lib.ptr
_cloud = _lib.cloud_f32


def _info(words):
    return dict(tests=int(words[NWF_INFO_TESTS]), cells_read=int(words[NWF_INFO_CELLS_READ]),
                cell_size=float(words[NWF_INFO_CELL_SIZE:NWF_INFO_CELL_SIZE + 1].view(np.float64)[0]), cells=int(words[NWF_INFO_CELLS]),
                neighbours=int(words[NWF_INFO_NEIGHBOURS]), few=int(words[NWF_INFO_FEW]), n_queries=int(words[NWF_INFO_N_QUERIES]),
                n_cloud=int(words[NWF_INFO_N_CLOUD]))


def quantum(radius):
    """The size of one step of the quantisation, R / 2^18 with R the smallest power of two >= radius: the unit of S1 (its square: of S2)."""
    f, e = np.frexp(float(radius))
    return (float(radius) if f == 0.5 else float(np.ldexp(1.0, e))) / Q_ONE


class StructureContext(_lib.QueryContext):
    """One nwf_ctx: a cloud taken in once by set_cloud and kept on the device with its cell grid, and any number of queries of it."""
    prefix, errors, gpu_only, load = 'nwf_', ERRORS, 'the local shape runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_points = 0

    def set_cloud(self, points):
        """Take a float32 cloud in: (n,3) on the host, or (device pointer, n)."""
        keep, ptr, n, on_device = _cloud(points)
        self.n_points = 0
        self.check(self.L.nwf_set_cloud(self.h, ptr, n, on_device), 'nwf_set_cloud')
        self.n_points = n
        return self

    def query(self, radius, queries=None, viewpoint=None, moments=True, shape=True):
        """One query with the cloud at hand -> dict(moments (nq,10) int64 or None; eigenvalues (nq,3), vectors (nq,3,3) float64 and flags
        (nq,) uint8, or None; n_queries, n_cloud, info).  queries = None: the cloud's own points, each of them in its own neighbourhood.
        Otherwise (nq,3) on the host or (device pointer, nq).  viewpoint: three numbers the normals are to face, or None.  moments /
        shape = False leaves those arrays on the device."""
        if queries is None:
            keep, ptr, nq, on_device = None, None, 0, 0
            n_queries = self.n_points
        else:
            keep, ptr, nq, on_device = _cloud(queries)
            n_queries = nq
        view = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float64).reshape(3)
        mom = np.zeros((n_queries, NWF_MOMENT_WORDS), np.int64) if moments else None
        lam = np.zeros((n_queries, 3), np.float64) if shape else None
        vec = np.zeros((n_queries, 3, 3), np.float64) if shape else None
        flags = np.zeros(n_queries, np.uint8) if shape else None
        info = np.zeros(NWF_INFO_WORDS, np.int64)
        self.check(self.L.nwf_query(self.h, ptr, nq, on_device, float(radius), _p(view), _p(mom), _p(lam), _p(vec), _p(flags), _p(info)), 'nwf_query')
        return dict(moments=mom, eigenvalues=lam, vectors=vec, flags=flags, n_queries=n_queries, n_cloud=self.n_points, info=_info(info))


def _query(points, radius, other, viewpoint, context, device, **kw):
    own = context is None
    ctx = StructureContext(device) if own else context
    try:
        ctx.set_cloud(points if other is None else other)
        return ctx.query(radius, None if other is None else points, viewpoint, **kw)
    finally:
        if own:
            ctx.close()


def local_moments(points, radius, other=None, context=None, device=0):
    """The raw integers of every neighbourhood -> dict(n (nq,), S1 (nq,3), S2 (nq,6) in the order xx xy xz yy yz zz, moments (nq,10): all
    int64; quantum: the size of one step, so that S1 * quantum and S2 * quantum^2 are in the cloud's units; info).
    points: (n,3) on the host or (device pointer, n) of float32 triples.  other = None: every point of `points` against `points` itself
    (it is in its own neighbourhood).  other given: `points` are the queries and `other` is the cloud.  A neighbour is a cloud point with
    d2 <= radius^2 in float64, inclusive; its offset from the query is rounded to a multiple of quantum, ties to even.
    context: a StructureContext to use (it holds the cloud afterwards); one is made and closed otherwise."""
    r = _query(points, radius, other, None, context, device, shape=False)
    M = r['moments']
    return dict(n=M[:, 0].copy(), S1=M[:, 1:4].copy(), S2=M[:, 4:10].copy(), moments=M, quantum=quantum(radius), info=r['info'])


def shape_features(moments, eigenvalues, flags, radius):
    """The features of local_shape from the device's numbers, in float64 with max(lambda, 0), NaN where not valid:
        linearity (l0 - l1) / l0, planarity (l1 - l2) / l0, scattering l2 / l0 (the three add up to 1),
        surface_variation l2 / (l0 + l1 + l2), centroid_offset |S1 / n| * quantum (how far the neighbourhood's centroid is from the query).
    Host arithmetic with no exactness claim."""
    valid = (flags & NWF_FLAG_VALID) != 0
    with np.errstate(all='ignore'):
        l = np.maximum(eigenvalues, 0.0)
        l0, l1, l2 = l[:, 0], l[:, 1], l[:, 2]
        m = moments[:, 1:4].astype(np.float64) / moments[:, 0].astype(np.float64)[:, None]
        out = dict(linearity=(l0 - l1) / l0, planarity=(l1 - l2) / l0, scattering=l2 / l0, surface_variation=l2 / (l0 + l1 + l2),
                   centroid_offset=np.sqrt((m * m).sum(1)) * quantum(radius))
    out = {k: np.where(valid, v, np.nan) for k, v in out.items()}
    out['valid'] = valid
    return out


def local_shape(points, radius, other=None, viewpoint=None, context=None, device=0):
    """The shape of every neighbourhood -> dict(n (nq,) int64; eigenvalues (nq,3) float64, descending, in the cloud's units squared; axis
    (nq,3) the direction of the largest and normal (nq,3) the direction of the smallest eigenvalue; linearity, planarity, scattering,
    surface_variation, centroid_offset (see shape_features: NaN where not valid); valid (nq,) bool: n >= 3 and the largest eigenvalue > 0;
    vectors (nq,3,3) with rows axis, mid, normal; flags, moments, info).
    points, radius, other, context: as local_moments.  The eigenvalues and vectors come from the device: the covariance of the integer
    moments and a fixed number of Jacobi sweeps, the same float64 operations in the same order for every query.  A vector's component of
    largest magnitude is positive; with a viewpoint (three numbers) the normal faces it instead.  The orientation is local only."""
    r = _query(points, radius, other, viewpoint, context, device)
    out = dict(n=r['moments'][:, 0].copy(), eigenvalues=r['eigenvalues'], axis=r['vectors'][:, 0].copy(), normal=r['vectors'][:, 2].copy())
    out.update(shape_features(r['moments'], r['eigenvalues'], r['flags'], radius))
    out.update(vectors=r['vectors'], flags=r['flags'], moments=r['moments'], info=r['info'])
    return out


def cloud_normals(points, radius, viewpoint=None, context=None, device=0):
    """(n,3) float32: the normal of every localization's neighbourhood (zero where it has none: cross queries aside, that cannot happen,
    a point is its own neighbour).  Orientation as local_shape's."""
    r = _query(points, radius, None, viewpoint, context, device, moments=False)
    return r['vectors'][:, 2].astype(np.float32)


def radius_from_k(points, k=20, factor=1.5, device=0):
    """A radius for local_shape when none is known: factor x the median distance from a localization to its k-th neighbour (the neighbours
    unit's exact distances, the point itself not counted).  A helper with no exactness claim: the median of an even number of distances
    and the product are host float64 arithmetic, and the choice of k and factor is a rule of thumb."""
    from . import neighbours
    n = int(points[1]) if isinstance(points, tuple) else np.asarray(points).reshape(-1, 3).shape[0]
    k = int(k)
    if not 1 <= k < neighbours.MAX_K:
        raise ValueError('radius_from_k: k must be in 1..%d' % (neighbours.MAX_K - 1))
    if n <= k:
        raise ValueError('radius_from_k: %d localizations have no %d-th neighbour' % (n, k))
    r = float(factor) * float(np.median(neighbours.kth_distance(points, None, k + 1, np.inf, None, device)))
    if not (r > 0 and np.isfinite(r)):
        raise ValueError('radius_from_k: the median %d-th-neighbour distance is %g: give a radius' % (k, r))
    return r


# ---- recipe-module surface ----------------------------------------------------------------------------------------------------------------
def _table_points(src):
    return np.ascontiguousarray(np.vstack([src['x'], src['y'], src['z']]).T, np.float32)


class LocalShape(object):
    """Recipe-module surface for the local shape of a cloud, in the plain-attribute style of the other recipe mirrors: the table with x y z
    under `input` -> under `output` the same table plus n_neighbours, linearity planarity scattering (NaN where not valid), xn yn zn (the
    normal, the columns upstream's ScreenedPoissonMesh takes with use_normals), xa ya za (the axis) and shape_class: 0 line, 1 plane,
    2 blob by the largest of the three features, -1 where not valid.  radius = None takes radius_from_k(k).  PYME is not in the reference
    tree: the traits and the columns here are this project's own."""

    def __init__(self, **kw):
        self.input, self.output = 'filtered_localizations', 'shape_localizations'
        self.radius = None
        self.k = 20
        self.viewpoint = None
        self.device = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)

    def execute(self, namespace):
        src = namespace[self.input]
        P = _table_points(src)
        radius = radius_from_k(P, int(self.k), device=self.device) if self.radius is None else float(self.radius)
        r = local_shape(P, radius, viewpoint=self.viewpoint, device=self.device)
        out = {k: src[k] for k in src.keys() if k != 'metadata'}
        three = np.stack([r['linearity'], r['planarity'], r['scattering']], 1)
        cls = np.where(r['valid'], np.argmax(np.where(r['valid'][:, None], three, 0.0), 1), -1).astype(np.int32)
        out.update(n_neighbours=r['n'], linearity=r['linearity'], planarity=r['planarity'], scattering=r['scattering'],
                   xn=r['normal'][:, 0], yn=r['normal'][:, 1], zn=r['normal'][:, 2], xa=r['axis'][:, 0], ya=r['axis'][:, 1], za=r['axis'][:, 2],
                   shape_class=cls)
        out['metadata'] = {'radius': radius, 'k': int(self.k), 'viewpoint': self.viewpoint, 'info': r['info']}
        namespace[self.output] = out
        return out
