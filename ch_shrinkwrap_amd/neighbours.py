"""
The exact distance to the k-th nearest localization: ctypes binding of include/nw_neighbours.h (kernels in libnanowrap_hip.so,
csrc/nw_neighbours.hip) and what sits on top of it.

What it is for: a start surface whose bandwidth follows the cloud (isosurface.knn_isosurface).  Upstream's recipe is
Octree(n_points_min) -> DualMarchingCubes(threshold_density); the isosurface of the k-NN density k / (4/3 pi r_k^3) at threshold_density
is the level set r_k(x) = R_thr with R_thr = (3 k / (4 pi threshold_density))^(1/3).  The definitions (float64 distances to float32
points, duplicates counted, min(r_k, r_cap)) are the header's; tests/neighbours_ref.py restates them by brute force in NumPy.

    NeighbourContext    one nwk_ctx: set_cloud once, then kth_distance / node_field as often as needed
    kth_distance        one call: a cloud and queries in, min(r_k, r_cap) out
    local_density       k / (4/3 pi r^3) at every localization, r the distance to its k-th neighbour (itself not counted)

Everything runs on the device; there is no host fallback: without a GPU the context cannot be made and the call raises.
"""
import ctypes

import numpy as np

from . import _lib

SYMBOLS = ['nwk_abi_version', 'nwk_create', 'nwk_destroy', 'nwk_last_error', 'nwk_set_cloud', 'nwk_kth_distance', 'nwk_node_field',
           'nwk_field_ptr']
ABI_VERSION = 1
MAX_K = 32
FIELD_SHIFT = 20                                  # field = floor((r_cap - r_k) * 2^20)
NWK_OK, NWK_ERR_BADARG, NWK_ERR_HIP, NWK_ERR_NONFINITE, NWK_ERR_NOMEM, NWK_ERR_NOCLOUD = 0, -1, -2, -3, -4, -5
ERRORS = {NWK_ERR_BADARG: 'bad argument', NWK_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWK_ERR_NONFINITE: 'non-finite coordinate',
          NWK_ERR_NOMEM: 'out of device memory', NWK_ERR_NOCLOUD: 'the context holds no cloud'}

_L = None


def load():
    """The library's nwk_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
        L = _lib.load_entry_points(SYMBOLS, {
            'nwk_abi_version': [], 'nwk_create': [i32, ctypes.POINTER(vp)], 'nwk_destroy': [vp], 'nwk_last_error': [vp],
            'nwk_set_cloud': [vp, vp, i64, i32],
            'nwk_kth_distance': [vp, vp, i64, i32, i32, f64, vp],
            'nwk_node_field': [vp, vp, f32, vp, i32, f64, vp],
            'nwk_field_ptr': [vp]}, 'nwk_abi_version', ABI_VERSION, 'nw_neighbours')
        L.nwk_field_ptr.restype = vp                      # (the one entry point that returns a pointer)
        _L = L
    return _L


_p = _lib.ptr
_cloud = _lib.cloud_f32


class NeighbourContext(_lib.QueryContext):
    """One nwk_ctx: a cloud taken in once by set_cloud, its cell grid kept on the device, and any number of queries against it."""
    prefix, errors, gpu_only, load = 'nwk_', ERRORS, 'the k-th-neighbour distance runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_points = 0

    def set_cloud(self, points):
        """Take a float32 cloud in: (n,3) on the host, or (device pointer, n)."""
        keep, ptr, n, on_device = _cloud(points)
        self.n_points = 0
        self.check(self.L.nwk_set_cloud(self.h, ptr, n, on_device), 'nwk_set_cloud')
        self.n_points = n
        return self

    def kth_distance(self, queries, k=1, r_cap=np.inf):
        """min(r_k, r_cap) (nq,) float64 of `queries` ((nq,3) on the host, or (device pointer, nq) of float32 triples)."""
        keep, ptr, nq, on_device = _cloud(queries)
        out = np.empty(nq, np.float64)
        if nq:
            self.check(self.L.nwk_kth_distance(self.h, ptr, nq, on_device, int(k), float(r_cap), _p(out)), 'nwk_kth_distance')
        return out

    def node_field(self, lo, h, dims, k, r_cap, return_field=False):
        """The uint64 field floor((r_cap - min(r_k, r_cap)) * 2^20) at the nodes lo + (index + 1/2) h of a dims[0] x dims[1] x dims[2]
        lattice.  It stays on the device (field_pointer); with return_field a copy comes back, indexed [z, y, x]."""
        lo = np.ascontiguousarray(lo, np.float32).reshape(3)
        dims = np.ascontiguousarray(dims, np.int32).reshape(3)
        field = np.empty((int(dims[2]), int(dims[1]), int(dims[0])), np.uint64) if return_field else None
        self.check(self.L.nwk_node_field(self.h, _p(lo), float(h), _p(dims), int(k), float(r_cap), _p(field)), 'nwk_node_field')
        return field

    def field_pointer(self):
        """The device pointer of the last node_field's field, as an int (0 if there is none)."""
        return int(self.L.nwk_field_ptr(self.h) or 0)


def kth_distance(points, queries=None, k=1, r_cap=np.inf, context=None, device=0):
    """min(r_k, r_cap) at every query (default: at the cloud's own points, each of which then counts itself at distance 0).
    points / queries: (n,3) on the host or (device pointer, n) of float32 triples.  context: a NeighbourContext to use (it holds this
    cloud afterwards); one is made and closed otherwise."""
    own = context is None
    ctx = NeighbourContext(device) if own else context
    try:
        ctx.set_cloud(points)
        return ctx.kth_distance(points if queries is None else queries, k, r_cap)
    finally:
        if own:
            ctx.close()


def knn_density(r, k):
    """k / (4/3 pi r^3), inf where r = 0"""
    r = np.asarray(r, np.float64)
    with np.errstate(divide='ignore'):
        return float(k) / ((4.0 / 3.0 * np.pi) * (r * r * r))


def local_density(points, k=20, context=None, device=0):
    """The k-NN density (nm^-3) at every localization: k / (4/3 pi r^3), r the distance to its k-th neighbour -- the (k+1)-th smallest
    distance of kth_distance, whose first is the point itself.  inf where r = 0 (k + 1 coincident points); raises for n <= k."""
    n = int(points[1]) if isinstance(points, tuple) else np.asarray(points).reshape(-1, 3).shape[0]
    k = int(k)
    if not 1 <= k < MAX_K:
        raise ValueError('local_density: k must be in 1..%d' % (MAX_K - 1))
    if n <= k:
        raise ValueError('local_density: %d localizations have no %d-th neighbour' % (n, k))
    return knn_density(kth_distance(points, None, k + 1, np.inf, context, device), k)
