"""
A cloud split into objects: exact DBSCAN clustering.  ctypes binding of include/nw_clustering.h (kernels in libnanowrap_hip.so,
csrc/nw_clustering.hip) and what sits on top of it.

Every real SMLM table needs this before a surface is fitted: separating structure from background, and one structure from the next.
Upstream users run PYME's DBSCANClustering ahead of the surface recipe; PYME is not part of the reference tree, so nothing here mirrors
reference code: the definition is this project's own and is written down in csrc/nw_clustering_core.h.  Two points are near when their
float64 squared distance is at most eps^2; a point with at least min_points points near it (itself included) is core; clusters are the
connected components of the core points; a non-core point with a core point near it goes to the NEAREST core point's cluster, ties to
the smallest index -- not, as in scikit-learn, to whichever cluster reaches it first, which depends on the order of the cloud.  The
labels are therefore a function of the cloud alone; tests/dbscan_ref.py restates them by brute force in NumPy.

    ClusterContext     one nwp_ctx: set_cloud once, dbscan as often as needed (the cloud and its cell grid stay on the device)
    dbscan             one call: a cloud, eps and min_points in, labels, anchors, counts, core flags and the cluster table out
    split_objects      the clusters as index arrays
    denoise            the mask of the points that belong to a cluster
    k_distance_curve   the sorted k-th-neighbour distances, the usual aid for reading off eps
    DBSCANClustering   the recipe-module surface: a table of localizations -> the table plus dbscanClumpID, dbscanCore, dbscanNeighbours

Everything runs on the device; there is no host fallback: without a GPU the context cannot be made and every entry raises.
"""
import ctypes

import numpy as np

from . import _lib

SYMBOLS = ['nwp_abi_version', 'nwp_create', 'nwp_destroy', 'nwp_last_error', 'nwp_set_cloud', 'nwp_set_shortcuts', 'nwp_dbscan', 'nwp_cluster_stats']
ABI_VERSION = 1
NWP_OK, NWP_ERR_BADARG, NWP_ERR_HIP, NWP_ERR_NONFINITE, NWP_ERR_NOMEM, NWP_ERR_NOCLOUD = 0, -1, -2, -3, -4, -5
ERRORS = {NWP_ERR_BADARG: 'bad argument', NWP_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWP_ERR_NONFINITE: 'non-finite coordinate',
          NWP_ERR_NOMEM: 'out of device memory', NWP_ERR_NOCLOUD: 'the context holds no cloud, or no clustering yet'}
NWP_INFO_WORDS = 12
(NWP_INFO_N_CORE, NWP_INFO_N_BORDER, NWP_INFO_N_NOISE, NWP_INFO_N_CLUSTERS, NWP_INFO_CELLS, NWP_INFO_CELL_SIZE, NWP_INFO_TESTS, NWP_INFO_SHORTCUT_A,
 NWP_INFO_SHORTCUT_B, NWP_INFO_GUARD, NWP_INFO_TESTS_COUNT, NWP_INFO_TESTS_HOOK) = range(12)
MAX_N = 1 << 30
MAX_EPS = 2.0 ** 40
CELL_OF_EPS = 0.57            # the cell size a grid starts from, as a share of eps

_L = None


def load():
    """The library's nwp_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        _L = _lib.load_entry_points(SYMBOLS, {
            'nwp_abi_version': [], 'nwp_create': [i32, ctypes.POINTER(vp)], 'nwp_destroy': [vp], 'nwp_last_error': [vp],
            'nwp_set_cloud': [vp, vp, i64, i32], 'nwp_set_shortcuts': [vp, i32],
            'nwp_dbscan': [vp, f64, i64, i64, vp, vp, vp, vp, vp, vp], 'nwp_cluster_stats': [vp, vp, vp, vp, vp]},
            'nwp_abi_version', ABI_VERSION, 'nw_clustering')
    return _L


_p = _lib.ptr
_cloud = _lib.cloud_f32


def _info(words):
    return dict(n_core=int(words[NWP_INFO_N_CORE]), n_border=int(words[NWP_INFO_N_BORDER]), n_noise=int(words[NWP_INFO_N_NOISE]),
                n_clusters=int(words[NWP_INFO_N_CLUSTERS]), cells=int(words[NWP_INFO_CELLS]),
                cell_size=float(words[NWP_INFO_CELL_SIZE:NWP_INFO_CELL_SIZE + 1].view(np.float64)[0]), tests=int(words[NWP_INFO_TESTS]),
                shortcut_a=int(words[NWP_INFO_SHORTCUT_A]), shortcut_b=int(words[NWP_INFO_SHORTCUT_B]), guard=int(words[NWP_INFO_GUARD]),
                tests_count=int(words[NWP_INFO_TESTS_COUNT]), tests_hook=int(words[NWP_INFO_TESTS_HOOK]))


class ClusterContext(_lib.QueryContext):
    """One nwp_ctx: a cloud taken in once by set_cloud and kept on the device with its cell grid, and any number of clusterings of it."""
    prefix, errors, gpu_only, load = 'nwp_', ERRORS, 'DBSCAN clustering runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_points = 0
        self.n_clusters = -1

    def set_cloud(self, points):
        """Take a float32 cloud in: (n,3) on the host, or (device pointer, n)."""
        keep, ptr, n, on_device = _cloud(points)
        self.n_points, self.n_clusters = 0, -1
        self.check(self.L.nwp_set_cloud(self.h, ptr, n, on_device), 'nwp_set_cloud')
        self.n_points = n
        return self

    def set_shortcuts(self, on):
        """Switch the two shortcuts on or off (no output but info changes with it: for measuring and for testing)."""
        self.check(self.L.nwp_set_shortcuts(self.h, 1 if on else 0), 'nwp_set_shortcuts')
        return self

    def dbscan(self, eps, min_points, count_cap=None):
        """One clustering of the cloud in the context -> dict(labels (n,) int32, -1 noise; anchor (n,) int32; count (n,) int32 =
        min(n_eps, count_cap); core (n,) bool; n_clusters; info).  count_cap defaults to min_points."""
        n = self.n_points
        cap = int(min_points) if count_cap is None else int(count_cap)
        labels, anchor, count, core = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        nc = ctypes.c_int32(-1)
        info = np.zeros(NWP_INFO_WORDS, np.int64)
        self.n_clusters = -1
        self.check(self.L.nwp_dbscan(self.h, float(eps), int(min_points), cap, _p(labels), _p(anchor), _p(count), _p(core), ctypes.byref(nc), _p(info)),
                   'nwp_dbscan')
        self.n_clusters = int(nc.value)
        return dict(labels=labels, anchor=anchor, count=count, core=core.astype(bool), n_clusters=self.n_clusters, info=_info(info))

    def stats(self):
        """The last clustering's clusters -> dict(sizes (C,) int64: all labelled points; n_core (C,) int64; first (C,) int32: the smallest
        core index; bbox (C,6) float32: min x y z, max x y z of the members)."""
        C = max(self.n_clusters, 0)
        sizes, n_core, first, bbox = np.zeros(C, np.int64), np.zeros(C, np.int64), np.zeros(C, np.int32), np.zeros((C, 6), np.float32)
        self.check(self.L.nwp_cluster_stats(self.h, _p(sizes), _p(n_core), _p(first), _p(bbox)), 'nwp_cluster_stats')
        return dict(sizes=sizes, n_core=n_core, first=first, bbox=bbox)


def dbscan(points, eps, min_points, count_cap=None, context=None, device=0):
    """DBSCAN of a cloud -> dict(labels, anchor, count, core, n_clusters, sizes, n_core, first, bbox, info).
    points: (n,3) on the host or (device pointer, n) of float32 triples.  eps: two points are near when their squared distance is at most
    eps^2.  min_points: a point with at least that many points near it, itself included, is core.  Neither has a default: see
    k_distance_curve.  count_cap: count = min(n_eps, count_cap); min_points (the default) is the cheap choice, >= n gives full counts.
    context: a ClusterContext to use (it holds this cloud afterwards); one is made and closed otherwise."""
    own = context is None
    ctx = ClusterContext(device) if own else context
    try:
        ctx.set_cloud(points)
        out = ctx.dbscan(eps, min_points, count_cap)
        out.update(ctx.stats())
        return out
    finally:
        if own:
            ctx.close()


def split_objects(points, eps, min_points, min_size=1, context=None, device=0):
    """The clusters of a cloud as a list of ascending index arrays, in label order; clusters of fewer than min_size points (core and border
    together) are dropped."""
    r = dbscan(points, eps, min_points, context=context, device=device)
    order = np.argsort(r['labels'], kind='stable')
    starts = np.searchsorted(r['labels'][order], np.arange(r['n_clusters'] + 1))
    return [order[starts[c]:starts[c + 1]] for c in range(r['n_clusters']) if starts[c + 1] - starts[c] >= min_size]


def denoise(points, eps, min_points, context=None, device=0):
    """The bool mask labels >= 0: the points that are core or border."""
    return dbscan(points, eps, min_points, context=context, device=device)['labels'] >= 0


def k_distance_curve(points, k, context=None, device=0):
    """The distances from every point to its k-th nearest point, sorted in descending order: the usual aid for reading off eps (the knee).
    It is neighbours.kth_distance(points, points, k), and that function counts the query itself at distance 0.  So core[i] <=>
    r_{min_points}(p_i) <= eps, up to the rounding of one sqrt: the curve for k = min_points crosses eps where the core points begin.
    Nothing chooses eps automatically."""
    from .neighbours import kth_distance
    return np.sort(kth_distance(points, points, int(k), context=context, device=device))[::-1]


class DBSCANClustering(object):
    """Recipe-module surface for DBSCAN, in the plain-attribute style of the other recipe mirrors, named as PYME's module is: the table with
    x y z under `input` -> under `output` the input's columns plus `clump_column` (label + 1, 0 for noise), dbscanCore (bool) and
    dbscanNeighbours (count, capped at min_clump_size).  The cluster table (sizes, n_core, first, bbox) goes out as the output's metadata.
    PYME is not in the reference tree: the traits and the columns here are this project's own.  The two numeric defaults are the tested
    two-vesicle scene's (tests/test_dbscan_ref.py), not a recommendation: read search_radius off k_distance_curve for your own cloud."""

    def __init__(self, **kw):
        self.input, self.output = 'filtered_localizations', 'clustered_localizations'
        self.search_radius = 25.0
        self.min_clump_size = 10
        self.clump_column = 'dbscanClumpID'
        self.device = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)

    def execute(self, namespace):
        src = namespace[self.input]
        pts = np.ascontiguousarray(np.vstack([src['x'], src['y'], src['z']]).T, np.float32)
        r = dbscan(pts, float(self.search_radius), int(self.min_clump_size), device=self.device)
        out = {k: src[k] for k in src.keys() if k != 'metadata'}
        out[self.clump_column] = r['labels'] + 1
        out['dbscanCore'] = r['core']
        out['dbscanNeighbours'] = r['count']
        out['metadata'] = {'search_radius': float(self.search_radius), 'min_clump_size': int(self.min_clump_size), 'n_clusters': r['n_clusters'],
                           'sizes': r['sizes'], 'n_core': r['n_core'], 'first': r['first'], 'bbox': r['bbox'], 'info': r['info']}
        namespace[self.output] = out
        return out
