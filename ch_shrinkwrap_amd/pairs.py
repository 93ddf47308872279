"""
Pair statistics of a cloud: the exact pair-distance histogram, and Ripley's K and the pair correlation on top of it.  ctypes binding of
include/nw_pairs.h (kernels in libnanowrap_hip.so, csrc/nw_pairs.hip) and what sits on top of it.

The standard second-order statistics of an SMLM table answer: is this protein clustered, at what scale, and is channel A co-clustered
with channel B.  Upstream users take them from PYME (PairwiseDistanceHistogram, Ripleys); PYME is not part of the reference tree, so
nothing here mirrors reference code: the definition is this project's own and is written down in csrc/nw_pairs_core.h.  The counts
are integers of float64 squared distances compared with r_b * r_b -- a pair at exactly an edge belongs to the bin the edge closes, no
root is taken -- and so a function of the input alone; tests/pair_counts_ref.py restates them by brute force in NumPy.

  the exact layer
    PairContext                 one nwq_ctx: set_cloud once, set_edges and count as often as needed (the cloud and its grid stay on the device)
    pair_counts                 one call: a cloud (or queries and a cloud) and radii in; hist, cumulative and the per-point counts out
  normalisations: host float64 arithmetic on those integers, with no exactness claim and NO EDGE CORRECTION
    ripley                      K, L, H at the radii, and L per localization
    pair_correlation            g(r) on equal bins up to r_max
  recipe-module surfaces
    PairwiseDistanceHistogram   one or two tables -> a table of bin_left bin_right count g
    RipleysK                    a table -> a table of r K L H, and the input plus ripley_local_L

Everything that counts runs on the device; there is no host fallback: without a GPU the context cannot be made and every entry raises.
"""
import ctypes

import numpy as np

from . import _lib

SYMBOLS = ['nwq_abi_version', 'nwq_create', 'nwq_destroy', 'nwq_last_error', 'nwq_set_cloud', 'nwq_set_edges', 'nwq_count']
ABI_VERSION = 1
NWQ_OK, NWQ_ERR_BADARG, NWQ_ERR_HIP, NWQ_ERR_NONFINITE, NWQ_ERR_NOMEM, NWQ_ERR_NOCLOUD = 0, -1, -2, -3, -4, -5
ERRORS = {NWQ_ERR_BADARG: 'bad argument', NWQ_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWQ_ERR_NONFINITE: 'non-finite coordinate',
          NWQ_ERR_NOMEM: 'out of device memory', NWQ_ERR_NOCLOUD: 'the context holds no cloud, or no edges yet'}
NWQ_INFO_WORDS = 8
(NWQ_INFO_TESTS, NWQ_INFO_CELLS_READ, NWQ_INFO_CELL_SIZE, NWQ_INFO_CELLS, NWQ_INFO_VARIANT, NWQ_INFO_N_QUERIES, NWQ_INFO_N_CLOUD, NWQ_INFO_BINS) = range(8)
MAX_N = 1 << 30
MAX_R = 2.0 ** 40
MAX_BINS = 64
NARROW_BINS = 16              # up to here the kernel's bin is the literal sum, above it a search
CELL_OF_RMAX = 0.5            # the cell size a grid starts from, as a share of the largest radius

_L = None


def load():
    """The library's nwq_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        _L = _lib.load_entry_points(SYMBOLS, {
            'nwq_abi_version': [], 'nwq_create': [i32, ctypes.POINTER(vp)], 'nwq_destroy': [vp], 'nwq_last_error': [vp],
            'nwq_set_cloud': [vp, vp, i64, i32], 'nwq_set_edges': [vp, vp, i64], 'nwq_count': [vp, vp, i64, i32, vp, vp, vp]},
            'nwq_abi_version', ABI_VERSION, 'nw_pairs')
    return _L


_p = _lib.ptr
_cloud = _lib.cloud_f32


def _info(words):
    return dict(tests=int(words[NWQ_INFO_TESTS]), cells_read=int(words[NWQ_INFO_CELLS_READ]),
                cell_size=float(words[NWQ_INFO_CELL_SIZE:NWQ_INFO_CELL_SIZE + 1].view(np.float64)[0]), cells=int(words[NWQ_INFO_CELLS]),
                variant='wide' if words[NWQ_INFO_VARIANT] else 'narrow', n_queries=int(words[NWQ_INFO_N_QUERIES]), n_cloud=int(words[NWQ_INFO_N_CLOUD]),
                bins=int(words[NWQ_INFO_BINS]))


class PairContext(_lib.QueryContext):
    """One nwq_ctx: a cloud taken in once by set_cloud and kept on the device with its cell grid, edges set by set_edges, and any number
    of counts of them."""
    prefix, errors, gpu_only, load = 'nwq_', ERRORS, 'pair counting runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_points = 0
        self.n_bins = 0

    def set_cloud(self, points):
        """Take a float32 cloud in: (n,3) on the host, or (device pointer, n)."""
        keep, ptr, n, on_device = _cloud(points)
        self.n_points = 0
        self.check(self.L.nwq_set_cloud(self.h, ptr, n, on_device), 'nwq_set_cloud')
        self.n_points = n
        return self

    def set_edges(self, radii):
        """The radii of the later counts: 1 to 64 of them, finite, 0 <= r_0 < r_1 < ... <= 2^40, their float64 squares ascending too."""
        r = np.ascontiguousarray(radii, np.float64).reshape(-1)
        self.check(self.L.nwq_set_edges(self.h, _p(r), len(r)), 'nwq_set_edges')
        self.n_bins = len(r)
        return self

    def count(self, queries=None, local=False):
        """One count with the cloud and the edges at hand -> dict(hist (m,) uint64, cumulative (m,) uint64, local (n_queries, m) uint32 or
        None, n_queries, n_cloud, info).  queries = None: the cloud against itself, (i, i) left out by index, every unordered pair
        counted from both ends.  Otherwise (nq,3) on the host or (device pointer, nq): every (query, cloud point)."""
        m = self.n_bins
        if queries is None:
            keep, ptr, nq, on_device = None, None, 0, 0
            n_queries = self.n_points
        else:
            keep, ptr, nq, on_device = _cloud(queries)
            n_queries = nq
        hist = np.zeros(max(m, 1), np.uint64)
        loc = np.zeros((n_queries, m), np.uint32) if local else None
        info = np.zeros(NWQ_INFO_WORDS, np.int64)
        self.check(self.L.nwq_count(self.h, ptr, nq, on_device, _p(hist), _p(loc), _p(info)), 'nwq_count')
        hist = hist[:m]
        return dict(hist=hist, cumulative=np.cumsum(hist, dtype=np.uint64), local=loc, n_queries=n_queries, n_cloud=self.n_points, info=_info(info))


def pair_counts(points, edges, other=None, local=False, context=None, device=0):
    """Exact pair-distance counts -> dict(hist, cumulative, local, n_queries, n_cloud, info).
    points: (n,3) on the host or (device pointer, n) of float32 triples.  edges: the radii r_0 < r_1 < ...; hist[b] counts the pairs with
    r_{b-1}^2 < d2 <= r_b^2 (bin 0: d2 <= r_0^2), d2 in float64.  other = None: the ordered pairs (i, j), j != i, of `points` -- every
    unordered pair twice.  other given: `points` are the queries and `other` is the cloud; every (i, j) counts.  local: also the
    (n_queries, m) counts per query, in the caller's order; hist == local.sum(0).  context: a PairContext to use (it holds the cloud and
    the edges afterwards); one is made and closed otherwise."""
    own = context is None
    ctx = PairContext(device) if own else context
    try:
        ctx.set_cloud(points if other is None else other)
        ctx.set_edges(edges)
        return ctx.count(None if other is None else points, local=local)
    finally:
        if own:
            ctx.close()


# ---- normalisations: host float64 on top of the integers ----------------------------------------------------------------------------------
def _host_array(points):
    if isinstance(points, tuple):
        raise ValueError('the bounding box of a device cloud is not read back: give volume=')
    return np.ascontiguousarray(points, np.float32).reshape(-1, 3)


def _window(points, other, dim, volume):
    """the measure of the observation window: `volume`, or the bounding box of the cloud (dim = 2: its x-y rectangle)"""
    if volume is not None:
        v = float(volume)
        if not (v > 0 and np.isfinite(v)):
            raise ValueError('volume must be positive')
        return v
    P = _host_array(points if other is None else other).astype(np.float64)
    ext = (P.max(0) - P.min(0))[:dim]
    if not (ext > 0).all():
        raise ValueError('the cloud has no extent along an axis: its bounding box has no %s, give volume=' % ('area' if dim == 2 else 'volume'))
    return float(np.prod(ext))


def _pairs_total(r):
    return float(r['n_queries']) * float(r['n_cloud'] - 1 if r['auto'] else r['n_cloud'])


def _L_of_K(K, dim):
    return np.sqrt(K / np.pi) if dim == 2 else np.cbrt(3.0 * K / (4.0 * np.pi))


def ripley(points, radii, other=None, dim=3, volume=None, local=False, context=None, device=0):
    """Ripley's K at the radii, with its L and H forms -> dict(r, K, L, H, cumulative, hist, n_pairs, volume, info) and, with local=True,
    L_local (n_queries, m): the Getis-Franklin L of every localization.
        K = V * cumulative / N,   N = n (n - 1) for one cloud, n_A * n_B for `points` (A) against `other` (B)
        dim = 3: L = (3 K / (4 pi))^(1/3);   dim = 2: L = sqrt(K / pi), and V is an area (the counts are of 3-D distances all the same:
        give a flat cloud);   H = L - r
        L_local[i] = the same with K_i = V * cumulative_i / (N / n_queries)
    V defaults to the cloud's bounding box; a box without extent raises and asks for `volume`.
    The counts are exact; this normalisation is host float64 arithmetic and carries no exactness claim.  There is NO EDGE CORRECTION: a
    point near the window's border sees fewer neighbours, so K, L and H are biased low at radii that are not small against the
    window."""
    if dim not in (2, 3):
        raise ValueError('dim is 2 or 3')
    V = _window(points, other, dim, volume)
    r = np.ascontiguousarray(radii, np.float64).reshape(-1)
    c = pair_counts(points, r, other=other, local=local, context=context, device=device)
    c['auto'] = other is None
    N = _pairs_total(c)
    if not N > 0:
        raise ValueError('no pairs: one cloud needs at least two points')
    K = V * c['cumulative'].astype(np.float64) / N
    L = _L_of_K(K, dim)
    out = dict(r=r, K=K, L=L, H=L - r, cumulative=c['cumulative'], hist=c['hist'], n_pairs=N, volume=V, info=c['info'])
    if local:
        Ki = V * np.cumsum(c['local'], axis=1, dtype=np.uint64).astype(np.float64) / (N / c['n_queries'])
        out['L_local'] = _L_of_K(Ki, dim)
        out['local'] = c['local']
    return out


def pair_correlation(points, r_max, n_bins, other=None, dim=3, volume=None, context=None, device=0):
    """The pair correlation g(r) on n_bins equal bins of (0, r_max] -> dict(r_mid, g, hist, edges, n_pairs, volume, info).
        g_b = hist_b * V / (N * shell_b),   shell_b = 4/3 pi (r_b^3 - r_{b-1}^3), or pi (r_b^2 - r_{b-1}^2) for dim = 2
    with V, N and the counting as in ripley.  Coincident pairs (d = 0) fall into the first bin.  The counts are exact; this
    normalisation is host float64 arithmetic and carries no exactness claim.  There is NO EDGE CORRECTION: g is biased low at radii that
    are not small against the window."""
    if dim not in (2, 3):
        raise ValueError('dim is 2 or 3')
    n_bins = int(n_bins)
    if not (1 <= n_bins <= MAX_BINS) or not (float(r_max) > 0):
        raise ValueError('1 to %d bins up to a positive r_max' % MAX_BINS)
    V = _window(points, other, dim, volume)
    edges = np.linspace(0.0, float(r_max), n_bins + 1)
    c = pair_counts(points, edges[1:], other=other, context=context, device=device)
    c['auto'] = other is None
    N = _pairs_total(c)
    if not N > 0:
        raise ValueError('no pairs: one cloud needs at least two points')
    shell = np.pi * np.diff(edges ** 2) if dim == 2 else 4.0 / 3.0 * np.pi * np.diff(edges ** 3)
    g = c['hist'].astype(np.float64) * V / (N * shell)
    return dict(r_mid=0.5 * (edges[1:] + edges[:-1]), g=g, hist=c['hist'], edges=edges, n_pairs=N, volume=V, info=c['info'])


# ---- recipe-module surfaces ---------------------------------------------------------------------------------------------------------------
def _table_points(src):
    return np.ascontiguousarray(np.vstack([src['x'], src['y'], src['z']]).T, np.float32)


class _Recipe(object):
    def __init__(self, **kw):
        self.defaults()
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)


class PairwiseDistanceHistogram(_Recipe):
    """Recipe-module surface for the pair-distance histogram, in the plain-attribute style of the other recipe mirrors, named as PYME's
    module is: the table with x y z under `input` (and, if `input2` is set, a second one: the pairs are then (input, input2)) -> under
    `output` a table of bin_left bin_right count g on n_bins equal bins up to r_max.  PYME is not in the reference tree: the traits and the
    columns here are this project's own.  count is exact; g is pair_correlation's, without edge correction.  The numeric defaults are the
    tested two-cluster scene's, not a recommendation."""

    def defaults(self):
        self.input, self.input2, self.output = 'filtered_localizations', '', 'pair_histogram'
        self.r_max = 50.0
        self.n_bins = 25
        self.dim = 3
        self.volume = None
        self.device = 0

    def execute(self, namespace):
        A = _table_points(namespace[self.input])
        B = _table_points(namespace[self.input2]) if self.input2 else None
        r = pair_correlation(A, float(self.r_max), int(self.n_bins), other=B, dim=int(self.dim), volume=self.volume, device=self.device)
        out = {'bin_left': r['edges'][:-1], 'bin_right': r['edges'][1:], 'count': r['hist'], 'g': r['g'],
               'metadata': {'r_max': float(self.r_max), 'n_bins': int(self.n_bins), 'n_pairs': r['n_pairs'], 'volume': r['volume'], 'info': r['info']}}
        namespace[self.output] = out
        return out


class RipleysK(_Recipe):
    """Recipe-module surface for Ripley's K: the table with x y z under `input` (and, if `input2` is set, a second one) -> under `output` a
    table of r K L H at n_steps radii up to r_max.  With `local_radius` set, `output_local` gets the input's columns plus ripley_local_L,
    the Getis-Franklin L of every localization at that radius: a value column for mapping.SurfaceDensity, which then colours the fit by
    clustering index.  PYME is not in the reference tree: the traits and the columns here are this project's own.  No edge correction (see
    ripley).  The numeric defaults are the tested two-cluster scene's, not a recommendation."""

    def defaults(self):
        self.input, self.input2, self.output, self.output_local = 'filtered_localizations', '', 'ripleys_k', 'ripley_localizations'
        self.r_max = 50.0
        self.n_steps = 25
        self.dim = 3
        self.volume = None
        self.local_radius = None
        self.device = 0

    def execute(self, namespace):
        src = namespace[self.input]
        A = _table_points(src)
        B = _table_points(namespace[self.input2]) if self.input2 else None
        radii = np.linspace(0.0, float(self.r_max), int(self.n_steps) + 1)[1:]
        r = ripley(A, radii, other=B, dim=int(self.dim), volume=self.volume, device=self.device)
        out = {'r': r['r'], 'K': r['K'], 'L': r['L'], 'H': r['H'],
               'metadata': {'r_max': float(self.r_max), 'n_steps': int(self.n_steps), 'n_pairs': r['n_pairs'], 'volume': r['volume'], 'info': r['info']}}
        namespace[self.output] = out
        if self.local_radius is not None:
            one = ripley(A, [float(self.local_radius)], other=B, dim=int(self.dim), volume=r['volume'], local=True, device=self.device)
            loc = {k: src[k] for k in src.keys() if k != 'metadata'}
            loc['ripley_local_L'] = one['L_local'][:, 0]
            loc['metadata'] = {'local_radius': float(self.local_radius), 'volume': r['volume']}
            namespace[self.output_local] = loc
        return out
