"""
Distance along the fitted membrane: the geodesic graph distance of every vertex of a mesh from a set of source vertices, and which source
it belongs to.  ctypes binding of include/nw_geodesic.h (kernels in libnanowrap_hip.so, csrc/nw_geodesic.hip) and what sits on top of it.

Every other query of this package measures through space; a straight line cuts through the lumen and across the gap between two sheets.
What is asked of a fitted membrane is usually measured along it: how far along the ER a vertex is from the nearest contact site, how a
density falls off with that distance, which contact site a piece of membrane belongs to.  Upstream answers by skeletonisation; PYME is not
part of the reference tree and has no such module, so nothing here mirrors reference code: the definition is this project's own and is
written down in csrc/nw_geodesic_core.h; tests/mesh_geodesic_ref.py restates it in NumPy.

THIS IS A GRAPH DISTANCE WITH ONE LEVEL OF UNFOLDING, NOT AN EXACT POLYHEDRAL GEODESIC (no MMP, no heat method).  The arcs are the mesh's
edges and, with diagonals=True, across every interior edge the straight segment between the two opposite corners where it stays inside the
two unfolded faces.  Every value is the length of a real path on the surface: never below the Euclidean distance, and an upper bound of
the true geodesic.  On geodesic_sphere(12, 100) from one vertex, tests/test_mesh_geodesic_ref.py measures D / (R angle): at most 1.0415
(mean 1.0148) with diagonals, at most 1.2167 (mean 1.0824) on the edges alone.  "Exact" means: a function of the input alone, equal bit
for bit to the restatement, whatever the launch geometry, the batch size or the order of the faces.

  the exact layer
    GeodesicContext       one nwt_ctx: set_mesh once (the weights stay on the device), distances as often as needed
    geodesic_distance     one call: a mesh and sources in; distance, source and info out
    sources_from_faces    the vertices of a face mask or of face patch labels: contact_sites(a, b)['faces_a' / 'patches_a'] feed it directly
  on top of it: host float64 arithmetic with no exactness claim
    surface_profile       the area-weighted mean of a per-vertex value in bins of the distance
  recipe-module surface
    GeodesicDistance      a mesh and sources -> a table of x y z geodesic_distance nearest_source

Everything that relaxes runs on the device; there is no host fallback: without a GPU the context cannot be made and every entry raises.
"""
import ctypes

import numpy as np

from . import _lib

SYMBOLS = ['nwt_abi_version', 'nwt_create', 'nwt_destroy', 'nwt_last_error', 'nwt_set_mesh', 'nwt_distances']
ABI_VERSION = 1
NWT_OK, NWT_ERR_BADARG, NWT_ERR_HIP, NWT_ERR_NONFINITE, NWT_ERR_NOMEM, NWT_ERR_NOMESH, NWT_ERR_INTERNAL = 0, -1, -2, -3, -4, -5, -6
ERRORS = {NWT_ERR_BADARG: 'bad argument', NWT_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWT_ERR_NONFINITE: 'non-finite position',
          NWT_ERR_NOMEM: 'out of device memory', NWT_ERR_NOMESH: 'the context holds no mesh yet',
          NWT_ERR_INTERNAL: 'the rounds did not reach a fixed point'}
NWT_FLAG_DIAGONALS = 1
NWT_INFO_WORDS = 10
(NWT_INFO_HALFEDGES, NWT_INFO_DIAGONALS, NWT_INFO_REACHED, NWT_INFO_IN_BAND, NWT_INFO_ROUNDS, NWT_INFO_LABEL_ROUNDS, NWT_INFO_LAUNCHES,
 NWT_INFO_LOWERED, NWT_INFO_RELAXED, NWT_INFO_BATCH) = range(10)
MAX_N = 1 << 30
MAX_FACES = 1 << 29
BATCH = 16                    # rounds per read of the changed words: a first choice, unmeasured (csrc/nw_geodesic_core.h)
SWEEPS = 4                    # a workgroup's sweeps within a round: likewise
# the info entries that depend on the order in which the hardware runs workgroups: in no bit comparison
NOT_DETERMINISTIC = ('rounds', 'label_rounds', 'launches', 'lowered', 'relaxed')

_L = None


def load():
    """The library's nwt_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        _L = _lib.load_entry_points(SYMBOLS, {
            'nwt_abi_version': [], 'nwt_create': [i32, ctypes.POINTER(vp)], 'nwt_destroy': [vp], 'nwt_last_error': [vp],
            'nwt_set_mesh': [vp, vp, i64, vp, i64, vp, i32], 'nwt_distances': [vp, vp, vp, i64, f64, i32, vp, vp, vp]},
            'nwt_abi_version', ABI_VERSION, 'nw_geodesic')
    return _L


_p = _lib.ptr


def _info(words):
    return dict(halfedges=int(words[NWT_INFO_HALFEDGES]), diagonals=int(words[NWT_INFO_DIAGONALS]), reached=int(words[NWT_INFO_REACHED]),
                in_band=int(words[NWT_INFO_IN_BAND]), rounds=int(words[NWT_INFO_ROUNDS]), label_rounds=int(words[NWT_INFO_LABEL_ROUNDS]),
                launches=int(words[NWT_INFO_LAUNCHES]), lowered=int(words[NWT_INFO_LOWERED]), relaxed=int(words[NWT_INFO_RELAXED]),
                batch=int(words[NWT_INFO_BATCH]))


def _source_ids(sources, n_vertices):
    """vertex ids (int32) of an id array or of a boolean vertex mask"""
    s = np.asarray(sources)
    if s.dtype == np.bool_:
        if s.shape != (n_vertices,):
            raise ValueError('a source mask has one entry per vertex')
        s = np.flatnonzero(s)
    elif s.size and not np.issubdtype(s.dtype, np.integer):
        raise ValueError('sources are vertex ids or a boolean vertex mask')
    s = np.ascontiguousarray(s, np.int64).reshape(-1)
    if s.size < 1:
        raise ValueError('at least one source')
    if (s < 0).any() or (s >= n_vertices).any():
        raise ValueError('a source id is out of range')
    return s.astype(np.int32)


class GeodesicContext(_lib.QueryContext):
    """One nwt_ctx: a mesh taken in once by set_mesh, its edge and diagonal weights kept on the device, and any number of distance
    fields on it."""
    prefix, errors, gpu_only, load = 'nwt_', ERRORS, 'the distance along a mesh runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_vertices = 0
        self.has_twin = False

    def set_mesh(self, vertices, faces, twin=None):
        """Take a float32 mesh in.  vertices: (V,3) on the host, or (device pointer, V).  twin: int32 (3F,), -1 on a border, mutual; with
        it the context's distances use the face diagonals, without it (None) the plain edge graph, which a face array with a
        non-manifold edge has too."""
        if isinstance(vertices, tuple) and len(vertices) == 2 and isinstance(vertices[0], (int, np.integer)):
            pos, n, on_device = _p(int(vertices[0])), int(vertices[1]), 1
        else:
            keep = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
            pos, n, on_device = _p(keep), keep.shape[0], 0
        faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        tw = None if twin is None else np.ascontiguousarray(twin, np.int32).ravel()
        if tw is not None and tw.size != 3 * faces.shape[0]:
            raise ValueError('twin must have three entries per face')
        self.n_vertices, self.has_twin = 0, False
        self.check(self.L.nwt_set_mesh(self.h, pos, n, _p(faces), faces.shape[0], _p(tw), on_device), 'nwt_set_mesh')
        self.n_vertices, self.has_twin = n, tw is not None
        return self

    def distances(self, sources, d0=None, max_distance=np.inf, labels=False):
        """One distance field on the mesh at hand -> dict(distance (V,) float64, source (V,) int32 or None, info).
        sources: vertex ids (duplicates allowed) or a boolean vertex mask.  d0: a start value per source, finite and >= 0 (None: zeros).
        max_distance: vertices farther than this get +inf, and nothing is relaxed from beyond it; no value at or below it changes.
        labels: also source[v], the index into `sources` (for a mask: into its set vertices, ascending) of the source v belongs to: the
        smallest index from which a walk of tight arcs (fl(D[u] + w) == D[v]) leads to v; -1 where the distance is +inf.  With rounded
        sums that rule need not agree with "the source of some shortest walk"; the rule is what is computed.
        This is a graph distance with one level of unfolding (module docstring), not an exact polyhedral geodesic.
        info: halfedges, diagonals, reached, in_band are functions of the input; rounds, label_rounds, launches, lowered and relaxed
        depend on the hardware's scheduling, ARE NOT DETERMINISTIC and belong in no comparison (NOT_DETERMINISTIC)."""
        if not self.n_vertices:
            raise RuntimeError('nwt_distances: %s' % ERRORS[NWT_ERR_NOMESH])
        ids = _source_ids(sources, self.n_vertices)
        start = None
        if d0 is not None:
            start = np.ascontiguousarray(d0, np.float64).reshape(-1)
            if start.size != ids.size:
                raise ValueError('d0 has one value per source')
        dist = np.empty(max(self.n_vertices, 1), np.float64)
        src = np.empty(max(self.n_vertices, 1), np.int32) if labels else None
        info = np.zeros(NWT_INFO_WORDS, np.int64)
        self.check(self.L.nwt_distances(self.h, _p(ids), _p(start), ids.size, float(max_distance), NWT_FLAG_DIAGONALS if self.has_twin else 0, _p(dist), _p(src),
                                        _p(info)), 'nwt_distances')
        return dict(distance=dist[:self.n_vertices], source=None if src is None else src[:self.n_vertices], info=_info(info))


def geodesic_distance(mesh, sources, d0=None, max_distance=np.inf, diagonals=True, labels=False, context=None, device=0):
    """The distance of every vertex from the sources along the mesh -> dict(distance, source, info) (GeodesicContext.distances).
    mesh: a TriMesh, a MembraneMesh or a (vertices, faces) pair.  sources: vertex ids or a boolean vertex mask.
    diagonals=True adds, across every interior edge, the segment between the two opposite corners where it stays inside the two unfolded
    faces; it needs the half-edge twins, so a mesh with a non-manifold edge raises (as distance_to_mesh(signed=True) does).
    diagonals=False is the plain edge graph and works on any face array.
    A graph distance with one level of unfolding, NOT an exact polyhedral geodesic: an upper bound of it, never below the Euclidean
    distance; the measured overestimate on a sphere is in the module docstring.
    context: a GeodesicContext to use (it holds the mesh afterwards); one is made and closed otherwise."""
    from .distance import _mesh_arrays
    pos, faces, twin = _mesh_arrays(mesh, bool(diagonals))
    own = context is None
    ctx = GeodesicContext(device) if own else context
    try:
        return ctx.set_mesh(pos, faces, twin).distances(sources, d0=d0, max_distance=max_distance, labels=labels)
    finally:
        if own:
            ctx.close()


def sources_from_faces(faces, face_mask_or_labels):
    """(vertex ids ascending (int32), the patch of each) of the faces a mask or a label array picks: a bool (F,) mask picks its set
    faces (patch 0 for all), an integer (F,) array the faces with a label >= 0 (a vertex of several patches gets the smallest).
    contact_sites(a, b)['faces_a'] and ['patches_a'] are such arrays for mesh a."""
    faces = np.asarray(faces).reshape(-1, 3)
    m = np.asarray(face_mask_or_labels).reshape(-1)
    if m.shape[0] != faces.shape[0]:
        raise ValueError('one entry per face')
    if m.dtype == np.bool_:
        pick, lab = m, np.zeros(m.shape[0], np.int64)
    else:
        pick, lab = m >= 0, m.astype(np.int64)
    v = faces[pick].reshape(-1)
    ids, inv = np.unique(v, return_inverse=True)
    patch = np.full(ids.size, np.iinfo(np.int64).max)
    np.minimum.at(patch, inv.reshape(-1), np.repeat(lab[pick], 3))
    return ids.astype(np.int32), patch.astype(np.int32)


def surface_profile(distance, values, area, edges):
    """The area-weighted mean of a per-vertex value (density, curvature, thickness) in bins of the distance along the mesh
    -> (r_mid, mean, area_in_bin, n_vertices).  Bin b holds the vertices with edges[b] <= distance < edges[b + 1] (the last bin is closed);
    vertices at +inf, with a non-finite value or outside the edges are left out; mean is nan for a bin without area.
    Host float64 arithmetic on top of the field: no exactness claim."""
    d = np.asarray(distance, np.float64).reshape(-1)
    x = np.asarray(values, np.float64).reshape(-1)
    a = np.asarray(area, np.float64).reshape(-1)
    e = np.asarray(edges, np.float64).reshape(-1)
    if not (d.shape == x.shape == a.shape) or e.size < 2 or not (np.diff(e) > 0).all():
        raise ValueError('distance, values and area per vertex, and at least two ascending edges')
    b = np.searchsorted(e, d, side='right') - 1
    b[d == e[-1]] = e.size - 2
    ok = np.isfinite(d) & np.isfinite(x) & np.isfinite(a) & (b >= 0) & (b < e.size - 1)
    nb = e.size - 1
    area_in_bin = np.bincount(b[ok], weights=a[ok], minlength=nb)
    total = np.bincount(b[ok], weights=(a * x)[ok], minlength=nb)
    n = np.bincount(b[ok], minlength=nb)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(area_in_bin > 0, total / area_in_bin, np.nan)
    return 0.5 * (e[1:] + e[:-1]), mean, area_in_bin, n


# ---- recipe-module surface ----------------------------------------------------------------------------------------------------------------
class GeodesicDistance(object):
    """Recipe-module surface for the distance along a fit, in the plain-attribute style of the other recipe mirrors: the mesh under
    `input_mesh` and the sources under `input_sources` -> under `output` a table with one row per vertex: x y z geodesic_distance
    (+inf beyond max_distance or where no source reaches) nearest_source (the vertex id of the source the vertex belongs to, -1 for none).
    `input_sources` names one of: a contact-sites result (proximity.contact_sites; its patches_<side> are the sources), a table whose
    column `source_column` has one entry per vertex or per face (non-zero: a source; per face: all three corners), or such an array.
    The table's metadata carries source_vertices and source_patch.  PYME is not in the reference tree: the traits and the columns here
    are this project's own.  A graph distance with one level of unfolding, not an exact polyhedral geodesic (see geodesic_distance)."""

    def __init__(self, **kw):
        self.input_mesh, self.input_sources, self.output = 'membrane', 'contacts', 'geodesic_distances'
        self.source_column = 'source'
        self.side = 'a'
        self.max_distance = np.inf
        self.diagonals = True
        self.device = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)

    def _sources(self, src, n_vertices, faces):
        if isinstance(src, dict) and 'patches_' + self.side in src:
            return sources_from_faces(faces, src['patches_' + self.side])
        col = np.asarray(src[self.source_column] if isinstance(src, dict) else src).reshape(-1)
        if col.shape[0] == n_vertices:
            ids = np.flatnonzero(col != 0).astype(np.int32)
            return ids, np.zeros(ids.size, np.int32)
        if col.shape[0] == faces.shape[0]:
            return sources_from_faces(faces, col != 0)
        raise ValueError('the sources have one entry per vertex or per face')

    def execute(self, namespace):
        from .distance import _mesh_arrays
        mesh = namespace[self.input_mesh]
        pos, faces, _ = _mesh_arrays(mesh, False)
        ids, patch = self._sources(namespace[self.input_sources], pos.shape[0], faces)
        r = geodesic_distance(mesh, ids, max_distance=float(self.max_distance), diagonals=bool(self.diagonals), labels=True, device=self.device)
        nearest = np.where(r['source'] >= 0, ids[np.maximum(r['source'], 0)], -1).astype(np.int32)
        out = {'x': pos[:, 0], 'y': pos[:, 1], 'z': pos[:, 2], 'geodesic_distance': r['distance'], 'nearest_source': nearest,
               'metadata': {'max_distance': float(self.max_distance), 'diagonals': bool(self.diagonals), 'source_vertices': ids, 'source_patch': patch,
                            'info': r['info']}}
        namespace[self.output] = out
        return out
