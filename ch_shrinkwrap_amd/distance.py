"""
The exact distance from points to a triangle mesh, with a sign for the side: ctypes binding of include/nw_distance.h (kernels in
libnanowrap_hip.so, csrc/nw_distance.hip) and what sits on top of it.

The first thing a user does with a fitted membrane is to ask, for every localization, how far it lies from the surface and on which
side.  Upstream users get that from PYME's `DistanceToMesh` recipe module; PYME is not part of the reference tree, so nothing here
mirrors reference code: the definitions are this project's own and are written down in csrc/nw_distance_core.h (point-triangle
distance in float64 on the float32 vertices, the angle-weighted pseudonormal of the closest feature for the sign; negative inside a
closed mesh whose faces wind counter-clockwise seen from outside, the sign convention of the simulator's shapes).

    DistanceContext     one nwd_ctx: set_mesh once, query as often as needed (the mesh and its cell grid stay on the device)
    distance_to_mesh    one call: points and a mesh in, distances (and closest points, faces) out
    DistanceToMesh      the recipe-module surface: a mesh and a table of localizations -> the table plus two columns

Everything runs on the device; there is no host fallback: without a GPU the context cannot be made and the call raises.
"""
import ctypes

import numpy as np

from . import _lib

SYMBOLS = ['nwd_abi_version', 'nwd_create', 'nwd_destroy', 'nwd_last_error', 'nwd_set_mesh', 'nwd_query']
ABI_VERSION = 1
NWD_OK, NWD_ERR_BADARG, NWD_ERR_HIP, NWD_ERR_NONFINITE, NWD_ERR_NOMEM, NWD_ERR_NOMESH = 0, -1, -2, -3, -4, -5
ERRORS = {NWD_ERR_BADARG: 'bad argument', NWD_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWD_ERR_NONFINITE: 'non-finite coordinate',
          NWD_ERR_NOMEM: 'out of device memory', NWD_ERR_NOMESH: 'the context holds no mesh'}
NWD_SIGNED, NWD_RINGS = 1, 2
FEATURE_MASK, FEATURE_CAPPED = 7, 8           # feature codes: 0 interior, 1-3 edge k, 4-6 vertex k; bit 3: the fan walk was cut short

_L = None


def load():
    """The library's nwd_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        _L = _lib.load_entry_points(SYMBOLS, {
            'nwd_abi_version': [], 'nwd_create': [i32, ctypes.POINTER(vp)], 'nwd_destroy': [vp], 'nwd_last_error': [vp],
            'nwd_set_mesh': [vp, vp, i64, vp, i64, vp],
            'nwd_query': [vp, vp, i64, i32, vp, vp, vp, vp, ctypes.POINTER(f64)]},
            'nwd_abi_version', ABI_VERSION, 'nw_distance')
    return _L


_p = _lib.ptr


def _points(points):
    """-> (what keeps the memory alive, pointer, n): an (n,3) array (copied to float64 if it is not) or (device pointer, n)"""
    if isinstance(points, tuple) and len(points) == 2 and isinstance(points[0], (int, np.integer)):
        return None, _p(int(points[0])), int(points[1])
    a = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    return a, _p(a), a.shape[0]


def mesh_twins(faces, n_vertices):
    """twin[3f+k] of an oriented face array (-1 on a border): the remesher's linear-time pairing (nwr_halfedge_twins).  A face array
    with a non-manifold edge has no twin table and no sides: the pairing's error is passed on (query it with signed=False)."""
    from .remesh import halfedge_twins
    return halfedge_twins(faces, n_vertices)


def _mesh_arrays(mesh, need_twin):
    """(positions float32, faces int32, twin or None) of a TriMesh / MembraneMesh or a (vertices, faces) pair"""
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        pos, faces = _lib.mesh_arrays(mesh[0], mesh[1])
        return pos, faces, (mesh_twins(faces, pos.shape[0]) if need_twin else None)
    pos, faces = _lib.mesh_arrays(mesh.vertices if hasattr(mesh, 'vertices') else mesh._vertices['position'], mesh.faces)
    twin = None
    if need_twin:
        he = getattr(mesh, '_halfedges', None)                    # the half-edge substrate, if the mesh has one with twins in it
        names = getattr(getattr(he, 'dtype', None), 'names', None) or ()
        if he is not None and 'twin' in names and len(he) == 3 * faces.shape[0]:
            twin = np.ascontiguousarray(he['twin'], np.int32)
            h = np.flatnonzero(twin >= 0)
            if (twin < -1).any() or (twin >= twin.size).any() or (twin[twin[h]] != h).any():
                # (TriMesh pairs a face array the native pairing rejects by sorting, which need not be mutual)
                raise ValueError('distance_to_mesh: the mesh has a non-manifold edge (its half-edge twins are not mutual), so it has no '
                                 'sides; query it with signed=False')
        else:
            twin = mesh_twins(faces, pos.shape[0])
    return pos, faces, twin


class DistanceContext(_lib.QueryContext):
    """One nwd_ctx: a mesh taken in once by set_mesh, its centroid grid kept on the device, and any number of queries against it."""
    prefix, errors, gpu_only, load = 'nwd_', ERRORS, 'the distance to a mesh runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_faces = 0
        self.has_twin = False

    def set_mesh(self, vertices, faces, twin=None):
        """Take a float32 mesh in.  twin: int32 (3F,), -1 on a border; None for a mesh that is only queried unsigned."""
        pos, faces = _lib.mesh_arrays(vertices, faces)
        tw = None if twin is None else np.ascontiguousarray(twin, np.int32).ravel()
        if tw is not None and tw.size != 3 * faces.shape[0]:
            raise ValueError('twin must have three entries per face')
        self.n_faces, self.has_twin = 0, False
        self.check(self.L.nwd_set_mesh(self.h, _p(pos), pos.shape[0], _p(faces), faces.shape[0], _p(tw)), 'nwd_set_mesh')
        self.n_faces, self.has_twin = faces.shape[0], tw is not None
        return self

    def query(self, points, signed=True, return_closest=False, return_face=False, return_feature=False, return_sum=False, rings=False):
        """Distances (n,) float64 of `points` ((n,3) on the host, or (device pointer, n)) from the mesh, signed if asked (negative
        inside).  With any return_* flag a tuple: (dist[, closest (n,3)][, face (n,) int32][, feature (n,) int32][, sum of dist^2]).
        rings=True: the feature codes carry the ring at which each walk ended in bits 8..15."""
        keep, ptr, n = _points(points)
        dist = np.empty(n, np.float64)
        closest = np.empty((n, 3), np.float64) if return_closest else None
        face = np.empty(n, np.int32) if return_face else None
        feature = np.empty(n, np.int32) if return_feature else None
        s = ctypes.c_double()
        if n:
            flags = (NWD_SIGNED if signed else 0) | (NWD_RINGS if rings else 0)
            self.check(self.L.nwd_query(self.h, ptr, n, flags, _p(dist), _p(closest), _p(face), _p(feature), ctypes.byref(s)), 'nwd_query')
        out = (dist,) + tuple(a for a in (closest, face, feature) if a is not None) + ((float(s.value),) if return_sum else ())
        return out if len(out) > 1 else dist


def distance_to_mesh(points, mesh, signed=True, return_closest=False, return_face=False, context=None, device=0):
    """The exact distance of every point from the mesh's triangles: dist (n,) float64, negative inside with signed=True; with
    return_closest / return_face a tuple (dist[, closest (n,3) float64][, face (n,) int32]).
    points: (n,3) on the host, or (device pointer, n) of float64 triples.  mesh: a TriMesh / MembraneMesh or (vertices, faces); the
    twin table a sign needs comes from the mesh's half-edge records or from nwr_halfedge_twins; a mesh with a non-manifold edge has
    none and raises with signed=True.  context: a DistanceContext to use (it
    holds this mesh afterwards); one is made and closed otherwise."""
    pos, faces, twin = _mesh_arrays(mesh, signed)
    own = context is None
    ctx = DistanceContext(device) if own else context
    try:
        ctx.set_mesh(pos, faces, twin)
        return ctx.query(points, signed=signed, return_closest=return_closest, return_face=return_face)
    finally:
        if own:
            ctx.close()


class DistanceToMesh(object):
    """Recipe-module surface for the distance of localizations from a fitted surface, in the plain-attribute style of
    ShrinkwrapMembrane: the mesh under `input_mesh` and a table with x y z under `input_points` -> under `output` the table's columns
    plus `distance_to_mesh` (nm, negative inside with signed=True) and `closest_face`.
    PYME has a module of this name, but PYME is not in the reference tree: the traits, the sign convention and the columns here are
    this project's own, not a mirror of upstream code."""

    def __init__(self, **kw):
        self.input_mesh, self.input_points, self.output = 'membrane', 'filtered_localizations', 'distances'
        self.signed = True
        self.device = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)

    def execute(self, namespace):
        src = namespace[self.input_points]
        pts = np.ascontiguousarray(np.vstack([src['x'], src['y'], src['z']]).T, np.float64)
        dist, face = distance_to_mesh(pts, namespace[self.input_mesh], signed=bool(self.signed), return_face=True, device=self.device)
        table = {k: src[k] for k in src.keys()}
        table['distance_to_mesh'] = dist
        table['closest_face'] = face
        namespace[self.output] = table
        return table
