"""
Which pairs of faces of a mesh cross each other: ctypes binding of include/nw_intersections.h (kernels in libnanowrap_hip.so,
csrc/nw_intersections.hip) and what sits on top of it.

"Closed and manifold" are statements about the face array; a surface can be both and still pass through itself.  This is the check
of the third property, embedded.  PYME is not part of the reference tree, so nothing here mirrors reference code: the definition is
this project's own and is written down in csrc/nw_intersections_core.h (a crossing is proper: the interior of an edge of one face
passes through the interior of the other; touching, coplanar overlap and faces sharing an edge are none; float64 on the float32
positions).

    IntersectionContext   one nwx_ctx: set_mesh, then find; may be kept across calls (its buffers stay on the device)
    self_intersections    one call: a mesh in, dict(n_pairs, n_faces, count, pairs) out

Everything runs on the device; there is no host fallback: without a GPU the context cannot be made and the call raises.
"""
import ctypes

import numpy as np

from . import _lib

SYMBOLS = ['nwx_abi_version', 'nwx_create', 'nwx_destroy', 'nwx_last_error', 'nwx_set_mesh', 'nwx_find', 'nwx_get_pairs', 'nwx_get_stats']
ABI_VERSION = 1
NWX_OK, NWX_ERR_BADARG, NWX_ERR_HIP, NWX_ERR_NONFINITE, NWX_ERR_NOMEM, NWX_ERR_NOMESH, NWX_ERR_TOOMANY, NWX_ERR_NOPAIRS = 0, -1, -2, -3, -4, -5, -6, -7
ERRORS = {NWX_ERR_BADARG: 'bad argument', NWX_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWX_ERR_NONFINITE: 'non-finite coordinate',
          NWX_ERR_NOMEM: 'out of device memory', NWX_ERR_NOMESH: 'the context holds no mesh', NWX_ERR_TOOMANY: 'more pairs than the unit lists',
          NWX_ERR_NOPAIRS: 'the context holds no list of pairs'}
NWX_PAIRS, NWX_STATS = 1, 2
NWX_MAX_PAIRS = 1 << 24

_L = None


def load():
    """The library's nwx_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        _L = _lib.load_entry_points(SYMBOLS, {
            'nwx_abi_version': [], 'nwx_create': [i32, ctypes.POINTER(vp)], 'nwx_destroy': [vp], 'nwx_last_error': [vp],
            'nwx_set_mesh': [vp, vp, i64, vp, i64],
            'nwx_find': [vp, i32, vp, ctypes.POINTER(i64), ctypes.POINTER(i64)],
            'nwx_get_pairs': [vp, vp, i64], 'nwx_get_stats': [vp, vp]},
            'nwx_abi_version', ABI_VERSION, 'nw_intersections')
    return _L


_p = _lib.ptr


def _mesh_arrays(mesh):
    """(positions float32, faces int32) of a TriMesh / MembraneMesh or a (vertices, faces) pair"""
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        return _lib.mesh_arrays(mesh[0], mesh[1])
    return _lib.mesh_arrays(mesh.vertices if hasattr(mesh, 'vertices') else mesh._vertices['position'], mesh.faces)


class IntersectionContext(_lib.QueryContext):
    """One nwx_ctx: a mesh taken in by set_mesh, its centroid grid kept on the device, and find() against it."""
    prefix, errors, gpu_only, load = 'nwx_', ERRORS, 'the self-intersection check runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_faces = 0

    def set_mesh(self, vertices, faces):
        pos, faces = _lib.mesh_arrays(vertices, faces)
        self.n_faces = 0
        self.check(self.L.nwx_set_mesh(self.h, _p(pos), pos.shape[0], _p(faces), faces.shape[0]), 'nwx_set_mesh')
        self.n_faces = faces.shape[0]
        return self

    def find(self, return_pairs=True, return_count=True, stats=False):
        """dict(n_pairs, n_faces (the crossed ones), count (F,) int32 or None, pairs (n_pairs, 2) int32 sorted by (f, g), f < g, or None);
        with stats=True also candidates / tested: the ordered pairs of faces whose centroids were read, and those that reached the
        predicate.  A mesh with more than NWX_MAX_PAIRS pairs has its counts and pairs=None."""
        count = np.empty(self.n_faces, np.int32) if return_count else None
        n_pairs, n_crossed = ctypes.c_int64(), ctypes.c_int64()
        code = self.L.nwx_find(self.h, (NWX_PAIRS if return_pairs else 0) | (NWX_STATS if stats else 0), _p(count), ctypes.byref(n_pairs),
                               ctypes.byref(n_crossed))
        if code != NWX_ERR_TOOMANY:
            self.check(code, 'nwx_find')
        out = dict(n_pairs=int(n_pairs.value), n_faces=int(n_crossed.value), count=count, pairs=None)
        if return_pairs and code == NWX_OK:
            pairs = np.empty((out['n_pairs'], 2), np.int32)
            self.check(self.L.nwx_get_pairs(self.h, _p(pairs), pairs.shape[0]), 'nwx_get_pairs')
            out['pairs'] = pairs
        if stats:
            st = np.zeros(2, np.int64)
            self.check(self.L.nwx_get_stats(self.h, _p(st)), 'nwx_get_stats')
            out['candidates'], out['tested'] = int(st[0]), int(st[1])
        return out


def self_intersections(mesh, return_pairs=True, context=None, device=0):
    """The proper crossings of a mesh with itself: dict(n_pairs, n_faces, count, pairs) -- the number of unordered pairs of faces that
    cross, the number of faces in one, per face the number of faces it crosses, and (return_pairs) the pairs (n_pairs, 2) int32,
    f < g, sorted.  mesh: a TriMesh / MembraneMesh or (vertices, faces).  context: an IntersectionContext to use (it holds this mesh
    afterwards); one is made and closed otherwise."""
    pos, faces = _mesh_arrays(mesh)
    own = context is None
    ctx = IntersectionContext(device) if own else context
    try:
        return ctx.set_mesh(pos, faces).find(return_pairs=return_pairs)
    finally:
        if own:
            ctx.close()
