"""
Rays against a triangle mesh, exactly: ctypes binding of include/nw_rays.h (kernels in libnanowrap_hip.so, csrc/nw_rays.hip) and what
sits on top of it -- the local thickness of a fitted surface and a parity test for a point's side.

How wide a fitted structure is at a place (a tube's diameter, a sheet's thickness, the gap to the next membrane) is the length of a
ray along the inward normal to the first face it meets, the "shape diameter".  Upstream answers the question with
SkeletonizeMembrane, which is out of this project's scope; PYME is not part of the reference tree, so nothing here
mirrors reference code: the definition of a hit is this project's own and is written down in csrc/nw_rays_core.h (an inclusive edge
test, so that no ray leaks through an edge or a vertex of a closed mesh; float64 on the float32 positions).

    RayContext       one nwc_ctx: set_mesh once, cast as often as needed (the mesh and its cell grid stay on the device)
    cast_rays        one call: a mesh and rays in, dict(t, face, exits, hits) out
    thickness        per vertex, the median length of rays inside a cone about the inward (or outward) normal
    inside           the parity of the faces hit along one fixed direction: a third way to a point's side, next to the sign of
                     distance.distance_to_mesh and to the winding number of surgery.py
    MeshThickness    the recipe-module surface: a mesh -> a table x y z thickness n_valid

Everything runs on the device; there is no host fallback: without a GPU the context cannot be made and the call raises.
"""
import ctypes

import numpy as np

from . import _lib

SYMBOLS = ['nwc_abi_version', 'nwc_create', 'nwc_destroy', 'nwc_last_error', 'nwc_set_mesh', 'nwc_cast', 'nwc_get_stats']
ABI_VERSION = 1
NWC_OK, NWC_ERR_BADARG, NWC_ERR_HIP, NWC_ERR_NONFINITE, NWC_ERR_NOMEM, NWC_ERR_NOMESH = 0, -1, -2, -3, -4, -5
ERRORS = {NWC_ERR_BADARG: 'bad argument', NWC_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWC_ERR_NONFINITE: 'non-finite coordinate',
          NWC_ERR_NOMEM: 'out of device memory', NWC_ERR_NOMESH: 'the context holds no mesh'}
NWC_COUNT, NWC_STATS = 1, 2
NWC_INFO_EXITS = 1
MAX_RAYS_PER_CALL = 1 << 22                   # thickness() and inside() build their rays on the host in chunks of at most this many
# the direction of inside(): fixed, of unit length and along no axis, no face diagonal and no space diagonal of a lattice
DEFAULT_DIRECTION = (0.3143, 0.5377, 0.7823)

_L = None


def load():
    """The library's nwc_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        _L = _lib.load_entry_points(SYMBOLS, {
            'nwc_abi_version': [], 'nwc_create': [i32, ctypes.POINTER(vp)], 'nwc_destroy': [vp], 'nwc_last_error': [vp],
            'nwc_set_mesh': [vp, vp, i64, vp, i64],
            'nwc_cast': [vp, vp, vp, i64, vp, vp, f64, i32, vp, vp, vp, vp],
            'nwc_get_stats': [vp, vp]},
            'nwc_abi_version', ABI_VERSION, 'nw_rays')
    return _L


_p = _lib.ptr


def _triples(a):
    """-> (what keeps the memory alive, pointer, n): an (n,3) array (copied to float64 if it is not) or (device pointer, n)"""
    if isinstance(a, tuple) and len(a) == 2 and isinstance(a[0], (int, np.integer)):
        return None, _p(int(a[0])), int(a[1])
    a = np.ascontiguousarray(a, np.float64).reshape(-1, 3)
    return a, _p(a), a.shape[0]


def _ids(a, n, what):
    """-> (what keeps the memory alive, pointer): None, an (n,) array (copied to int32 if it is not) or a raw device pointer"""
    if a is None:
        return None, None
    if isinstance(a, (int, np.integer)):
        return None, _p(int(a))
    a = np.ascontiguousarray(a, np.int32).ravel()
    if a.size != n:
        raise ValueError('%s must have one entry per ray' % what)
    return a, _p(a)


def _mesh_arrays(mesh):
    """(positions float32, faces int32) of a TriMesh / MembraneMesh or a (vertices, faces) pair"""
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        return _lib.mesh_arrays(mesh[0], mesh[1])
    return _lib.mesh_arrays(mesh.vertices if hasattr(mesh, 'vertices') else mesh._vertices['position'], mesh.faces)


class RayContext(_lib.QueryContext):
    """One nwc_ctx: a mesh taken in once by set_mesh, its centroid grid kept on the device, and any number of casts against it."""
    prefix, errors, gpu_only, load = 'nwc_', ERRORS, 'ray casting runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_faces = 0

    def set_mesh(self, vertices, faces):
        pos, faces = _lib.mesh_arrays(vertices, faces)
        self.n_faces = 0
        self.check(self.L.nwc_set_mesh(self.h, _p(pos), pos.shape[0], _p(faces), faces.shape[0]), 'nwc_set_mesh')
        self.n_faces = faces.shape[0]
        return self

    def cast(self, origins, directions, skip_vertex=None, skip_face=None, t_max=np.inf, count=False, stats=False):
        """dict(t (n,) float64: the parameter of the nearest hit along `directions` (of any finite length), +inf for a miss; face (n,) int32,
        -1 for a miss; exits (n,) bool: the ray leaves through the back of that face; hits (n,) int32: the faces hit, with count=True,
        else None).  origins, directions: (n,3) on the host or (device pointer, n) of float64 triples; skip_vertex, skip_face: per ray
        the id of a vertex whose faces, and of a face, that the ray passes over (-1 for none), (n,) on the host, a raw device pointer
        or None.  With stats=True also pieces / centroids / tested: the walk's three counters summed over the rays."""
        keep_o, po, n = _triples(origins)
        keep_d, pd, nd = _triples(directions)
        if nd != n:
            raise ValueError('origins and directions must have one row per ray each')
        keep_v, pv = _ids(skip_vertex, n, 'skip_vertex')
        keep_f, pf = _ids(skip_face, n, 'skip_face')
        t, face, info = np.full(n, np.inf), np.full(n, -1, np.int32), np.zeros(n, np.int32)
        hits = np.zeros(n, np.int32) if count else None
        if n:
            flags = (NWC_COUNT if count else 0) | (NWC_STATS if stats else 0)
            self.check(self.L.nwc_cast(self.h, po, pd, n, pv, pf, float(t_max), flags, _p(t), _p(face), _p(info), _p(hits)), 'nwc_cast')
        out = dict(t=t, face=face, exits=(info & NWC_INFO_EXITS) != 0, hits=hits)
        if stats:
            st = np.zeros(3, np.int64)
            self.check(self.L.nwc_get_stats(self.h, _p(st)), 'nwc_get_stats')
            out['pieces'], out['centroids'], out['tested'] = int(st[0]), int(st[1]), int(st[2])
        return out


def cast_rays(mesh, origins, directions, skip_vertex=None, skip_face=None, t_max=np.inf, count=False, context=None, device=0):
    """RayContext.cast in one call.  mesh: a TriMesh / MembraneMesh or (vertices, faces).  context: a RayContext to use (it holds this
    mesh afterwards); one is made and closed otherwise."""
    pos, faces = _mesh_arrays(mesh)
    own = context is None
    ctx = RayContext(device) if own else context
    try:
        return ctx.set_mesh(pos, faces).cast(origins, directions, skip_vertex, skip_face, t_max, count)
    finally:
        if own:
            ctx.close()


def cone_directions(axis, n_rays, cone_angle):
    """(n, n_rays, 3) unit directions inside the cone of full opening angle `cone_angle` (degrees) about each unit `axis` (n,3):
    a spherical-Fibonacci cap, cos theta_k = 1 - (k + 1/2) / K (1 - cos(cone_angle / 2)), phi_k = k pi (3 - sqrt 5), k = 0 .. K - 1,
    in the frame (u, w, axis) with u = e - (e.axis) axis normalised, e the coordinate axis of the axis's smallest component in
    magnitude (the first of equals), and w = axis x u.  n_rays = 1 gives the axis itself."""
    axis = np.asarray(axis, np.float64).reshape(-1, 3)
    K = int(n_rays)
    if K == 1:
        return axis[:, None, :].copy()
    k = np.arange(K, dtype=np.float64)
    ct = 1.0 - (k + 0.5) / K * (1.0 - np.cos(np.radians(0.5 * float(cone_angle))))
    st = np.sqrt(np.maximum(0.0, 1.0 - ct * ct))
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    e = np.zeros_like(axis)
    e[np.arange(axis.shape[0]), np.argmin(np.abs(axis), axis=1)] = 1.0
    u = e - (e * axis).sum(1)[:, None] * axis
    u /= np.sqrt((u * u).sum(1))[:, None]
    w = np.cross(axis, u)
    return (ct[None, :, None] * axis[:, None, :] + (st * np.cos(phi))[None, :, None] * u[:, None, :]
            + (st * np.sin(phi))[None, :, None] * w[:, None, :])


def thickness_rays(mesh, direction='in', n_rays=1, cone_angle=120.0):
    """The rays of thickness(): (vertex ids (m,), origins (m,3) float64, directions (m, n_rays, 3) float64) for the mesh's valid vertices
    (those a face refers to and whose normal is a finite non-zero vector)."""
    if direction not in ('in', 'out'):
        raise ValueError("direction must be 'in' or 'out'")
    if int(n_rays) < 1 or not (0.0 < float(cone_angle) <= 360.0):
        raise ValueError('n_rays must be at least 1 and cone_angle within (0, 360]')
    pos = np.asarray(mesh.vertices, np.float32)
    nrm = np.asarray(mesh.vertex_normals, np.float64)
    valid = np.zeros(pos.shape[0], bool)
    valid[np.asarray(mesh.faces).ravel()] = True
    if hasattr(mesh, 'valid_vertex_mask'):
        valid &= np.asarray(mesh.valid_vertex_mask())[:pos.shape[0]]
    length = np.sqrt((nrm * nrm).sum(1))
    valid &= np.isfinite(length) & (length > 0)
    ids = np.flatnonzero(valid)
    axis = nrm[ids] / length[ids, None]
    if direction == 'in':
        axis = -axis
    return ids, pos[ids].astype(np.float64), cone_directions(axis, n_rays, cone_angle)


def thickness(mesh, direction='in', n_rays=1, cone_angle=120.0, t_max=np.inf, context=None, device=0):
    """The local thickness of the structure a mesh encloses (direction='in') or of the gap around it ('out'), per vertex:
    dict(thickness (M,) float64, n_valid (M,) int32, face (M,) int32) over the mesh's M vertex slots.

    From every valid vertex (one a face refers to, with a finite non-zero normal) rays start at its float32 position and pass over the
    faces of the vertex itself (skip_vertex = its id).  The axis is minus (direction='in') or plus ('out') the vertex's row of
    `mesh.vertex_normals`, widened to float64 and normalised.  With n_rays = 1 the one ray runs along the axis; with n_rays = K > 1 the
    directions are a spherical-Fibonacci cap of full opening angle `cone_angle` (degrees) about it:
        cos theta_k = 1 - (k + 1/2) / K (1 - cos(cone_angle / 2)),  phi_k = k pi (3 - sqrt 5),  k = 0 .. K - 1,
        d_k = cos theta_k axis + sin theta_k (cos phi_k u + sin phi_k w),
    where u = e - (e.axis) axis, normalised, e is the coordinate axis along which the axis has its smallest component in magnitude,
    and w = axis x u.  A ray is valid if it hits a face within t_max and leaves through that face's back (for an inward ray inside an
    outward-oriented surface: the far wall seen from within).  thickness = the median of t over the vertex's valid rays (directions
    have unit length, so t is a length), NaN where there is none; n_valid = their number; face = the face hit by the valid ray with
    the lower median t, -1 where there is none.
    The rays are built on the host and cast in chunks of at most 2^22.  mesh: a TriMesh / MembraneMesh.  context: a RayContext to use
    (it holds this mesh afterwards); one is made and closed otherwise."""
    return _thickness(mesh, direction, n_rays, cone_angle, t_max, context, device)[0]


def _thickness(mesh, direction, n_rays, cone_angle, t_max, context, device):
    """thickness() and the ids of the valid vertices its rays started from"""
    ids, origins, dirs = thickness_rays(mesh, direction, n_rays, cone_angle)
    pos, faces = _mesh_arrays(mesh)
    M, K = pos.shape[0], int(n_rays)
    out = dict(thickness=np.full(M, np.nan), n_valid=np.zeros(M, np.int32), face=np.full(M, -1, np.int32))
    own = context is None
    ctx = RayContext(device) if own else context
    try:
        ctx.set_mesh(pos, faces)
        step = max(1, MAX_RAYS_PER_CALL // K)
        for s in range(0, ids.size, step):
            e = min(ids.size, s + step)
            r = ctx.cast(np.repeat(origins[s:e], K, axis=0), dirs[s:e].reshape(-1, 3), skip_vertex=np.repeat(ids[s:e], K), t_max=t_max)
            ok = ((r['face'] >= 0) & r['exits']).reshape(-1, K)
            t = np.where(ok, r['t'].reshape(-1, K), np.inf)
            n = ok.sum(1)
            order = np.argsort(t, axis=1, kind='stable')
            ts = np.take_along_axis(t, order, axis=1)
            rows, some = np.arange(e - s), n > 0
            lo, hi = np.maximum(n - 1, 0) // 2, n // 2                  # the two middle ranks (equal for an odd count)
            with np.errstate(invalid='ignore'):
                med = 0.5 * (ts[rows, lo] + ts[rows, np.minimum(hi, K - 1)])
            out['thickness'][ids[s:e]] = np.where(some, med, np.nan)
            out['n_valid'][ids[s:e]] = n
            out['face'][ids[s:e]] = np.where(some, r['face'].reshape(-1, K)[rows, order[rows, lo]], -1)
    finally:
        if own:
            ctx.close()
    return out, ids


def inside(points, mesh, direction=DEFAULT_DIRECTION, context=None, device=0):
    """Whether each point lies inside a closed mesh, from the parity of the faces a ray from it hits along `direction` (one fixed
    direction for all points): (n,) bool.  A ray that meets an edge or a vertex in rounded arithmetic counts every face of the fan
    (csrc/nw_rays_core.h), so a point whose ray does may get the wrong parity: the default direction is along no lattice direction,
    which makes that rare, not impossible.  points: (n,3).  mesh: a TriMesh / MembraneMesh or (vertices, faces)."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    d = np.asarray(direction, np.float64).reshape(3)
    pos, faces = _mesh_arrays(mesh)
    out = np.zeros(p.shape[0], bool)
    own = context is None
    ctx = RayContext(device) if own else context
    try:
        ctx.set_mesh(pos, faces)
        for s in range(0, p.shape[0], MAX_RAYS_PER_CALL):
            e = min(p.shape[0], s + MAX_RAYS_PER_CALL)
            out[s:e] = (ctx.cast(p[s:e], np.broadcast_to(d, (e - s, 3)), count=True)['hits'] & 1) != 0
    finally:
        if own:
            ctx.close()
    return out


class MeshThickness(object):
    """Recipe-module surface for the local thickness of a fitted surface, in the plain-attribute style of ShrinkwrapMembrane: the mesh
    under `input` -> under `output` a table with one row per valid vertex: x y z (its position), thickness (nm, NaN where no ray was
    valid) and n_valid.  PYME is not in the reference tree: the traits and the columns here are this project's own."""

    def __init__(self, **kw):
        self.input, self.output = 'membrane', 'thickness'
        self.direction, self.n_rays, self.cone_angle, self.t_max = 'in', 1, 120.0, np.inf
        self.device = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)

    def execute(self, namespace):
        mesh = namespace[self.input]
        r, ids = _thickness(mesh, self.direction, int(self.n_rays), float(self.cone_angle), float(self.t_max), None, self.device)
        pos = np.asarray(mesh.vertices, np.float32)[ids]
        table = {'x': pos[:, 0].copy(), 'y': pos[:, 1].copy(), 'z': pos[:, 2].copy(), 'thickness': r['thickness'][ids], 'n_valid': r['n_valid'][ids]}
        namespace[self.output] = table
        return table
