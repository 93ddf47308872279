"""
The exact distance between two triangle meshes, and the contact sites between two fitted membranes: ctypes binding of
include/nw_proximity.h (kernels in libnanowrap_hip.so, csrc/nw_proximity.hip) and what sits on top of it.

Of two fitted membranes -- ER against mitochondria, ER against plasma membrane, two vesicles -- users ask where they come within d nm
of each other, how large that patch is and what the gap is there.  distance_to_mesh of A's vertices against B answers another
question: it is the distance from A's vertices, so it overestimates the gap wherever the nearest approach lies inside a face or
between two edges, and it is positive for two surfaces that pass through each other between their vertices.  PYME is not part of the
reference tree and upstream has no such module, so nothing here mirrors reference code: the definition is this project's own and is
written down in csrc/nw_proximity_core.h (triangle against triangle in float64 on the float32 vertices: vertex-face, edge-edge and
piercing).

    ProximityContext   one nwm_ctx: set_mesh (mesh B) once, query (mesh A) as often as needed
    mesh_distance      one call: two meshes in, per face of A the distance, the partner face of B, the kind of pair, closest points
    contact_sites      the faces of each mesh within a distance of the other, their edge-connected patches and areas
    MembraneContacts   the recipe-module surface: two meshes -> a table with one row per in-contact face of A

Everything runs on the device; there is no host fallback: without a GPU the context cannot be made and every entry raises.
"""
import ctypes

import numpy as np

from . import _lib

SYMBOLS = ['nwm_abi_version', 'nwm_create', 'nwm_destroy', 'nwm_last_error', 'nwm_set_mesh', 'nwm_query']
ABI_VERSION = 1
NWM_OK, NWM_ERR_BADARG, NWM_ERR_HIP, NWM_ERR_NONFINITE, NWM_ERR_NOMEM, NWM_ERR_NOMESH = 0, -1, -2, -3, -4, -5
ERRORS = {NWM_ERR_BADARG: 'bad argument', NWM_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWM_ERR_NONFINITE: 'non-finite coordinate',
          NWM_ERR_NOMEM: 'out of device memory', NWM_ERR_NOMESH: 'the context holds no mesh'}
NWM_KIND_PIERCED, NWM_KIND_EDGE_EDGE = 0, 7   # kinds: 0 pierced, 1-3 corner k of A, 4-6 corner k of B, 7 + 3i + j edge i of A and edge j of B
NWM_INFO_WORDS = 7
NWM_INFO_IN_BAND, NWM_INFO_AT_ZERO, NWM_INFO_RINGS, NWM_INFO_CENTROIDS, NWM_INFO_TESTS, NWM_INFO_CELLS, NWM_INFO_CELL_SIZE = range(7)

_L = None


def load():
    """The library's nwm_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        _L = _lib.load_entry_points(SYMBOLS, {
            'nwm_abi_version': [], 'nwm_create': [i32, ctypes.POINTER(vp)], 'nwm_destroy': [vp], 'nwm_last_error': [vp],
            'nwm_set_mesh': [vp, vp, i64, vp, i64, f64],
            'nwm_query': [vp, vp, i64, vp, i64, f64, vp, vp, vp, vp, vp, vp]},
            'nwm_abi_version', ABI_VERSION, 'nw_proximity')
    return _L


_p = _lib.ptr


def _mesh(mesh):
    """(positions float32, faces int32) of a TriMesh / MembraneMesh or a (vertices, faces) pair, as distance._mesh_arrays takes them"""
    from .distance import _mesh_arrays
    pos, faces, _ = _mesh_arrays(mesh, False)
    return pos, faces


class ProximityContext(_lib.QueryContext):
    """One nwm_ctx: mesh B taken in once by set_mesh, its centroid grid kept on the device, and any number of meshes A queried against it."""
    prefix, errors, gpu_only, load = 'nwm_', ERRORS, 'the distance between two meshes runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_faces = 0
        self.info = None

    def set_mesh(self, vertices, faces=None, cell_size=0.0):
        """Take mesh B in: a TriMesh / MembraneMesh (faces None) or float32 vertices and int32 faces.  cell_size: the cell size every
        query's grid starts from; 0 leaves it to the unit (include/nw_proximity.h)."""
        pos, f = _mesh(vertices if faces is None else (vertices, faces))
        self.n_faces = 0
        self.check(self.L.nwm_set_mesh(self.h, _p(pos), pos.shape[0], _p(f), f.shape[0], float(cell_size)), 'nwm_set_mesh')
        self.n_faces = f.shape[0]
        return self

    def query(self, vertices, faces=None, band=np.inf, return_closest=False):
        """Mesh A against the mesh in the context, per face of A: dict(distance (F,) float64, +inf out of band; partner (F,) int32, the
        nearest face of B, -1 out of band; kind (F,) int32; with return_closest closest_a, closest_b (F,3) float64, NaN out of band;
        info: the call's counters)."""
        pos, f = _mesh(vertices if faces is None else (vertices, faces))
        n = f.shape[0]
        out = dict(distance=np.empty(n, np.float64), partner=np.empty(n, np.int32), kind=np.empty(n, np.int32))
        if return_closest:
            out['closest_a'], out['closest_b'] = np.empty((n, 3), np.float64), np.empty((n, 3), np.float64)
        info = np.zeros(NWM_INFO_WORDS, np.int64)
        self.check(self.L.nwm_query(self.h, _p(pos), pos.shape[0], _p(f), n, float(band), _p(out['distance']), _p(out['partner']), _p(out['kind']),
                                    _p(out.get('closest_a')), _p(out.get('closest_b')), _p(info)), 'nwm_query')
        self.info = out['info'] = dict(in_band=int(info[NWM_INFO_IN_BAND]), at_zero=int(info[NWM_INFO_AT_ZERO]), faces=n, rings=int(info[NWM_INFO_RINGS]),
                                       centroids=int(info[NWM_INFO_CENTROIDS]), tests=int(info[NWM_INFO_TESTS]), cells=int(info[NWM_INFO_CELLS]),
                                       cell_size=float(info[NWM_INFO_CELL_SIZE:NWM_INFO_CELL_SIZE + 1].view(np.float64)[0]))
        return out


def mesh_distance(mesh_a, mesh_b, band=np.inf, return_closest=False, context=None, device=0):
    """The exact distance of every face of mesh_a from mesh_b's triangles: dict(distance, partner, kind[, closest_a, closest_b], info)
    (ProximityContext.query).  band: faces farther than this are out of band (distance +inf, partner -1, kind -1) and cost a few rings
    of the walk only.  Meshes: a TriMesh / MembraneMesh or (vertices, faces).  The result is not promised to be symmetric bit for bit
    in its two arguments: B against A is another call.  context: a ProximityContext to use (it holds mesh_b afterwards); one is made
    and closed otherwise."""
    own = context is None
    ctx = ProximityContext(device) if own else context
    try:
        return ctx.set_mesh(mesh_b).query(mesh_a, band=band, return_closest=return_closest)
    finally:
        if own:
            ctx.close()


def _contact_side(pctx, sctx, mesh, distance):
    """contact_sites' entries for one mesh against the mesh in pctx"""
    from .distance import mesh_twins
    pos, faces = _mesh(mesh)
    r = pctx.query(pos, faces, band=distance, return_closest=True)
    mask = r['partner'] >= 0
    twin = mesh_twins(faces, pos.shape[0])
    label, n = sctx.label_faces(faces, twin, mask.astype(np.uint8))
    st = sctx.component_stats(pos, faces, twin, label, n)
    patch_min = np.full(n, np.inf)
    np.minimum.at(patch_min, label[mask], r['distance'][mask])
    return dict(faces=mask, area=float(st['area'].sum()), patches=label, patch_area=st['area'], patch_min_distance=patch_min,
                patch_faces=st['faces'], n_crossing=int((r['kind'] == NWM_KIND_PIERCED).sum())), r


def contact_sites(mesh_a, mesh_b, distance=30.0, device=0):
    """Where two fitted membranes come within `distance` nm of each other.  dict with, for mesh_a:
        faces_a (F,) bool            the face is within `distance` of mesh_b (its exact face-to-mesh distance, mesh_distance)
        area_a                       the area of those faces
        patches_a (F,) int32         the patch of each in-contact face, -1 outside: an edge-connected set of in-contact faces, numbered
                                     in order of their smallest face id
        patch_area_a, patch_min_distance_a, patch_faces_a    per patch
        n_crossing_a                 the faces at distance 0 because an edge pierces a face (kind 0)
        result_a                     mesh_distance's dict for mesh_a against mesh_b, closest points included
    and the same entries with _b from the second call, mesh_b against mesh_a.  Labels and areas come from nws_label_faces(mask=...) and
    nws_component_stats (include/nw_surgery.h): area has no kernel of its own here.  Meshes: a TriMesh / MembraneMesh or
    (vertices, faces); a mesh with a non-manifold edge has no half-edge twins and raises."""
    from .surgery import SurgeryContext
    pctx, sctx = ProximityContext(device), None
    try:
        sctx = SurgeryContext(device)
        out = {}
        for tag, mine, other in (('a', mesh_a, mesh_b), ('b', mesh_b, mesh_a)):
            pctx.set_mesh(other)
            side, r = _contact_side(pctx, sctx, mine, float(distance))
            for k, v in side.items():
                out[k + '_' + tag] = v
            out['result_' + tag] = r
        out['distance'] = float(distance)
        return out
    finally:
        if sctx is not None:
            sctx.close()
        pctx.close()


class MembraneContacts(object):
    """Recipe-module surface for the contact sites of two fitted surfaces, in the plain-attribute style of MeshThickness: the meshes
    under `input_a` and `input_b` -> under `output` a table with one row per face of A within `contact_distance` nm of B: x y z (the
    closest point on A), distance (nm), partner (the nearest face of B) and patch (the face's contact patch).  The table's `metadata`
    carries the areas: area_a, area_b, patch_area_a, patch_area_b, n_crossing_a, n_crossing_b, contact_distance.  PYME is not in the
    reference tree: the traits and the columns here are this project's own."""

    def __init__(self, **kw):
        self.input_a, self.input_b, self.output = 'membrane', 'membrane2', 'contacts'
        self.contact_distance = 30.0
        self.device = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)

    def execute(self, namespace):
        c = contact_sites(namespace[self.input_a], namespace[self.input_b], float(self.contact_distance), device=self.device)
        r, rows = c['result_a'], np.flatnonzero(c['faces_a'])
        at = r['closest_a'][rows]
        table = {'x': at[:, 0].copy(), 'y': at[:, 1].copy(), 'z': at[:, 2].copy(), 'distance': r['distance'][rows], 'partner': r['partner'][rows],
                 'patch': c['patches_a'][rows],
                 'metadata': {'area_a': c['area_a'], 'area_b': c['area_b'], 'patch_area_a': c['patch_area_a'], 'patch_area_b': c['patch_area_b'],
                              'n_crossing_a': c['n_crossing_a'], 'n_crossing_b': c['n_crossing_b'], 'contact_distance': float(self.contact_distance)}}
        namespace[self.output] = table
        return table
